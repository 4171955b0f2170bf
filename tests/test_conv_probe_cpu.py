"""CPU side of the convolution variant tests (tests/test_gpu_conv_variants.py): the descriptor mirror, the route and feature numbering
shared with csrc/conv.h, and the case table itself (routes, alignment, coverage rows, refusals)."""
import ctypes
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV_H = os.path.join(ROOT, "image-matching-webui_amd", "csrc", "conv.h")
ERR_ARG = -1


def test_descriptor_mirror_matches_the_library(lib):
    from imcui_hip import backend

    assert ctypes.sizeof(backend.ConvDesc) == lib.imcui_hip_conv_desc_bytes()


def _enum(name):
    body = re.search(r"enum " + name + r"\s*\{(.*?)\};", open(CONV_H).read(), re.S).group(1)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b([A-Z][A-Z0-9_]+)\s*=\s*(\d+)", body)}


def test_route_and_feature_numbering_matches_conv_h():
    import test_gpu_conv_variants as t

    from imcui_hip import backend

    kinds = _enum("ConvRouteKind")
    nkind = kinds.pop("CR_NKIND")
    kinds = {k[3:].lower(): v for k, v in kinds.items()}
    assert kinds == backend.CONV_ROUTE_KINDS
    assert nkind == max(kinds.values()) + 1
    feats = {k[3:].lower(): v for k, v in _enum("ConvFeature").items()}
    assert feats == backend.CONV_FEATURES == t.FEATURES
    assert sorted(feats.values()) == [1 << i for i in range(10)]
    assert re.search(r"#define CONV_ROUTE\(kind\) \(kind\)", open(CONV_H).read())
    assert backend.conv_route("tall_single") == 7 and backend.conv_route_name(9) == "fused_tall"
    assert backend.conv_feature_names(2 | 64) == ["resid", "cout_live"]


def test_probe_refuses_null_descriptor_and_handle(lib):
    from imcui_hip import backend

    d = backend.ConvDesc()
    assert lib.imcui_hip_conv_probe_f32(None, ctypes.byref(d), None) == ERR_ARG
    assert lib.imcui_hip_conv_probe_f32(None, None, None) == ERR_ARG
    assert lib.imcui_hip_conv_last_route(None) == -1
    assert lib.imcui_hip_conv_route_counts(None, None, 0) == -1 and lib.imcui_hip_conv_route_features(None, None, 0) == -1
    assert lib.imcui_hip_conv_route_reset(None) == ERR_ARG


def test_conv_weights_pack_round_trips(lib):
    """ConvWeights: the packed f32 layout and the hi / lo planes hold the OIHW weights where conv.hip reads them; zero padding to
    cout_pad, the first cin_used input channels only."""
    from imcui_hip import backend

    g = torch.Generator().manual_seed(5)
    w = torch.randn(100, 96, 3, 3, generator=g) + torch.arange(100.0)[:, None, None, None] * 0.01
    b = torch.randn(100, generator=g)
    wt = backend.ConvWeights(w, b, torch.device("cpu"), cout_pad=128, cin_used=64)
    assert (wt.Cout, wt.Cin) == (128, 64) and wt.bias.shape == (128,) and (wt.bias[100:] == 0).all()
    want = torch.zeros(128, 64, 9, dtype=torch.float64)
    want[:100] = w[:, :64].reshape(100, 64, 9).double()
    # f32: [Cin/32][9][8 cq][Cout][4]  <-  w[co][ch*32 + cq*4 + j][tap]
    p = torch.from_numpy(wt.packed_host).double().reshape(2, 9, 8, 128, 4).permute(3, 0, 2, 4, 1).reshape(128, 64, 9)
    assert torch.equal(p, want)
    # split: [Cin/32][9][4 octets][Cout][8]  <-  w[co][ch*32 + oc*8 + j][tap] * 2^e, hi + lo
    planes = (wt.hi_host.view(np.float16).astype(np.float64) + wt.lo_host.view(np.float16).astype(np.float64)) * wt.scale
    s = torch.from_numpy(planes).reshape(2, 9, 4, 128, 8).permute(3, 0, 2, 4, 1).reshape(128, 64, 9)
    assert (s - want).abs().max().item() <= 2.0**-21 * want.abs().max().item()
    assert (s[100:] == 0).all()
    assert torch.equal(backend.ConvWeights.first_layer(w[:64, :1])[4], w[:64, 0, 1, 1])


def expected_route(c, opts):
    """The routing rules of csrc/conv.hip restated on the host."""
    narrow, tall = opts.get("conv_narrow", 0), opts.get("conv_tall", 1)
    if c["entry"] == "f32":
        return "f32"
    if c["entry"] == "conv1a":
        return "conv1a"
    if c["entry"] == "fused":
        return "fused_tall" if tall >= 1 else "fused_8row"
    B, H, W, cout = c["B"], c["H"], c["W"], c["cout"]
    live = c.get("cout_live", 0) or cout
    narrow_only = narrow == 1
    if narrow == 0 and not c.get("head") and cout % 128 == 0 and -(-W // 32) * -(-H // 8) * (cout // 128) * B < 256:
        narrow_only = True
    wide = cout % 128 == 0 and not narrow_only
    sfx = "_single" if c.get("single") else ""
    if not wide and live == cout and tall >= 2:
        return "tall" + sfx
    return ("split_n4" if wide else "split_n2") + sfx


def workgroups(c, route):
    th, tw, cw = {"f32": (8, 16, 64), "tall": (16, 32, 64), "tall_single": (16, 32, 64), "fused_tall": (16, 32, 64), "split_n4": (8, 32, 128),
                  "split_n4_single": (8, 32, 128)}.get(route, (8, 32, 64))  # fmt: skip
    return -(-c["W"] // tw) * -(-c["H"] // th) * (c.get("cout", 64) // cw) * c["B"]


RULES = {  # refusal rule -> what the case must violate (conv3x3_split_launch)
    "pool_resid": lambda c, o: c.get("pool") and c.get("resid"),
    "resid2_alone": lambda c, o: c.get("resid2") and not c.get("resid"),
    "cin_mod_32": lambda c, o: c["cin"] % 32 != 0,
    "cout_mod_64": lambda c, o: c["cout"] % 64 != 0,
    "pool_odd": lambda c, o: c.get("pool") and (c["H"] % 2 or c["W"] % 2),
    "cin_stride_small": lambda c, o: 0 < c.get("cin_stride", 0) < c["cin"],
    "cin_stride_mod_4": lambda c, o: c.get("cin_stride", 0) >= c["cin"] and c["cin_stride"] % 4 != 0,
    "null_out": lambda c, o: c.get("null_out") and not c.get("head"),
    "head_cout": lambda c, o: c.get("head") and c["cout"] != 128,
    "head_pool": lambda c, o: c.get("head") and c.get("pool"),
    "head_resid": lambda c, o: c.get("head") and c.get("resid"),
    "head_act": lambda c, o: c.get("head") and c.get("act") != 1,
    "head_cout_live": lambda c, o: c.get("head") and 0 < c.get("cout_live", 0) < c["cout"],
    "head_narrow": lambda c, o: c.get("head") and o.get("conv_narrow") == 1,
    "head_pointer": lambda c, o: c.get("head") and c.get("missing") in ("head_w", "head_b", "head_pts", "head_conf"),
}


def _violations(c, o):
    return {k for k, f in RULES.items() if f(c, o)}


def test_case_table_is_well_formed():
    import test_gpu_conv_variants as t

    from imcui_hip import backend

    assert len({c["id"] for c in t.CASES}) == len(t.CASES)
    launched = [c for c in t.CASES if not c.get("refusal")]
    for c in launched:
        o = t.case_options(c)
        assert c["route"] in backend.CONV_ROUTE_KINDS and c["route"] != "none", c["id"]
        assert expected_route(c, o) == c["route"], (c["id"], expected_route(c, o))
        assert c["entry"] != "split" or not _violations(c, o), (c["id"], _violations(c, o))
        if c["entry"] in ("f32", "split"):
            assert c["cin"] % 32 == 0 and c["cout"] % 64 == 0, c["id"]
            assert c.get("cin_stride", 0) == 0 or (c["cin_stride"] >= c["cin"] and c["cin_stride"] % 4 == 0), c["id"]
            assert c["route"] not in ("split_n4", "split_n4_single") or c["cout"] % 128 == 0, c["id"]
            assert c["entry"] == "split" or not (c.get("resid") or c.get("single") or c.get("relu_in") or c.get("act", 0) > 1), c["id"]
        if c.get("pool"):
            assert c["H"] % 2 == 0 and c["W"] % 2 == 0, c["id"]
            assert -(-(c["W"] // 2) // 16) > 1 and (c["W"] // 2) % 16 and (c["H"] // 2) % 4, f"{c['id']}: pooled tiles must be ragged"
        elif c["H"] > 8:
            th, tw = (16, 32) if "tall" in c["route"] else (8, 16) if c["route"] == "f32" else (8, 32)
            assert c["H"] > th and c["W"] > tw and c["H"] % th and c["W"] % tw, f"{c['id']}: more than one tile and a ragged edge both ways"
        assert c["B"] in (2, 3), c["id"]
    for c in t.CASES:
        if c.get("refusal"):
            o = t.case_options(c)
            assert c["refusal"] == ERR_ARG and c["entry"] == "split"
            assert _violations(c, o) == {c["rule"]}, (c["id"], _violations(c, o))
    assert {c["rule"] for c in t.CASES if c.get("refusal")} == set(RULES)


def test_case_table_has_every_coverage_row():
    import test_gpu_conv_variants as t

    launched = [c for c in t.CASES if not c.get("refusal")]
    plain = [c for c in launched if c["entry"] == "split" and not c.get("pool")]
    assert {1, 31} <= {c["W"] % 32 for c in plain} and {1, 7} <= {c["H"] % 8 for c in plain}
    assert any(c["H"] == 3 and c["W"] == 5 for c in launched)
    assert {32, 64, 96} <= {c["cin"] for c in launched if "cin" in c} and {64, 128, 192, 256} <= {c["cout"] for c in launched if "cout" in c}
    nwg = {workgroups(c, c["route"]) % 8 == 0 for c in launched if c["entry"] == "split"}
    assert nwg == {True, False}, "xcd_remap: grids that are and are not a multiple of 8 workgroups"
    F = t.FEATURES

    def rows(route):
        return [(c.get("act", 0), t.case_features(c), c) for c in launched if c["route"] == route]

    assert {(c.get("act", 0), bool(c.get("pool"))) for c in launched if c["route"] == "f32"} == {(0, False), (1, False), (0, True), (1, True)}
    for route in ("split_n2", "split_n4"):
        r = rows(route)
        assert {a for a, _, _ in r} == {0, 1, 2}, route
        feats = [f for _, f, _ in r]
        for need in (F["pool"], F["resid"], F["resid"] | F["resid2"], F["cin_stride"], F["cout_live"]):
            assert any(f & need == need for f in feats), (route, need)
        assert {a for a, f, _ in r if f & F["relu_in"]} == {0, 1, 2}, f"{route}: relu codes 4, 5 and 6"
        assert {(c["cin"], c.get("cin_stride")) for _, f, c in r if f & F["cin_stride"]} == {(224, 256)}
        assert {(c["cout"], c["cout_live"]) for _, f, c in r if f & F["cout_live"]} >= {(256, 224), (256, 200)}
    for route in ("split_n2_single", "split_n4_single"):
        assert any(f & (F["resid"] | F["relu_in"]) == F["resid"] | F["relu_in"] for _, f, _ in rows(route)), route
    for route in ("tall", "tall_single"):
        r = rows(route)
        assert {c["cout"] for _, _, c in r} == {64, 192}, route
        for need in (F["pool"], F["resid"] | F["resid2"], F["relu_in"], F["cin_stride"]):
            assert any(f & need == need for _, f, _ in r), (route, need)
    assert any(t.case_options(c).get("conv_tall") == 2 and c.get("cout_live") and c["route"] == "split_n2" for c in launched)
    assert any(t.case_options(c).get("conv_narrow") == 0 and c["route"] == "split_n2" and c["cout"] % 128 == 0 for c in launched)
    for route in ("split_n4", "split_n4_single"):
        heads = {(c.get("head_out", True), c.get("head_raw", True)) for _, _, c in rows(route) if c.get("head") and not c.get("zero")}
        assert heads == {(True, True), (False, True), (True, False)}, route
    assert any(c.get("zero") for c in launched)
    assert {(c["route"], bool(c.get("pool"))) for c in launched if c["entry"] == "fused"} == {(r, p) for r in ("fused_tall", "fused_8row") for p in (False, True)}
    assert any(c["route"] == "conv1a" for c in launched)
    cov = t.covered_pairs()
    assert ("split_n4", 0) in cov and ("split_n4", F["resid2"]) in cov and ("tall_single", F["pool"]) in cov
