"""CPU side of the fused-FFN variant tests (tests/test_gpu_ffn_variants.py): the descriptor mirror, the route numbering shared with
csrc/ffn.h, the shape of the case table, and -- with no device involved -- the float64 reference, the emulation of the kernel's operand
rounding and the wrong references of that file: every wrong reference must lie farther than 4 x the bar from the right one on the
case's own inputs, or the case could not tell them apart."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FFN_H = os.path.join(ROOT, "image-matching-webui_amd", "csrc", "ffn.h")


def test_descriptor_mirror_matches_the_library(lib):
    from imcui_hip import backend

    assert ctypes.sizeof(backend.FfnDesc) == lib.imcui_hip_ffn_desc_bytes()


def test_descriptor_has_every_launcher_field_but_dbg():
    from imcui_hip import backend

    body = re.search(r"struct FfnP\s*\{(.*?)\n\};", open(FFN_H).read(), re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = set()
    for decl in body.split(";"):
        names |= {m.group(1) for m in re.finditer(r"\*?\s*\b([A-Za-z_]\w*)\s*=\s*[^,]+", decl)}
    assert "dbg" in names and len(names) == 19, sorted(names)
    assert names - {"dbg"} == {n for n, _ in backend.FfnDesc._fields_}


def test_route_numbering_matches_ffn_h():
    from imcui_hip import backend

    src = open(FFN_H).read()
    body = re.sub(r"//[^\n]*", "", re.search(r"enum FfnRouteKind\s*\{(.*?)\};", src, re.S).group(1))
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b([A-Z][A-Z0-9_]+)\s*=\s*(\d+)", body)}
    nkind = enum.pop("FR_NKIND")
    kinds = {k[3:].lower(): v for k, v in enum.items()}
    assert kinds == backend.FFN_ROUTE_KINDS == {"t128_rolled": 0, "t128": 1, "t64": 2, "t32": 3}
    assert nkind == max(kinds.values()) + 1
    assert re.search(r"#define FFN_ROUTE\(kind, act\) \(1 \+ \(kind\) \* 4 \+ \(act\)\)", src)
    assert backend.ffn_route("t128_rolled", 0) == 1 and backend.ffn_route("t64", 3) == 1 + 2 * 4 + 3 and backend.ffn_route("t32", 3) == 16
    assert backend.ffn_route_name(backend.ffn_route("t32", 2)) == "t32/act2" and backend.ffn_route_name(0) == "none"
    routes = [backend.ffn_route(k, a) for k in kinds for a in range(4)]
    assert sorted(routes) == list(range(1, 17)), "the formula numbers the sixteen instantiations 1 .. 16, 0 is none"


def test_case_table_is_well_formed():
    import test_gpu_ffn_variants as t

    from imcui_hip import backend

    assert len({c["id"] for c in t.CASES}) == len(t.CASES)
    cov = t.covered_routes()
    assert cov == {backend.ffn_route(k, a) for k in ("t128", "t64", "t32") for a in range(4)}, "all twelve shipped instantiations, and only those"
    for c in t.CASES:
        if c["kind"] == "refusal":
            assert c["expect"] in (0, t.ERR_ARG, t.ERR_UNSUPPORTED) and t.case_route(c) is None
            continue
        assert c["tile"] in (128, 64, 32) or (c["tile"] == 0 and c["kind"] == "auto"), c["id"]
        assert c["form"] in t.FORMS[c["act"]], c["id"]
        if c["kind"] == "ragged":
            assert c["R"] % 128 == 0 and c["M"] == len(c["cnt"]) * c["R"] and all(0 <= n <= c["R"] for n in c["cnt"]), c["id"]
            assert c["active"] is None or len(c["active"]) == len(c["cnt"]) // 2, c["id"]
    # the automatic rule: tile 32, 64, 64, 128 at the two thresholds
    assert [t.auto_tile(M) for M in (8192, 8193, 16384, 16385)] == [32, 64, 64, 128]
    dense = {(c["act"], c["form"], c["M"], c["tile"]) for c in t.CASES if c["kind"] == "dense"}
    assert dense == {(a, f, M, tl) for a in range(4) for f in t.FORMS[a] for M in t.DENSE_M for tl in t.TILES}


def test_plane_unpacking_and_split_emulation(lib):
    """The emulation's operands: the unpacked planes are the weights to 2^-21 of the largest one (hi + lo of w 2^e, two nearest f16
    roundings), W2's in the original K order; split2's hi + lo pair is the value to 2^-21 relative, hi never above |v|, and saturates."""
    import test_gpu_ffn_variants as t

    w = t.wset(1)
    for name, planes, N, perm in (("w1", w["p1"], 512, False), ("w2", w["p2"], 256, True)):
        u = t.unpack_planes(planes, N, 512, permuted=perm)
        assert (u - w[name].double()).abs().max().item() <= 2.0**-21 * w[name].abs().max().item(), name
    assert sorted(t.PERM.tolist()) == list(range(512))
    g = torch.Generator().manual_seed(5)
    v = torch.cat([torch.randn(4096, generator=g) * 3, torch.randn(4096, generator=g) * 1e4, torch.tensor([0.0, 1.0, -1.0, 65504.0, -3.3e4])])
    s = t.split2_emu(v.double())
    assert torch.isfinite(s).all()
    # lo is the nearest f16 of a remainder below one ulp of hi: 2^-21 relative, or half a step of the f16 subnormals (2^-25)
    assert ((s - v.double()).abs() <= torch.clamp(2.0**-21 * v.abs().double(), min=2.0**-25)).all()
    # hi saturates instead of overflowing: 65504 + the remainder, still finite
    assert t.split2_emu(torch.tensor([7e4, -1e5]).double()).tolist() == [7e4, -1e5]


def _datasets(t):
    """One case per data key: the cases that share a key share inputs, reference and wrong references."""
    seen = {}
    for c in t.CASES:
        if c["kind"] != "refusal":
            seen.setdefault(c["data"], c)
    return list(seen.values())


def test_wrong_references_are_told_apart_on_every_case():
    """For every data set of the GPU table: each wrong reference is farther than 4 x bar from the right one on the rows the case compares
    (for the ragged cases: on the valid rows of every (cnt, active) combination in the table)."""
    import test_gpu_ffn_variants as t

    for c in _datasets(t):
        e = t._expect(c)
        assert torch.isfinite(e["ref"]).all(), c["id"]
        if c["kind"] == "ragged":
            combos = {tuple(map(bool, t.ragged_masks(k["cnt"], k["active"], 128, k["R"])[0].tolist())) for k in t.CASES if k.get("data") == c["data"]}
            rowsets = [torch.tensor(m) for m in combos if any(m)]
        else:
            rowsets = [None]
        for rows in rowsets:
            d = t.wrong_distances(e, rows)
            assert set(d) == set(t.wrong_names(c["act"], c["form"], c["kind"] == "eps"))
            n = "all" if rows is None else int(rows.sum())
            print(f"[ffn-cpu] {c['data']} rows {n} bar {e['bar']:.1e}: " + ", ".join(f"{k} {v:.1e}" for k, v in d.items()))
            for k, v in d.items():
                assert v > 4 * e["bar"], f"{c['data']} (rows {n}): the wrong reference '{k}' is only {v:.2e} away, bar {e['bar']:.1e}"


def test_emulated_operand_rounding_stays_under_the_bar_at_unit_scale():
    """e_emu (float64 on the operands rounded as the kernel rounds them, against plain float64) of the unit-scale data sets that carry
    it -- M = 160 of every activation and form, and the two hidden-range cases: 2 e_emu < 3e-6, so the 3e-6 bar stands everywhere but
    in the scaled epsilon cases, whose e_emu and bar are printed."""
    import test_gpu_ffn_variants as t

    n = 0
    for c in _datasets(t):
        if c["kind"] == "eps":
            e = t._expect(c)
            print(f"[ffn-cpu] {c['data']}: e_emu {e['e_emu']:.2e} -> bar {e['bar']:.2e}")
            assert e["bar"] == max(t.BAR, 2 * e["e_emu"])
        elif c.get("emu"):
            e = t._expect(c)
            print(f"[ffn-cpu] {c['data']}: e_emu {e['e_emu']:.2e}")
            assert 2 * e["e_emu"] < t.BAR, (c["data"], e["e_emu"])
            n += 1
    assert n == 7 + 2


def test_range_cases_are_scaled_as_documented():
    """The hidden-range cases: the largest hidden activation is between 1.5e4 and 3.3e4, inside the f16 range."""
    import test_gpu_ffn_variants as t

    for act in (1, 3):
        w = t.wset(act, "range")
        x, ctx = t.inputs(f"range_a{act}", 160)
        h = torch.cat([x, ctx], 1).double() @ w["w1"].double().t() + (w["b1"].double() if act == 1 else 0.0)
        top = torch.relu(h).max().item()
        print(f"[ffn-cpu] range_a{act}: largest hidden activation {top:.3e}")
        assert 1.5e4 <= top <= 3.3e4


def test_ragged_rules():
    """The right rule on the table's counts, and that the table can tell both wrong readings from it at every tile."""
    import test_gpu_ffn_variants as t

    v, u = t.ragged_masks([256, 129, 1, 0], [1, 0], 64, 256)
    assert v.sum().item() == 256 + 129 and v[256 + 128] and not v[256 + 129]
    assert not u[:256].any() and not u[256 : 256 + 192].any() and u[256 + 192 :].all()
    v, u = t.ragged_masks([128, 128, 97, 33], None, 32, 256)
    assert v.sum().item() == 128 + 128 + 97 + 33
    assert u[128:256].all() and not u[512 : 512 + 128].any() and u[512 + 128 : 768].all() and not u[768 : 768 + 64].any() and u[768 + 64 :].all()
    for tile in t.TILES:
        for act in (0, 1):
            told = set()
            for c in t.CASES:
                if c["kind"] == "ragged" and c["tile"] == tile and c["act"] == act:
                    told |= set(t.excluded_rules(c["cnt"], c["active"], tile, c["R"]))
            assert told == set(t.RAGGED_WRONG_RULES), (tile, act, told)
    assert t.excluded_rules([256, 129, 1, 0], None, 128, 256) == ["cnt by pair"]
    assert t.excluded_rules([256, 129, 1, 0], [1, 0], 128, 256) == ["active by sequence"]  # (the pair that could tell the counts is off)
    assert t.excluded_rules([128, 128, 97, 33], [0, 1], 32, 256) == ["cnt by pair", "active by sequence"]
