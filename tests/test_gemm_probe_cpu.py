"""CPU side of the GEMM variant tests (tests/test_gpu_gemm_variants.py): the descriptor mirror, the weight packing the probe uses and
the route and feature numbering shared with csrc/gemm.h."""
import ctypes
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMM_H = os.path.join(ROOT, "image-matching-webui_amd", "csrc", "gemm.h")


def test_descriptor_mirror_matches_the_library(lib):
    from imcui_hip import backend

    assert ctypes.sizeof(backend.GemmDesc) == lib.imcui_hip_gemm_desc_bytes()


def _unpack_planes(hi, lo, scale, N, K):
    """Fragment-major planes [ceil(N/32)][K/16][2][32][8] -> [N, K] float64 (hi + lo) * 2^-e."""
    nf = (N + 31) // 32
    h = hi.view(np.float16).astype(np.float64).reshape(nf, K // 16, 2, 32, 8)
    l = lo.view(np.float16).astype(np.float64).reshape(nf, K // 16, 2, 32, 8)
    w = (h + l).transpose(0, 3, 1, 2, 4).reshape(nf * 32, K) * scale
    return w[:N], w[N:]


def test_conv_weight_packing_round_trips(lib):
    from imcui_hip import backend

    g = torch.Generator().manual_seed(3)
    for cout, cin, k, cin_pad in ((65, 256, 1, 256), (32, 48, 5, 64), (128, 96, 3, 96)):
        w = torch.randn(cout, cin, k, k, generator=g) + torch.arange(cout).float()[:, None, None, None] * 0.01
        wg, _ = backend._conv_gemm_layout(w, torch.zeros(cout), cout, cin_pad)
        hi, lo, sc = backend.pack_linear_split(wg)
        got, pad_rows = _unpack_planes(hi, lo, sc, cout, k * k * cin_pad)
        got = got.reshape(cout, k * k, cin_pad)
        assert np.all(got[:, :, cin:] == 0), "padded input channels must be zero"
        assert np.all(pad_rows == 0), "rows past Cout must be zero"
        oihw = torch.from_numpy(got[:, :, :cin]).reshape(cout, k, k, cin).permute(0, 3, 1, 2)
        err = (oihw - w.double()).abs().max().item() / w.abs().max().item()
        assert err <= 2.0**-22, err


def _enum(name):
    src = open(GEMM_H).read()
    body = re.search(r"enum " + name + r"\s*\{(.*?)\};", src, re.S).group(1)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b([A-Z][A-Z0-9_]+)\s*=\s*(\d+)", body)}


def test_route_numbering_matches_gemm_h():
    from imcui_hip import backend

    kinds = {k[3:].lower(): v for k, v in _enum("GemmRouteKind").items() if k != "GR_NKIND"}
    assert kinds == backend.GEMM_ROUTE_KINDS
    epis = {k[4:].lower(): v for k, v in _enum("GemmEpi").items()}
    assert epis == backend.GEMM_EPI
    assert re.search(r"#define GEMM_ROUTE\(kind, epi\) \(\(kind\) \* 16 \+ \(epi\)\)", open(GEMM_H).read())
    assert backend.gemm_route("wreg_mt1", "qkv_vit") == 17 * 16 + 7


def test_feature_numbering_matches_gemm_h():
    """GemmFeature of gemm.h against backend.GEMM_FEATURES: the same names and bits, every bit single and distinct; the threshold of the
    two-level sum and the kinds with 256-column tiles the case tables derive n_mod_tile / chunk / long_k from."""
    from imcui_hip import backend

    feats = {k[3:].lower(): v for k, v in _enum("GemmFeature").items()}
    assert feats == backend.GEMM_FEATURES
    bits = list(feats.values())
    assert all(b > 0 and b & (b - 1) == 0 for b in bits) and len(set(bits)) == len(bits) and max(bits) < 2**31
    src = open(GEMM_H).read()
    assert int(re.search(r"#define GEMM_CHUNK_MIN_K (\d+)", src).group(1)) == backend.GEMM_CHUNK_MIN_K
    assert int(re.search(r"#define GEMM_EXACT_CHUNK_MIN_K (\d+)", src).group(1)) == backend.GEMM_EXACT_CHUNK_MIN_K
    wide = re.search(r"const bool wide = (.*?);", src, re.S).group(1)
    named = {m.lower() for m in re.findall(r"kind == GR_(\w+)", wide)}
    lo, hi = re.search(r"kind >= GR_(\w+) && kind <= GR_(\w+)", wide).groups()
    kinds = _enum("GemmRouteKind")
    ranged = {k[3:].lower() for k, v in kinds.items() if kinds["GR_" + lo] <= v <= kinds["GR_" + hi]}
    assert named | ranged == set(backend.GEMM_WIDE_KINDS)
    # the widths themselves, where the kernels define them: 256 columns per workgroup of gemm_wreg.hip, 128 of the others unless `wide`
    csrc = os.path.dirname(GEMM_H)
    assert re.search(r"#define WR_BN 256\b", open(os.path.join(csrc, "gemm_wreg.hip")).read())
    assert re.search(r"#define BN 128\b", open(os.path.join(csrc, "gemm_tile.h")).read())
    assert len(re.findall(r"cdiv\(p\.N, wide \? 256 : BN\)", open(os.path.join(csrc, "gemm.hip")).read())) == 2
    assert re.search(r"p\.N % \(wide \? 256 : 128\)", src)
    assert backend.gemm_feature_names(feats["conv_k3"] | feats["stride2"]) == ["conv_k3", "stride2"]


def test_case_table_routes_are_well_formed():
    """Every route the GPU case table names exists (a misspelt kind would silently cover nothing)."""
    import test_gpu_gemm_variants as t

    from imcui_hip import backend

    cov = t.covered_routes()
    assert all(0 < r < 320 for r in cov)
    names = {backend.gemm_route_name(r) for r in cov}
    for want in ("conv_128/conv", "conv_256/conv", "conv_128_single/conv", "conv_256_single/conv", "exact/conv", "wreg_pipe/qkv_vit",
                 "wreg_mt2/conv", "wreg_mt1/conv", "wreg_rolled/resid", "split_128/bias", "split_f32b/bias"):
        assert want in names, want
    pairs = t.covered_pairs()
    assert {r for r, _ in pairs} >= cov, "every route of the table is a pair with feature 0"
    bits = set(backend.GEMM_FEATURES.values()) | {0}
    assert all(b in bits and 0 < r < 352 for r, b in pairs)
    F_ = backend.GEMM_FEATURES
    for kind, epi, feat in (("conv_128", "conv", "stride2"), ("conv_256", "conv", "conv_k1"), ("conv_128", "conv", "rup"),
                            ("split_128", "bias", "mcnt"), ("split_f32b", "bias", "ncnt"), ("wreg_pipe", "qkv_vit", "ln"), ("convd_128", "conv", "dilated"),
                            ("exact_dil", "conv", "conv_kother"), ("split_128", "bias", "a2"), ("exact", "bias", "wsel")):  # fmt: skip
        assert (backend.gemm_route(kind, epi), F_[feat]) in pairs, (kind, epi, feat)
