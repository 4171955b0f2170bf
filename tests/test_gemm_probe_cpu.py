"""CPU side of the GEMM variant tests (tests/test_gpu_gemm_variants.py): the descriptor mirror, the weight packing the probe uses and
the route numbering shared with csrc/gemm.h."""
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
