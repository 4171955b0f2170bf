"""Dilated implicit-im2col convolutions of the shared GEMM (csrc/gemm.hip, GemmP.conv_dil), entered through imcui_hip_gemm_probe_f32
and compared with float64 F.conv2d(dilation=...).

conv_dil > 1 selects instantiations of their own (ASRC = 2 of gemm_split_kernel: routes convd_128 / convd_256 / convd_f32b; DIL of the
exact kernel: exact_dil); conv_dil 0 / 1 is the undilated launch, instantiation and bits.  Every case asserts
  * the route the launch site recorded and the feature mask recorded with it (launch_features: what the case declares),
  * the result within the bars of tests/test_gpu_gemm_variants.py, relative to max |reference|: 2e-6 exact f32, 4e-6 split,
  * NaN sentinels (private payload) in the rows past M and the columns past N inside ldc, bitwise unchanged,
  * that plausible wrong references (undilated taps, taps transposed) miss the bar.
Shapes: B = 2, 13 x 17 -- M = 442 rows = four 128-row tiles, the last partial; smaller than the widest tap span, so at dilation 16
every output pixel has a tap outside the image and some have every tap of a row outside.  k = 2 with pad = d / 2 puts the taps at
-d/2 and +d/2 (the last three layers of R2D2's Quad_L2Net)."""
from __future__ import annotations

import math
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN_F32 = 0x7FC00ABC  # float32 NaN with a payload no arithmetic produces
ERR_UNSUPPORTED, ERR_ARG = -4, -1
B, H, W = 2, 13, 17


def _backend():
    from imcui_hip import backend

    return backend


def _bar(mode):
    return 2e-6 if mode == 0 else 4e-6


def _rel(out, ref):
    return (out.double() - ref).abs().max().item() / ref.abs().max().item()


def _operands(cid, cin, cout, k):
    g = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
    x = torch.randn(B, cin, H, W, generator=g)
    # a tap- and row-dependent offset: a shifted, transposed or undilated tap walk cannot pass
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k) + torch.arange(cout).float()[:, None, None, None] * 1e-3
    b = torch.randn(cout, generator=g) * 0.1
    return x, w, b


def launch_features(kind, k, dil, pad, cin, cout, act, ldc=None, stride=1):
    """GEMM_FEATURES mask (csrc/gemm.h GemmFeature) a launch of this file's shape records on the route kind `kind`: B x H x W map, bias
    given, no residual.  The gate of tests/test_gpu_gemm_variants.py counts the cases of this file through it."""
    be = _backend()
    F_ = be.GEMM_FEATURES
    d = max(dil or 1, 1)
    span = (k - 1) * d + 1
    M = B * ((H + 2 * pad - span) // stride + 1) * ((W + 2 * pad - span) // stride + 1)
    f = F_[{1: "conv_k1", 3: "conv_k3", 5: "conv_k5"}.get(k, "conv_kother")]
    f |= F_["stride2"] if stride == 2 else F_["stride_other"] if stride > 2 else 0
    f |= F_["pad_not_same"] if pad != (k - 1) * d // 2 else 0
    f |= F_["dilated"] if d > 1 else 0
    if k * k * cin >= be.GEMM_CHUNK_MIN_K:
        f |= F_["chunk"] if (kind == "exact" and k * k * cin >= be.GEMM_EXACT_CHUNK_MIN_K) or kind in ("exact_dil", "convd_128") else F_["long_k"]
    f |= {0: 0, 1: F_["act1"], 2: F_["act2"], 3: F_["act3"]}[act]
    f |= F_["ldc"] if (ldc or cout) != cout else 0
    f |= F_["n_mod32"] if cout % 32 else 0
    f |= F_["n_mod_tile"] if cout % (256 if kind in be.GEMM_WIDE_KINDS else 128) else 0
    f |= F_["m_small"] if M < 128 else 0
    return f


def _launch(x, w, b, k, dil, pad, act, mode, planes=True, ldc=None, expect=None, stride=1, **extra):
    """One probe launch into a sentinel buffer [M + 3, ldc]; returns (route or refusal code, buffer, M).  A launch that is not refused
    must have recorded the feature mask of launch_features."""
    be = _backend()
    be.gemm_route_reset(DEV)
    cout, cin = w.shape[:2]
    span = (k - 1) * max(dil or 1, 1) + 1
    ho, wo = (H + 2 * pad - span) // stride + 1, (W + 2 * pad - span) // stride + 1
    M = B * ho * wo
    ldc = ldc or cout
    wt = be.GemmWeights.conv([w], DEV)
    buf = torch.full((M + 3, ldc), NAN_F32, dtype=torch.int32, device=DEV).view(torch.float32)
    f = dict(epi="conv", A=x.permute(0, 2, 3, 1).contiguous().to(DEV), conv_k=k, conv_stride=stride, conv_pad=pad, conv_hin=H, conv_win=W,
             conv_hout=ho, conv_wout=wo, conv_cin=cin, K=k * k * cin, M=M, N=cout, C=buf, ldc=ldc, bias=b.to(DEV), act=act,
             **wt.fields(mode == 1, planes), **extra)  # fmt: skip
    if dil is not None:
        f["conv_dil"] = dil
    if isinstance(expect, int):
        rc = be.gemm_probe(DEV, check=False, **f)
        torch.cuda.synchronize()
        return rc, buf, M
    r = be.gemm_probe(DEV, **f)
    torch.cuda.synchronize()
    kind = be.gemm_route_name(r).split("/")[0]
    got, want = be.gemm_route_features(DEV).get(r, 0), launch_features(kind, k, dil, pad, cin, cout, act, ldc, stride)
    assert be.gemm_route_counts(DEV) == {r: 1} and got == want, (be.gemm_feature_names(got), be.gemm_feature_names(want))
    return r, buf, M


def table_launches():
    """[(route kind per mode {1: .., 0: ..}, arguments of launch_features)] of every launch the two case tables below make."""
    out = []
    for k, dil, pad, cin, cout in LAYERS:
        for act in (1, 0):
            out.append(({1: "convd_128" if dil > 1 else "conv_128", 0: "exact_dil" if dil > 1 else "exact"}, (k, dil, pad, cin, cout, act, cout + 4, 1)))
    for c in OTHER:
        out.append((c["routes"], (c["k"], c["dil"], c["pad"], c["cin"], c["cout"], 1, None, c.get("stride", 1))))
    return out


def _check_sentinels(buf, M, cout):
    bits = buf.view(torch.int32).cpu()
    written = torch.zeros(bits.shape, dtype=torch.bool)
    written[:M, :cout] = True
    bad = (bits[~written] != NAN_F32).sum().item()
    assert bad == 0, f"{bad} elements written outside the documented region"
    assert not torch.isnan(buf[:M, :cout]).any().item(), "an output element was not written"


def _ref(x, w, b, dil, pad, act, stride=1):
    y = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad, dilation=dil).permute(0, 2, 3, 1).reshape(-1, w.shape[0])
    return torch.relu(y) if act == 1 else y


# (k, dilation, pad, cin, cout): the six layer shapes R2D2 launches on the matrix engine (its layers 1-8)
LAYERS = [(3, 1, 1, 32, 32), (3, 2, 2, 64, 128), (3, 4, 4, 128, 128), (2, 4, 2, 128, 128), (2, 8, 4, 128, 128), (2, 16, 8, 128, 128)]


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("layer", LAYERS, ids=[f"k{k}_d{d}_p{p}_c{ci}_{co}" for k, d, p, ci, co in LAYERS])
def test_dilated_conv_against_float64(layer, relu, precision):
    be = _backend()
    k, dil, pad, cin, cout = layer
    cid = f"dil_k{k}_d{dil}_c{cin}_{cout}"
    x, w, b = _operands(cid, cin, cout, k)
    act = 1 if relu else 0
    route, buf, M = _launch(x, w, b, k, dil, pad, act, precision, ldc=cout + 4)
    want = ("exact_dil" if dil > 1 else "exact") if precision == 0 else ("convd_128" if dil > 1 else "conv_128")
    assert route == be.gemm_route(want, "conv"), f"route {be.gemm_route_name(route)}, expected {want}/conv"
    assert M == B * H * W  # pad = ((k - 1) d) // 2 keeps the size
    _check_sentinels(buf, M, cout)
    out = buf[:M, :cout].cpu()
    ref = _ref(x, w, b, dil, pad, act)
    err = _rel(out, ref)
    wrong = {"taps transposed": _ref(x, w.transpose(2, 3), b, dil, pad, act)}
    if dil > 1:  # the undilated walk of the same size (k = 3: around the centre; k = 2: from the pixel itself)
        lo, hi = (k - 1) // 2, k - 1 - (k - 1) // 2
        wrong["taps not dilated"] = _ref(F.pad(x, (lo, hi, lo, hi)), w, b, 1, 0, act)
    werr = {n: _rel(out, r) for n, r in wrong.items()}
    print(f"[gemm-dil] {cid} act {act} mode {precision} {be.gemm_route_name(route)}: err {err:.2e}  wrong refs: "
          + ", ".join(f"{n} {e:.1e}" for n, e in werr.items()))  # fmt: skip
    for n, e in werr.items():
        assert e > 4 * _bar(precision), f"the wrong reference '{n}' passes ({e:.2e}): the case cannot tell"
    assert err < _bar(precision), err


# the other two split instantiations (256-column tiles; f32 weights split on the fly), and a strided dilated launch
OTHER = [
    dict(id="wide_k3_d2_c32_256", k=3, dil=2, pad=2, cin=32, cout=256, routes={1: "convd_256", 0: "exact_dil"}),
    dict(id="f32b_k3_d4_c32_64", k=3, dil=4, pad=4, cin=32, cout=64, planes=False, routes={1: "convd_f32b", 0: "exact_dil"}),
    dict(id="stride2_k3_d2_c64_64", k=3, dil=2, pad=2, cin=64, cout=64, stride=2, routes={1: "convd_128", 0: "exact_dil"}),
    dict(id="n65_scalar_stores_k2_d4", k=2, dil=4, pad=2, cin=32, cout=65, routes={1: "convd_128", 0: "exact_dil"}),
    # K = 4608 >= GEMM_CHUNK_MIN_K: the two-level sum (D2-Net's dilated 512-channel layers); pre-split planes take the 128-column kernel whatever N
    dict(id="chunk_k3_d2_c512_512", k=3, dil=2, pad=2, cin=512, cout=512, routes={1: "convd_128", 0: "exact_dil"}),
    dict(id="chunk_k3_d2_c512_64", k=3, dil=2, pad=2, cin=512, cout=64, routes={1: "convd_128", 0: "exact_dil"}),
]


@pytest.mark.parametrize("c", OTHER, ids=[c["id"] for c in OTHER])
def test_dilated_conv_other_routes(c, precision):
    be = _backend()
    x, w, b = _operands(c["id"], c["cin"], c["cout"], c["k"])
    st = c.get("stride", 1)
    route, buf, M = _launch(x, w, b, c["k"], c["dil"], c["pad"], 1, precision, planes=c.get("planes", True), stride=st)
    want = c["routes"][precision]
    assert route == be.gemm_route(want, "conv"), f"route {be.gemm_route_name(route)}, expected {want}/conv"
    _check_sentinels(buf, M, c["cout"])
    ref = _ref(x, w, b, c["dil"], c["pad"], 1, st)
    assert ref.shape[0] == M
    err = _rel(buf[:M].cpu(), ref)
    print(f"[gemm-dil] {c['id']} mode {precision} {be.gemm_route_name(route)}: err {err:.2e}")
    assert err < _bar(precision), err


def test_no_dilation_is_the_undilated_launch_bitwise(precision):
    """conv_dil = 0 and conv_dil = 1 take the route of a launch that does not set the field and return its bits."""
    be = _backend()
    k, pad, cin, cout = 3, 1, 64, 128
    x, w, b = _operands("dil_off", cin, cout, k)
    outs = {}
    for dil in (None, 0, 1):
        route, buf, M = _launch(x, w, b, k, dil, pad, 1, precision)
        assert route == be.gemm_route("conv_128" if precision == 1 else "exact", "conv"), be.gemm_route_name(route)
        outs[dil] = buf.view(torch.int32).cpu()
    assert torch.equal(outs[None], outs[0]) and torch.equal(outs[None], outs[1])
    assert _rel(outs[None][:M].view(torch.float32), _ref(x, w, b, 1, pad, 1)) < _bar(precision)


def test_refusals(precision):
    """The launcher's refusals hold for dilated launches (cin % 32, K = k^2 cin), the single-product arithmetic is not built for them,
    a negative dilation and a dilation without conv_k are argument errors; a refused call writes nothing and records no route."""
    be = _backend()
    hd = be.get_handle(DEV)
    x, w, b = _operands("dil_refuse", 32, 64, 3)
    rc, buf, M = _launch(x, w, b, 3, 2, 2, 0, precision, expect=ERR_UNSUPPORTED, single=1)
    assert rc == ERR_UNSUPPORTED, rc
    assert hd.lib.imcui_hip_gemm_last_route(hd.h) == 0
    assert (buf.view(torch.int32) == NAN_F32).all().item()
    rc, buf, M = _launch(x, w, b, 3, -2, 2, 0, precision, expect=ERR_ARG)
    assert rc == ERR_ARG and (buf.view(torch.int32) == NAN_F32).all().item()
    x48, w48, b48 = _operands("dil_refuse48", 48, 64, 3)
    rc, buf, M = _launch(x48, w48, b48, 3, 2, 2, 0, precision, expect=ERR_ARG)
    assert rc == ERR_ARG and (buf.view(torch.int32) == NAN_F32).all().item()
    # a plain matrix launch with a dilation set
    wt = be.GemmWeights([torch.randn(64, 32)], DEV)
    a = torch.randn(128, 32, device=DEV)
    c = torch.zeros(128, 64, device=DEV)
    rc = be.gemm_probe(DEV, check=False, epi="conv", A=a, lda=32, K=32, M=128, N=64, C=c, ldc=64, conv_dil=2, **wt.fields(precision == 1))
    assert rc == ERR_ARG, rc
