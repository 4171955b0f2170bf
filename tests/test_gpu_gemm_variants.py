"""Every instantiation of the shared GEMM (csrc/gemm.hip, csrc/gemm_wreg.hip) that the networks launch, entered directly through
imcui_hip_gemm_probe_f32 and compared with a plain float64 restatement of the same operation.

One case table (CASES).  Every case names the kernel instantiation it targets per arithmetic mode -- or the refusal it expects -- and
asserts it through the route the launch site recorded (imcui_hip_gemm_last_route), together with the feature mask the launcher derived
from the parameters (imcui_hip_gemm_route_features, GemmFeature of csrc/gemm.h): the case declares its mask (mask_of, from what the
case table says about the launch) and the recorder must hold exactly it.  Every case then checks three things:
  * the result against float64 within the building-block bars, relative to max |reference|: 2e-6 exact f32, 4e-6 otherwise.  The
    single-product variants are compared with float64 on the operands rounded the way gemm.hip documents (nearest-even f16 of the
    scaled weight, saturating nearest-even f16 of the activation), with the same 4e-6 bar;
  * memory the kernel must not write (NaN sentinels with a private payload: columns past N inside ldc, rows past M, rows past the
    device-side row counts, skipped tiles of ragged sequences, plane padding) is bitwise unchanged;
  * a plausible wrong reference for each fused feature misses the bar (the inputs can tell the difference).
The four new cases of undilated launches that sum K >= 2048 (3x3 at 512 channels, K = 4608, two column tiles; the bottleneck 1x1 and the
valid 8 x 8 layer, K = 2048; flag long_k_bar -- no other case) are held to max(bar, 2 E), E being the error of float32 CPU torch on the same operands against the same float64 reference, computed in the
case and printed next to the device's error.
test_routes_of_every_network_are_covered reads network_sweep() -- ONE cached pass over every network of the tree (networks(): the list
and the variants left out are in its docstring) in both arithmetic modes that collects the GEMM, attention, 3x3-convolution and FFN
recorders per network; the four gates share it -- and fails on a (route, feature bit) pair that neither this table nor that of
tests/test_gpu_gemm_dilated.py launches, and on a network that uses the shared GEMM and recorded no launch.
Keyed on the route alone the gate had passed; keyed on (route, feature) and run on every network it reported 55 pairs of the parent's
tables without a case (cnt / active under the row-major epilogues, null bias, batched + second slab + mcnt, the second slab under
EPI_CONV, implicit im2col under mcnt, the two-level sum, long undilated K, the single-product 1x1 and stride-2 launches, per-pair
weights under EPI_QKV_VIT, ...): the cases after "launches of the networks the gate found without a case" close them."""
from __future__ import annotations

import functools
import math
import time
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN_F32 = 0x7FC00ABC  # float32 NaN with a payload no arithmetic produces
NAN_F16 = 0x7E5B  # the same for the f16 planes
ERR_ARG, ERR_UNSUPPORTED = -1, -4


def _backend():
    from imcui_hip import backend

    return backend


def _bar(mode):
    return 2e-6 if mode == 0 else 4e-6


def _rel(out, ref):
    return (out.double() - ref).abs().max().item() / ref.abs().max().item()


def _sentinel(*shape):
    return torch.full(shape, NAN_F32, dtype=torch.int32, device=DEV).view(torch.float32)


def _untouched(buf, written):
    """Every element of `buf` outside the boolean mask `written` still holds the sentinel, bit for bit."""
    bits = buf.view(torch.int32 if buf.dtype == torch.float32 else torch.int16).cpu()
    want = NAN_F32 if buf.dtype == torch.float32 else NAN_F16
    bad = (bits[~written] != want).sum().item()
    assert bad == 0, f"{bad} elements written outside the documented region"


def _weights(g, N, K, scale=None, ramp=0.01):
    """Random weights with a row-dependent offset: a transposed or shifted store cannot pass."""
    s = scale if scale is not None else 1.0 / math.sqrt(K)
    return torch.randn(N, K, generator=g) * s + torch.arange(N).float()[:, None] * (ramp * s)


def _act(y, act):
    if act == 1:
        return torch.relu(y)
    if act == 2:
        return F.leaky_relu(y, 0.01)
    if act == 3:
        return F.gelu(y)  # exact erf
    return y


def _round_single(w, wscale):
    """The operand of the single-product arithmetic: nearest-even f16 of w * 2^e (split_one), back in float64."""
    return (w.float() / wscale).half().double() * wscale


def _round_act(x):
    """half2_rtn: nearest-even f16 of the activation, saturating at +-65504."""
    return x.float().clamp(-65504.0, 65504.0).half().double()


def mask_of(kind, epi, M, N, K, *, conv_k=0, stride=1, pad=None, dil=1, resid=False, rup=False, act=0, ldc=None, a2=False, batch=1, mcnt=False,
            ncnt=False, cnt=False, active=False, wsel=False, ln=False, alpha=1.0, bias=True):
    """GEMM_FEATURES mask (csrc/gemm.h GemmFeature) of a launch on the route kind `kind`, from what a case of the table says about it."""
    be = _backend()
    F_ = be.GEMM_FEATURES
    f = 0
    if conv_k:
        f |= F_[{1: "conv_k1", 3: "conv_k3", 5: "conv_k5"}.get(conv_k, "conv_kother")]
        f |= F_["stride2"] if stride == 2 else F_["stride_other"] if stride > 2 else 0
        f |= F_["pad_not_same"] if (conv_k // 2 if pad is None else pad) != (conv_k - 1) * dil // 2 else 0
        f |= F_["dilated"] if dil > 1 else 0
        f |= F_["conv_batched"] if batch > 1 or mcnt else 0
    if K >= be.GEMM_CHUNK_MIN_K:
        f |= F_["chunk"] if (kind == "exact" and K >= be.GEMM_EXACT_CHUNK_MIN_K) or kind in ("exact_dil", "convd_128") else F_["long_k"]
    f |= F_["rup"] if rup else F_["resid"] if resid or epi == "resid" else 0
    f |= {0: 0, 1: F_["act1"], 2: F_["act2"], 3: F_["act3"]}[act] if epi == "conv" else 0
    f |= F_["ldc"] if epi in ("bias", "relu", "resid", "conv") and (ldc or N) != N else 0
    f |= F_["n_mod32"] if N % 32 else 0
    f |= F_["n_mod_tile"] if N % (256 if kind in be.GEMM_WIDE_KINDS else 128) else 0
    f |= F_["m_small"] if M < 128 else 0
    for name, on in (("a2", a2), ("batch", batch > 1), ("mcnt", mcnt), ("ncnt", ncnt), ("cnt", cnt), ("active", active), ("wsel", wsel), ("ln", ln),
                     ("alpha", alpha != 1.0 and epi in ("bias", "qkv", "cross", "qkv_vit")), ("no_bias", not bias)):  # fmt: skip
        f |= F_[name] if on else 0
    return f


def _probe(feat, expect, **fields):
    """Launch; `expect` is a route (kind, epi) or a negative refusal code; feat(kind) is the feature mask the case declares for a launch
    on that route kind, and the recorder must hold exactly it.  Returns the route."""
    be = _backend()
    be.gemm_route_reset(DEV)
    if isinstance(expect, int):
        rc = be.gemm_probe(DEV, check=False, **fields)
        assert rc == expect, f"expected refusal {expect}, got {rc}"
        assert be.get_handle(DEV).lib.imcui_hip_gemm_last_route(be.get_handle(DEV).h) == 0
        assert be.gemm_route_counts(DEV) == {} and be.gemm_route_features(DEV) == {}
        return None
    r = be.gemm_probe(DEV, **fields)
    torch.cuda.synchronize()
    assert r == be.gemm_route(*expect), f"route {be.gemm_route_name(r)}, expected {expect}"
    got, want = be.gemm_route_features(DEV).get(r, 0), feat(expect[0])
    assert be.gemm_route_counts(DEV) == {r: 1}
    assert got == want, f"features {be.gemm_feature_names(got)}, the case declares {be.gemm_feature_names(want)}"
    return r


def _report(cid, mode, route, err, wrong=None):
    be = _backend()
    w = "" if not wrong else "  wrong refs: " + ", ".join(f"{k} {v:.1e}" for k, v in wrong.items())
    print(f"[gemm] {cid} mode {mode} {be.gemm_route_name(route) if route else 'refused'}: err {err:.2e}{w}")


def _discriminates(out, wrong_refs, mode):
    errs = {k: _rel(out, r) for k, r in wrong_refs.items()}
    for k, e in errs.items():
        assert e > 4 * _bar(mode), f"the wrong reference '{k}' passes ({e:.2e}): the case cannot tell"
    return errs


# ------------------------------------------------------------------ implicit-im2col convolutions
def _conv_out(c):
    k, pad = c["k"], c.get("pad", c["k"] // 2)
    return (c["H"] + 2 * pad - k) // c["stride"] + 1, (c["W"] + 2 * pad - k) // c["stride"] + 1


def feat_conv(c, kind):
    ho, wo = _conv_out(c)
    return mask_of(kind, "conv", c["B"] * ho * wo, c["cout"], c["k"] ** 2 * c["cin"], conv_k=c["k"], stride=c["stride"], pad=c.get("pad"),
                   resid=c.get("resid", False), act=c.get("act", 0), ldc=c.get("ldc"))  # fmt: skip


def _long_k_bar(mode, out32, ref):
    """Bar of the undilated K >= 2048 cases: max(the building-block bar, 2 E), E = the error of float32 CPU torch on the same operands
    against the same float64 reference (the factor 2: another summation order, nothing more).  Returns (bar, E)."""
    e = _rel(out32, ref)
    return max(_bar(mode), 2 * e), e


def run_conv(c, mode):
    be = _backend()
    B, H, W, cin, cout, k, st = c["B"], c["H"], c["W"], c["cin"], c["cout"], c["k"], c["stride"]
    act, use_res, single, planes = c.get("act", 0), c.get("resid", False), c.get("single", False), c.get("planes", True)
    ldc, col0 = c.get("ldc", cout), c.get("col0", 0)
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k) + torch.arange(cout).float()[:, None, None, None] * 1e-3
    b = torch.randn(cout, generator=g) * 0.1
    pad = c.get("pad", k // 2)
    ho, wo = _conv_out(c)
    M = B * ho * wo
    wt = be.GemmWeights.conv([w], DEV)
    res = torch.randn(M, cout, generator=g) if use_res else None
    buf = _sentinel(M + 3, ldc)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    f = dict(epi="conv", A=xd, conv_k=k, conv_stride=st, conv_pad=pad, conv_hin=H, conv_win=W, conv_hout=ho, conv_wout=wo, conv_cin=cin,
             K=k * k * cin, M=M, N=cout, C=buf[:, col0:], ldc=ldc, bias=b.to(DEV), act=act, single=int(single),
             resid=None if res is None else res.to(DEV), ldr=cout, **wt.fields(mode == 1, planes))  # fmt: skip
    route = _probe(lambda kind: feat_conv(c, kind), c["routes"][mode], **f)
    written = torch.zeros(M + 3, ldc, dtype=torch.bool)
    if route is not None:
        written[:M, col0 : col0 + cout] = True
    _untouched(buf, written)
    if route is None:
        return _report(c["id"], mode, None, 0.0)
    out = buf[:M, col0 : col0 + cout].cpu()
    assert not torch.isnan(out).any().item(), "an output element was not written"
    xs, ws = (x.double(), w.double()) if not single else (_round_act(x), _round_single(w, wt.wscale[0].item()))

    def ref_of(r, stride=st, padding=pad, xs=xs, ws=ws, bias=b.double()):
        y = F.conv2d(xs, ws, bias, stride=stride, padding=padding)[:, :, :ho, :wo].permute(0, 2, 3, 1).reshape(M, cout)
        return _act(y + (0 if r is None else r), act)

    r64 = None if res is None else res.double()
    ref = ref_of(r64)
    err = _rel(out, ref)
    wrong = {}
    if res is not None:
        r_row, r_col = res.double().clone(), res.double().clone()
        r_row[-1] = 0
        r_col[:, -1] = 0
        wrong.update({"residual dropped on the last row": ref_of(r_row), "residual dropped on the last column": ref_of(r_col)})
    if c.get("tap_refs"):  # the tap walk of a strided / un-padded launch: the walk of stride 1, and one more ring of padding
        if st > 1:
            wrong["stride-1 walk"] = ref_of(r64, stride=1)
        wrong["pad + 1"] = ref_of(r64, padding=pad + 1)
        if k > 1:
            wrong["taps transposed"] = ref_of(r64, ws=ws.transpose(2, 3))
    wrong = _discriminates(out, wrong, mode) if wrong else {}
    _report(c["id"], mode, route, err, wrong)
    bar = _bar(mode)
    if c.get("long_k_bar"):  # only the cases that ask for it: every other case keeps the plain bar whatever its K
        assert k * k * cin >= be.GEMM_CHUNK_MIN_K and not single
        r32 = None if res is None else res
        bar, e32 = _long_k_bar(mode, ref_of(r32, xs=x, ws=w, bias=b), ref)
        print(f"[gemm] {c['id']} mode {mode}: K = {k * k * cin}, device err {err:.2e}, float32 CPU torch E {e32:.2e}, bar max({_bar(mode):.0e}, 2 E) = {bar:.2e}")
    assert err < bar, (err, bar)


# ------------------------------------------------------------------ implicit im2col, batched, with device-side row counts (DoG + HardNet / SOSNet)
def feat_conv_batched(c, kind):
    ho, wo = _conv_out(c)
    return mask_of(kind, "conv", ho * wo, c["cout"], c["k"] ** 2 * c["cin"], conv_k=c["k"], stride=c["stride"], act=c.get("act", 0), ldc=c.get("ldc"),
                   batch=c["batch"], mcnt=True)  # fmt: skip


def run_conv_batched(c, mode):
    """Batch item z = one image; mcnt[z] = how many of its output pixels (rows) are live.  Rows past mcnt[z] and whole skipped items keep
    their bits; the live rows equal float64 within the bar AND, bit for bit, the rows of the unbatched launch on that image alone."""
    be = _backend()
    Z, H, W, cin, cout, k, st, act = c["batch"], c["H"], c["W"], c["cin"], c["cout"], c["k"], c["stride"], c.get("act", 0)
    pad, ldc = k // 2, c.get("ldc", cout)
    ho, wo = _conv_out(c)
    M, mc = ho * wo, c["mcnt"]
    assert len(mc) == Z and max(mc) == M
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    x = torch.randn(Z, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k) + torch.arange(cout).float()[:, None, None, None] * 1e-3
    b = torch.randn(cout, generator=g) * 0.1
    wt = be.GemmWeights.conv([w], DEV)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    buf = _sentinel(Z, M + 3, ldc)
    common = dict(epi="conv", conv_k=k, conv_stride=st, conv_pad=pad, conv_hin=H, conv_win=W, conv_hout=ho, conv_wout=wo, conv_cin=cin, K=k * k * cin,
                  M=M, N=cout, ldc=ldc, bias=b.to(DEV), act=act, **wt.fields(mode == 1))  # fmt: skip
    route = _probe(lambda kind: feat_conv_batched(c, kind), c["routes"][mode], A=xd, C=buf, batch=Z, a_bs=H * W * cin, c_bs=(M + 3) * ldc,
                   mcnt=torch.tensor(mc, dtype=torch.int32).to(DEV), cnt_stride=1, **common)  # fmt: skip
    written = torch.zeros(Z, M + 3, ldc, dtype=torch.bool)
    for z in range(Z):
        written[z, : mc[z], :cout] = True
    _untouched(buf, written)
    ref = _act(F.conv2d(x.double(), w.double(), b.double(), stride=st, padding=pad), act).permute(0, 2, 3, 1).reshape(Z, M, cout)
    swapped = _act(F.conv2d(x.double(), w.double().transpose(2, 3), b.double(), stride=st, padding=pad), act).permute(0, 2, 3, 1).reshape(Z, M, cout)
    errs = []
    for z in range(Z):
        if mc[z] == 0:
            continue
        got = buf[z, : mc[z], :cout].cpu()
        assert not torch.isnan(got).any().item(), "a live output element was not written"
        errs.append(_rel(got, ref[z, : mc[z]]))
        _discriminates(got, {"image of the next batch item": ref[(z + 1) % Z, : mc[z]], "taps transposed": swapped[z, : mc[z]]}, mode)
        solo = _sentinel(M + 3, ldc)
        r1 = be.gemm_probe(DEV, A=xd[z], C=solo, **common)
        torch.cuda.synchronize()
        assert r1 == route
        assert torch.equal(solo[: mc[z], :cout].view(torch.int32).cpu(), got.view(torch.int32)), f"item {z}: the batched rows differ from the unbatched launch"
    _report(c["id"], mode, route, max(errs))
    assert max(errs) < _bar(mode), errs


# ------------------------------------------------------------------ bilinear x2 up-sampled residual (LoFTR / EfficientLoFTR FPN)
def feat_rup(c, kind):
    return mask_of(kind, "conv", c["B"] * 4 * c["h"] * c["w"], c["cout"], c["cin"], conv_k=1, rup=True, act=c.get("act", 0))


def run_rup(c, mode):
    be = _backend()
    B, h, w, cin, cout, align = c["B"], c["h"], c["w"], c["cin"], c["cout"], c["align"]
    H, W = 2 * h, 2 * w
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    x = torch.randn(B, cin, H, W, generator=g)
    wgt = torch.randn(cout, cin, 1, 1, generator=g) / math.sqrt(cin) + torch.arange(cout).float()[:, None, None, None] * 1e-3
    b = torch.randn(cout, generator=g) * 0.1
    low = torch.randn(B, cout, h, w, generator=g)
    wt = be.GemmWeights.conv([wgt], DEV)
    M = B * H * W
    buf = _sentinel(M + 2, cout)
    f = dict(epi="conv", A=x.permute(0, 2, 3, 1).contiguous().to(DEV), conv_k=1, conv_stride=1, conv_pad=0, conv_hin=H, conv_win=W,
             conv_hout=H, conv_wout=W, conv_cin=cin, K=cin, M=M, N=cout, C=buf, ldc=cout, bias=b.to(DEV), act=c.get("act", 0),
             resid=low.permute(0, 2, 3, 1).contiguous().to(DEV), ldr=cout, rup_h=h, rup_w=w, rup_align=align, **wt.fields(mode == 1))  # fmt: skip
    route = _probe(lambda kind: feat_rup(c, kind), c["routes"][mode], **f)
    written = torch.zeros(M + 2, cout, dtype=torch.bool)
    if route is not None:
        written[:M] = True
    _untouched(buf, written)
    if route is None:
        return _report(c["id"], mode, None, 0.0)
    out = buf[:M].cpu()
    y = F.conv2d(x.double(), wgt.double(), b.double())

    def ref_of(al, drop=None):
        up = F.interpolate(low.double(), size=(H, W), mode="bilinear", align_corners=bool(al))
        if drop == "row":
            up[:, :, -1, :] = 0
        elif drop == "col":
            up[:, :, :, -1] = 0
        return _act(y + up, c.get("act", 0)).permute(0, 2, 3, 1).reshape(M, cout)

    err = _rel(out, ref_of(align))
    wrong = _discriminates(out, {"align_corners flipped": ref_of(1 - align), "residual dropped on the last row": ref_of(align, "row"),
                                 "residual dropped on the last column": ref_of(align, "col")}, mode)  # fmt: skip
    _report(c["id"], mode, route, err, wrong)
    assert err < _bar(mode), err


# ------------------------------------------------------------------ plain matrix operand: epilogues, tiles, ldc, A2, wsel, batches
def feat_matrix(c, kind):
    epi = c["epi"]
    return mask_of(kind, epi, c["M"], c["N"], c["K"], resid=bool(c.get("resid")) and epi in ("resid", "conv"), act=c.get("act", 0), ldc=c.get("ldc"),
                   a2=c.get("K1") is not None, wsel=c.get("sets", 1) > 1, ln=bool(c.get("ln")), alpha=c.get("alpha", 1.0), cnt="cnt" in c,
                   active="active" in c, bias=c.get("bias", True))  # fmt: skip


def _row_tile(kind):
    """Rows per workgroup of a route kind: ragged sequences and inactive pairs are skipped by whole row tiles."""
    return {"wreg_mt1": 32, "wreg_mt2": 64}.get(kind, 128)


def run_matrix(c, mode):
    """Row-major A [M, K] (optionally a second K slab), C = epi(A W^T + bias) with the case's extras.  With `cnt` (rows per sequence of
    R rows) and `active` (per pair of sequences): row tiles whose first row is past the count, and every tile of an inactive pair, are not
    launched -- their rows keep the bits they held; the rows below the count of an active pair are compared."""
    be = _backend()
    M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    nsets = c.get("sets", 1)
    ws = [_weights(g, N, K, ramp=c.get("ramp", 0.01)) for _ in range(nsets)]
    bs = [torch.randn(N, generator=g) * 0.1 for _ in range(nsets)]
    if nsets > 1:
        ws[1] = ws[1] * 8  # a power of two: set 1 packs with its own scale 2^-e (wscale[1] = 8 wscale[0])
    if "bias_sweep" in c:
        ws = [w * 0.01 for w in ws]
        bs = [torch.linspace(-c["bias_sweep"], c["bias_sweep"], N)]
    has_bias = c.get("bias", True)
    if not has_bias:
        bs = [torch.zeros(N) for _ in range(nsets)]
    wt = be.GemmWeights(ws, DEV)
    lda = c.get("lda", K)
    K1 = c.get("K1")
    a = torch.randn(M, K, generator=g)
    ldc = c.get("ldc", N)
    act, single = c.get("act", 0), c.get("single", False)
    buf = _sentinel(M + 2, ldc)
    f = dict(epi=epi, M=M, N=N, K=K, C=buf, ldc=ldc, act=act, single=int(single), alpha=c.get("alpha", 1.0),
             bias=torch.cat(bs).to(DEV) if has_bias else None, **wt.fields(mode == 1, c.get("planes", True)))  # fmt: skip
    if K1 is not None:
        a1 = torch.zeros(M, lda)
        a1[:, :K1] = a[:, :K1]
        a2 = torch.zeros(M, K - K1 + 8)
        a2[:, : K - K1] = a[:, K1:]
        f.update(A=a1.to(DEV), lda=lda, A2=a2.to(DEV), lda2=K - K1 + 8, K1=K1)
    else:
        ap = torch.zeros(M, lda)
        ap[:, :K] = a
        f.update(A=ap.to(DEV), lda=lda)
    sel = torch.zeros(M, dtype=torch.long)
    R = c.get("R")
    if R:
        f.update(rows_per_seq=R)
    if nsets > 1:
        wsel = torch.tensor(c["wsel"], dtype=torch.int32)
        sel = (wsel.long()[torch.arange(M) // R // 2] + c["wsel_off"])
        f.update(wsel=wsel.to(DEV), wsel_off=c["wsel_off"], b_stride=N)
    live = torch.ones(M, dtype=torch.bool)  # rows the launch must compute
    seq, row = (torch.arange(M) // R, torch.arange(M) % R) if R else (None, None)
    if "cnt" in c:
        cnts = torch.tensor(c["cnt"], dtype=torch.int32)
        assert len(cnts) * R == M
        f.update(cnt=cnts.to(DEV))
        live &= row < cnts.long()[seq]
    if "active" in c:
        actv = torch.tensor(c["active"], dtype=torch.int32)
        assert 2 * len(actv) * R == M
        f.update(active=actv.to(DEV))
        live &= actv.bool()[seq // 2]
    assert live.any()

    def rows_written(kind):
        """Rows of the tiles that are launched: whole row tiles that hold a live row."""
        if R is None or ("cnt" not in c and "active" not in c):
            return torch.ones(M, dtype=torch.bool)
        t = _row_tile(kind)
        first = torch.arange(M) // t * t  # (R % 128 == 0: a tile never straddles two sequences)
        return live[first] if "cnt" in c else live

    res = None
    if epi in ("resid", "conv") and c.get("resid", False):
        res = torch.randn(M, N, generator=g)
        buf[:M, :N] = res.to(DEV)  # in place: C is the residual
        if epi == "conv":
            f.update(resid=buf, ldr=ldc)
    ratio = c.get("ln_ratio")
    if c.get("ln"):
        a, w0, b0, gam, bet, fl = _ln_operands(g, N, M, K, ratio, mode)
        ws, bs = [w0], [b0]
        f.update(A=a.to(DEV), lda=K, **fl)
    snapshot = buf.clone()
    snap_bits = snapshot.view(torch.int32).cpu()
    runs = []
    for opts, expect in c["routes"][mode]:
        buf.copy_(snapshot)
        with be.option(DEV, **opts):
            route = _probe(lambda kind: feat_matrix(c, kind), expect, **f)
        written = torch.zeros(M + 2, ldc, dtype=torch.bool)
        if route is not None:
            written[:M, :N] = rows_written(expect[0])[:, None]
        bits = buf.view(torch.int32).cpu()
        bad = (bits[~written] != snap_bits[~written]).sum().item()  # the sentinels, and the pre-loaded residual of rows that are skipped
        assert bad == 0, f"{bad} elements written outside the documented region"
        if route is not None:
            assert not torch.isnan(buf[:M, :N].cpu()[live]).any().item(), "a live output element was not written"
        runs.append((route, buf[:M, :N].cpu().clone()))
    if runs[0][0] is None:
        return _report(c["id"], mode, None, 0.0)
    a64 = a.double() if not c.get("ln") else F.layer_norm(a.double(), (K,), gam.double(), bet.double(), eps=1e-6)
    wsel_sets = torch.stack([w.double() for w in ws])
    bsel = torch.stack([b.double() for b in bs])
    if single:
        a64 = _round_act(a)
        wsel_sets = torch.stack([_round_single(w, wt.wscale[i].item()) for i, w in enumerate(ws)])

    def ref_of(selv, drop_last_col=False):
        if nsets == 1:  # (one set: no [M, N, K] gather)
            y = a64 @ wsel_sets[0].t() + bsel[0]
        else:
            y = torch.einsum("mk,mnk->mn", a64, wsel_sets[selv]) + bsel[selv]
        if epi == "bias":
            y = y * c.get("alpha", 1.0)
        if res is not None:
            r = res.double().clone()
            if drop_last_col:
                r[:, -1] = 0
            y = y + r
        return _act(y, act) if epi == "conv" else torch.relu(y) if epi == "relu" else y

    ref = ref_of(sel)
    wrong = {}
    if nsets > 1:
        other = sel.clone()
        pair = torch.arange(M) // c["R"] // 2
        other[pair == 0] = sel[pair == 1][0]
        wrong["wsel of the other pair"] = ref_of(other)
        sc = wt.wscale.cpu().double()
        assert sc[1] != sc[0], "the weight sets must carry different scales"
        good = wsel_sets
        wsel_sets = good * (sc[0] / sc)[:, None, None]  # every set read with the scale of set 0
        wrong["scale of set 0"] = ref_of(sel)
        wsel_sets = good
    if res is not None:
        wrong["residual dropped on the last column"] = ref_of(sel, True)
    if "bias_sweep" in c:
        y = torch.einsum("mk,mnk->mn", a64, wsel_sets[sel]) + bsel[sel]
        wrong["tanh GELU"] = F.gelu(y, approximate="tanh")
    if K1 is not None and epi == "conv":  # (the plain-epilogue slab cases predate this reference and keep their checks)
        flipped = torch.cat([a64[:, K1:], a64[:, :K1]], 1) if 2 * K1 == K else torch.cat([a64[:, :K1], a64[:, K1:].flip(1)], 1)
        good_a, a64 = a64, flipped
        wrong["second K slab read in another order"] = ref_of(sel)
        a64 = good_a
    bar = _bar(mode) if not c.get("ln") or ratio <= 4 else _ln_bound(ratio, K)
    e32 = None
    if c.get("long_k_bar"):  # one long sum: the bar of _long_k_bar, only for the cases that ask for it
        assert K >= be.GEMM_CHUNK_MIN_K and not c.get("ln") and not single and nsets == 1 and epi != "bias"
        y32 = a @ ws[0].t() + bs[0] + (0 if res is None else res)
        bar, e32 = _long_k_bar(mode, (_act(y32, act) if epi == "conv" else torch.relu(y32) if epi == "relu" else y32)[live], ref[live])
    worst = 0.0
    for route, out in runs:
        err = _rel(out[live], ref[live])
        if nsets > 1:  # sets of different magnitude: each pair relative to its own output
            pair = torch.arange(M) // c["R"] // 2
            err = max(_rel(out[live & (pair == p)], ref[live & (pair == p)]) for p in range(int(pair.max()) + 1) if (live & (pair == p)).any())
        errs = _discriminates(out[live], {k: v[live] for k, v in wrong.items()}, mode) if wrong else {}
        _report(c["id"], mode, route, err, errs)
        if e32 is not None:
            print(f"[gemm] {c['id']} mode {mode}: K = {K}, device err {err:.2e}, float32 CPU torch E {e32:.2e}, bar max({_bar(mode):.0e}, 2 E) = {bar:.2e}")
        assert err < bar, (err, bar)
        worst = max(worst, err)
    if c.get("bitwise"):
        for _, out in runs[1:]:
            assert torch.equal(out, runs[0][1]), "the token tiles are documented bitwise equal"
    return worst


# ------------------------------------------------------------------ batched: device-side row / column counts per batch item
def feat_batched(c, kind):
    return mask_of(kind, c.get("epi", "bias"), c["M"], c["N"], c["K"], batch=c["batch"], mcnt=True, ncnt=bool(c.get("f32b")) and c.get("ncnt") is not None,
                   alpha=c.get("alpha", 1.0), a2=c.get("K1") is not None, bias=c.get("bias", True))  # fmt: skip


def run_batched(c, mode):
    be = _backend()
    Z, M, N, K = c["batch"], c["M"], c["N"], c["K"]
    mc, nc = c["mcnt"], c.get("ncnt")
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    a_bs, c_bs = (M + 5) * K, (M + 3) * N
    a = torch.randn(Z, M + 5, K, generator=g)
    buf = _sentinel(Z, M + 3, N)
    b = torch.randn(N, generator=g) * (0.1 if c.get("bias", True) else 0.0)
    epi, K1 = c.get("epi", "bias"), c.get("K1")
    post = torch.relu if epi == "relu" else (lambda y: y)
    cnt = torch.tensor([v for pair in zip(mc, nc or mc) for v in pair], dtype=torch.int32)  # (m, n) interleaved: cnt_stride 2
    f = dict(epi=epi, A=a.to(DEV), lda=K, M=M, N=N, K=K, C=buf, ldc=N, c_bs=c_bs, a_bs=a_bs, batch=Z, bias=b.to(DEV) if c.get("bias", True) else None,
             mcnt=cnt.to(DEV), cnt_stride=2, alpha=c.get("alpha", 1.0))  # fmt: skip
    if K1 is not None:  # the K axis in two slabs of their own (LoFTR's [message | x] MLP input), each with its batch stride
        f.update(A=a[..., :K1].contiguous().to(DEV), lda=K1, a_bs=(M + 5) * K1, A2=a[..., K1:].contiguous().to(DEV), lda2=K - K1, a2_bs=(M + 5) * (K - K1), K1=K1)
    if c.get("f32b"):
        w = torch.stack([_weights(g, N, K) for _ in range(Z)])
        f.update(W=w.to(DEV), ldw=K, w_bs=N * K)
        if nc is not None:
            f["ncnt"] = cnt[1:].to(DEV)
    else:
        w = _weights(g, N, K)[None].expand(Z, N, K)
        f.update(be.GemmWeights([w[0]], DEV).fields(mode == 1))
    route = _probe(lambda kind: feat_batched(c, kind), c["routes"][mode], **f)
    written = torch.zeros(Z, M + 3, N, dtype=torch.bool)
    for z in range(Z):
        written[z, : mc[z], : (nc[z] if nc else N)] = True
    _untouched(buf, written)
    errs = []
    for z in range(Z):
        if mc[z] == 0:
            continue
        n = nc[z] if nc else N
        ref = post((a[z, : mc[z]].double() @ w[z, :n].double().t() + b[:n].double()) * c.get("alpha", 1.0))
        errs.append(_rel(buf[z, : mc[z], :n].cpu(), ref))
        # the wrong batch item's operand must miss
        zz = (z + 1) % Z
        wrong = {"operand of the next batch item": post((a[zz, : mc[z]].double() @ w[z, :n].double().t() + b[:n].double()) * c.get("alpha", 1.0))}
        if K1 is not None:
            mixed = torch.cat([a[z, : mc[z], :K1], a[zz, : mc[z], K1:]], 1).double()
            wrong["second slab of the next batch item"] = post((mixed @ w[z, :n].double().t() + b[:n].double()) * c.get("alpha", 1.0))
        _discriminates(buf[z, : mc[z], :n].cpu(), wrong, mode)
    _report(c["id"], mode, route, max(errs))
    assert max(errs) < _bar(mode), errs


# ------------------------------------------------------------------ ViT projections: q / k / v^T planes with RoPE2D (DUSt3R / MASt3R)
def _rope_tables(grids, rows):
    """cos / sin [rows][32] (entry 16 half + i: position of the y (half 0) / x (half 1) axis times 100^(-2i/32)) for the token
    grids laid out back to back; returns the tables, each grid's first row and its (y, x) positions."""
    inv = 1.0 / (100.0 ** (torch.arange(0, 32, 2).float() / 32))  # float32, as oracle/dust3r.py: rope2d
    ang = torch.zeros(rows, 32)
    starts, poss = [], []
    r0 = 0
    for gh, gw in grids:
        t = torch.arange(gh * gw)
        pos = torch.stack([t // gw, t % gw], 1)
        ang[r0 : r0 + gh * gw, :16] = pos[:, :1].float() * inv
        ang[r0 : r0 + gh * gw, 16:] = pos[:, 1:].float() * inv
        starts.append(r0)
        poss.append(pos)
        r0 += gh * gw
    return ang.cos(), ang.sin(), starts, poss


def _pairs_adjacent(t, pos):
    """A WRONG RoPE: feature i rotated with i + 1 (interleaved pairs) instead of i + 16."""
    inv = 1.0 / (100.0 ** (torch.arange(0, 32, 2).double() / 32))
    out = t.clone()
    for half in range(2):
        fr = pos[:, half].double()[:, None] * inv  # [N, 16]
        x = t[..., 32 * half : 32 * half + 32]
        a, b = x[..., 0::2], x[..., 1::2]
        out[..., 32 * half : 32 * half + 32 : 2] = a * fr.cos() - b * fr.sin()
        out[..., 32 * half + 1 : 32 * half + 32 : 2] = b * fr.cos() + a * fr.sin()
    return out


def feat_qkv_vit(c, kind):
    return mask_of(kind, "qkv_vit", len(c["cnt"]) * c["R"], (3 - c["role0"]) * 64 * c["heads"], c["K"], cnt=True, alpha=0.125, ln=c.get("ln_ratio") is not None,
                   wsel="wsel" in c)  # fmt: skip


def feat_qkv(c, kind):
    return mask_of(kind, "cross" if c["cross"] else "qkv", len(c["cnt"]) * c["R"], 512 if c["cross"] else 768, c["K"], cnt=True, alpha=0.18,
                   active="active" in c)  # fmt: skip


def run_qkv_vit(c, mode):
    from oracle.dust3r import rope2d

    be = _backend()
    heads, role0, R, K, cnts, grids = c["heads"], c["role0"], c["R"], c["K"], c["cnt"], c["grids"]
    Cw = 64 * heads
    nblk = 3 - role0
    N, nseq = nblk * Cw, len(cnts)
    M = nseq * R
    alpha = 0.125
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    x = torch.randn(M, K, generator=g)
    w = _weights(g, N, K)
    b = torch.randn(N, generator=g) * 0.1
    seq_grid = [s % len(grids) for s in range(nseq)]
    rows = max(a + R for a in _rope_tables(grids, 1 << 14)[2])
    cos, sin, starts, poss = _rope_tables(grids, rows)
    row0 = torch.tensor([starts[seq_grid[s]] for s in range(nseq)], dtype=torch.int32)
    ph = nseq * Cw * R
    planes = [torch.full((2 * ph + 64,), NAN_F16, dtype=torch.int16, device=DEV) for _ in range(3)]
    f = dict(epi="qkv_vit", A=x.to(DEV), lda=K, M=M, N=N, K=K, bias=b.to(DEV), alpha=alpha, cnt=torch.tensor(cnts, dtype=torch.int32).to(DEV),
             rows_per_seq=R, heads=heads, role0=role0, split_out=1, v_transposed=1, plane_halves=ph, Q=planes[0], Kt=planes[1], V=planes[2],
             rope_cos=cos.to(DEV), rope_sin=sin.to(DEV), rope_seq_row0=row0.to(DEV), **be.GemmWeights([w], DEV).fields(mode == 1))  # fmt: skip
    wsel = c.get("wsel")  # per pair of sequences: which of two weight sets (MASt3R's decoders); set 1 has its own scale and bias
    if wsel is not None:
        assert "ln_ratio" not in c and len(wsel) * 2 == nseq
        w1, b1 = _weights(g, N, K) * 8, torch.randn(N, generator=g) * 0.1
        wt2 = be.GemmWeights([w, w1], DEV)
        assert wt2.wscale[0] != wt2.wscale[1]
        f.update(wsel=torch.tensor(wsel, dtype=torch.int32).to(DEV), wsel_off=0, b_stride=N, bias=torch.cat([b, b1]).to(DEV), **wt2.fields(mode == 1))
    ln = c.get("ln_ratio")
    if ln is not None:
        x, w, b, gam, bet, fl = _ln_operands(g, N, M, K, ln, mode)
        f.update(A=x.to(DEV), **fl)
    route = _probe(lambda kind: feat_qkv_vit(c, kind), c["routes"][mode], **f)
    tiles = [math.ceil(n / 128) * 128 for n in cnts]  # rows written per sequence: whole 128-row tiles that hold a live row
    for t, p in enumerate(planes):
        role = t
        present = role0 <= role
        w4 = torch.zeros(2, nseq, heads, R, 64, dtype=torch.bool) if role < 2 else torch.zeros(2, nseq, heads, 64, R, dtype=torch.bool)
        if present and route is not None:
            for s in range(nseq):
                if role < 2:
                    w4[:, s, :, : tiles[s]] = True
                else:
                    w4[:, s, :, :, : tiles[s]] = True
        written = torch.cat([w4.reshape(-1), torch.zeros(64, dtype=torch.bool)])
        _untouched(p, written)
    if route is None:
        return _report(c["id"], mode, None, 0.0)
    xin = x.double()
    if ln is not None:
        xin = F.layer_norm(xin, (K,), gam.double(), bet.double(), eps=1e-6)
    y = xin @ w.double().t() + b.double()  # [M, N]
    y_other = None
    if wsel is not None:
        y1 = xin @ w1.double().t() + b1.double()
        pick = torch.tensor(wsel)[torch.arange(M) // R // 2].bool()[:, None]
        y, y_other = torch.where(pick, y1, y), torch.where(pick, y, y1)
    errs, wrong_errs = [], {}
    for blk in range(nblk):
        role = blk + role0
        yb = y[:, blk * Cw : (blk + 1) * Cw].reshape(nseq, R, heads, 64).permute(0, 2, 1, 3)  # [seq, head, row, 64]
        p = planes[role][: 2 * ph].cpu().numpy().view(np.float16).astype(np.float64).reshape(2, -1)
        got = torch.from_numpy(p[0] + p[1])
        got = got.reshape(nseq, heads, R, 64) if role < 2 else got.reshape(nseq, heads, 64, R).transpose(-1, -2)
        for s in range(nseq):
            n = cnts[s]
            if n == 0:
                continue
            pos = poss[seq_grid[s]][:n]
            ref = yb[s, :, :n]
            wrong = None
            if role < 2:
                wrong = _pairs_adjacent(ref, pos)
                ref = rope2d(ref[None], pos[None], 100.0)[0]
                if role == 0:
                    ref, wrong = ref * alpha, wrong * alpha
            e = _rel(got[s, :, :n], ref)
            errs.append(e)
            if wrong is not None:
                wrong_errs[f"RoPE pairs (i, i+1) role {role}"] = _discriminates(got[s, :, :n], {"rope": wrong}, mode)["rope"]
            if y_other is not None and role == 2:  # (v: no rotation between the product and the plane)
                yo = y_other[:, blk * Cw : (blk + 1) * Cw].reshape(nseq, R, heads, 64).permute(0, 2, 1, 3)[s, :, :n]
                wrong_errs["weight set of the other selection"] = _discriminates(got[s, :, :n], {"wsel": yo}, mode)["wsel"]
    err = max(errs)
    _report(c["id"], mode, route, err, wrong_errs)
    bar = _bar(mode) if ln is None or ln <= 4 else _ln_bound(ln, K)
    assert err < bar, (err, bar)
    return err


def run_qkv(c, mode):
    """LightGlue's SelfBlock (EPI_QKV: [q | k | v], rotary pairs (2j, 2j + 1) on q and k, q *= alpha) and CrossBlock (EPI_CROSS:
    [qk | v], qk *= alpha) projections, 4 heads: f16 hi / lo planes in the split mode, f32 head-major outputs in the exact mode."""
    be = _backend()
    cross, R, K, cnts = c["cross"], c["R"], c["K"], c["cnt"]
    nseq = len(cnts)
    M, N = nseq * R, (512 if cross else 768)
    alpha = 0.18
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    x = torch.randn(M, K, generator=g)
    w = _weights(g, N, K)
    b = torch.randn(N, generator=g) * 0.1
    ang = torch.rand(M, 32, generator=g) * 6.28
    cos, sin = ang.cos(), ang.sin()
    split = mode == 1
    nout = 2 if cross else 3
    per = nseq * 4 * R * 64
    outs = [torch.full(((2 * per + 64) if split else (per + 64),), NAN_F16 if split else NAN_F32, dtype=torch.int16 if split else torch.int32,
                       device=DEV) for _ in range(nout)]  # fmt: skip
    if not split:
        outs = [o.view(torch.float32) for o in outs]
    Q, Kt, V = (outs[0], None, outs[1]) if cross else outs
    f = dict(epi="cross" if cross else "qkv", A=x.to(DEV), lda=K, M=M, N=N, K=K, bias=b.to(DEV), alpha=alpha, cnt=torch.tensor(cnts, dtype=torch.int32).to(DEV),
             rows_per_seq=R, heads=4, split_out=int(split), v_transposed=1, plane_halves=per, Q=Q, Kt=Kt, V=V, rope_cos=cos.to(DEV),
             rope_sin=sin.to(DEV), **be.GemmWeights([w], DEV).fields(split))  # fmt: skip
    if "active" in c:  # per pair of sequences: an inactive pair launches no tile, whatever its counts
        assert 2 * len(c["active"]) == nseq
        f["active"] = torch.tensor(c["active"], dtype=torch.int32).to(DEV)
        cnts = [n if c["active"][s // 2] else 0 for s, n in enumerate(cnts)]
    y = x.double() @ w.double().t() + b.double()
    for opts, expect in c["routes"][mode]:
        for o in outs:
            o.view(torch.int16 if split else torch.int32).fill_(NAN_F16 if split else NAN_F32)
        with be.option(DEV, **opts):
            route = _probe(lambda kind: feat_qkv(c, kind), expect, **f)
        errs, wrong_errs = [], {}
        tile = {"wreg_mt1": 32, "wreg_mt2": 64}.get(expect[0], 128)  # row tile of the route: tiles whose first row is >= cnt are skipped
        for t, o in enumerate(outs):
            vt = t == nout - 1
            w5 = torch.zeros(2 if split else 1, nseq, 4, 64 if vt else R, R if vt else 64, dtype=torch.bool)
            for s in range(nseq):
                rows = min(R, -(-cnts[s] // tile) * tile)
                if vt:
                    w5[:, s, :, :, :rows] = True
                else:
                    w5[:, s, :, :rows] = True
            _untouched(o, torch.cat([w5.reshape(-1), torch.zeros(64, dtype=torch.bool)]))
            if split:
                a = o[: 2 * per].cpu().numpy().view(np.float16).astype(np.float64).reshape(2, -1)
                got = torch.from_numpy(a[0] + a[1])
            else:
                got = o[:per].cpu().double()
            got = got.reshape(nseq, 4, 64, R).transpose(-1, -2) if vt else got.reshape(nseq, 4, R, 64)
            ref = y[:, t * 256 : (t + 1) * 256].reshape(M, 4, 64)
            wrong = None
            if not cross and t < 2:
                cw, sw = cos.double()[:, None, :], sin.double()[:, None, :]
                e, o_ = ref[..., 0::2], ref[..., 1::2]
                rot = torch.empty_like(ref)
                rot[..., 0::2], rot[..., 1::2] = e * cw - o_ * sw, o_ * cw + e * sw
                h1, h2 = ref[..., :32], ref[..., 32:]  # the wrong convention: feature i rotated with i + 32 (rotate_half of the halves)
                wrong = torch.cat([h1 * cw - h2 * sw, h2 * cw + h1 * sw], -1)
                ref = rot
            if t == 0:
                ref = ref * alpha
                wrong = None if wrong is None else wrong * alpha
            ref = ref.reshape(nseq, R, 4, 64).permute(0, 2, 1, 3)
            wrong = None if wrong is None else wrong.reshape(nseq, R, 4, 64).permute(0, 2, 1, 3)
            for s in range(nseq):
                n = cnts[s]
                if n:
                    errs.append(_rel(got[s, :, :n], ref[s, :, :n]))
                    if wrong is not None:
                        wrong_errs[f"RoPE pairs (i, i+32) out {t}"] = _discriminates(got[s, :, :n], {"w": wrong[s, :, :n]}, mode)["w"]
        _report(c["id"], mode, route, max(errs), wrong_errs)
        assert max(errs) < _bar(mode), errs


def _ln_operands(g, N, M, K, ratio, mode):
    """Weights W [N, K] with random row sums (|sum_k W_nk| ~ |W_n|_2), bias b, raw rows x with |mean| / std = `ratio` exactly (a few
    outlier channels), LayerNorm gamma / beta, and the descriptor fields of the folded layer as the DUSt3R packer builds it: W gamma,
    b + W beta (backend._fold_layernorm), row sums of the folded f32 weights, and the per-row (mean, rstd) rounded to f32.
    Returns (x, W, b, gamma, beta, fields)."""
    be = _backend()
    b = torch.randn(N, generator=g) * 0.1
    w = torch.randn(N, K, generator=g) / math.sqrt(K) + torch.arange(N).float()[:, None] * (1e-4 / math.sqrt(K))  # row sums ~ |W_n|
    gam, bet = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    x = torch.randn(M, K, generator=g) + ratio * torch.sign(torch.randn(M, 1, generator=g))
    x[:, :3] *= 4  # outlier channels
    x64 = x.double()
    sd = x64.std(1, unbiased=False)
    x = (x64 + (ratio * sd - x64.mean(1).abs())[:, None] * torch.sign(x64.mean(1))[:, None]).float()  # |mean| = ratio * std exactly
    wf, bf = be._fold_layernorm(w, b, gam, bet)
    x64 = x.double()
    st = torch.stack([x64.mean(1), 1 / torch.sqrt(x64.var(1, unbiased=False) + 1e-6)], 1).float()
    fl = dict(ln_stats=st.to(DEV), ln_rowsum=wf.double().sum(1).float().to(DEV), bias=bf.to(DEV), **be.GemmWeights([wf], DEV).fields(mode == 1))
    return x, w, b, gam, bet, fl


def _ln_bound(ratio, K):
    """Error bound of the folded LayerNorm at |row mean| / row std = `ratio` (derived in test_layernorm_fold_sweep; independent of K)."""
    return 4e-6 + ratio * 8 * 2.0**-24


# ------------------------------------------------------------------ the case table
def _conv(id_, routes, **kw):
    return dict(id=id_, run=run_conv, routes=routes, **kw)


def _split_exact(kind, epi="conv"):
    return {1: (kind, epi), 0: ("exact", epi)}


def _mx(id_, routes, **kw):
    return dict(id=id_, run=run_matrix, routes=routes, **kw)


FEAT = {run_conv_batched: feat_conv_batched, run_conv: feat_conv, run_rup: feat_rup, run_matrix: feat_matrix, run_batched: feat_batched, run_qkv_vit: feat_qkv_vit, run_qkv: feat_qkv}

CASES = [
    # conv, pre-split planes: k in {1, 3, 5}, stride {1, 2} on odd sizes, Cin {32, 96, 256}, Cout {32, 64, 128, 256}, act 0-3, residual
    _conv("conv_k3_s1_c32_64_relu", _split_exact("conv_128"), B=2, H=13, W=17, cin=32, cout=64, k=3, stride=1, act=1),
    _conv("conv_k3_s2_c96_128_leaky_res", _split_exact("conv_128"), B=2, H=15, W=11, cin=96, cout=128, k=3, stride=2, act=2, resid=True),
    _conv("conv_k1_s1_c256_256_gelu_res", _split_exact("conv_256"), B=2, H=9, W=7, cin=256, cout=256, k=1, stride=1, act=3, resid=True),
    _conv("conv_k5_s1_c96_32_res", _split_exact("conv_128"), B=2, H=11, W=9, cin=96, cout=32, k=5, stride=1, resid=True),
    _conv("conv_k1_s2_c32_256", _split_exact("conv_256"), B=1, H=9, W=13, cin=32, cout=256, k=1, stride=2),
    _conv("conv_k5_s2_c32_64_relu", _split_exact("conv_128"), B=2, H=13, W=15, cin=32, cout=64, k=5, stride=2, act=1),
    _conv("conv_k3_s1_c256_128_gelu", _split_exact("conv_128"), B=1, H=7, W=9, cin=256, cout=128, k=3, stride=1, act=3),
    _conv("conv_f32_weights_split_on_the_fly", _split_exact("conv_f32b"), B=1, H=9, W=11, cin=32, cout=64, k=3, stride=1, act=1, planes=False),
    _conv("conv_single_narrow", {1: ("conv_128_single", "conv"), 0: ERR_ARG}, B=2, H=11, W=13, cin=96, cout=128, k=3, stride=1, act=1, resid=True, single=True),
    _conv("conv_single_wide", {1: ("conv_256_single", "conv"), 0: ERR_ARG}, B=2, H=9, W=11, cin=256, cout=256, k=3, stride=2, act=3, single=True),
    _conv("conv_single_k5", {1: ("conv_128_single", "conv"), 0: ERR_ARG}, B=1, H=9, W=7, cin=32, cout=64, k=5, stride=1, single=True),
    # output stride: DISK's 32-channel 5x5 layer into channels 64..95 of a 96-wide buffer; SuperPoint's 65-channel detector head
    _conv("ldc_disk_k5_n32_into_96_at_64", _split_exact("conv_128"), B=2, H=13, W=11, cin=96, cout=32, k=5, stride=1, ldc=96, col0=64),
    _conv("ldc_superpoint_n65_scalar_stores", _split_exact("conv_128"), B=2, H=7, W=9, cin=256, cout=65, k=1, stride=1),
    _conv("refuse_conv_cin_48", {1: ERR_ARG, 0: ERR_ARG}, B=1, H=5, W=5, cin=48, cout=64, k=3, stride=1),
    # bilinear x2 up-sampled residual: align_corners 1 (LoFTR) and 0 (EfficientLoFTR), 1 x w, h x 1, odd x odd, B = 2; exact mode refuses
    dict(id="rup_align1_odd", run=run_rup, routes={1: ("conv_128", "conv"), 0: ERR_ARG}, B=2, h=5, w=7, cin=32, cout=128, align=1, act=1),
    dict(id="rup_align0_odd", run=run_rup, routes={1: ("conv_128", "conv"), 0: ERR_ARG}, B=2, h=5, w=7, cin=64, cout=128, align=0),
    dict(id="rup_align1_1xw", run=run_rup, routes={1: ("conv_256", "conv"), 0: ERR_ARG}, B=2, h=1, w=9, cin=32, cout=256, align=1),
    dict(id="rup_align0_hx1", run=run_rup, routes={1: ("conv_128", "conv"), 0: ERR_ARG}, B=2, h=7, w=1, cin=32, cout=64, align=0),
    # GELU over -12..12 (both tails past the clamp of gelu_poly): exact, split and weights-in-registers kernels
    _mx("gelu_sweep", {0: [({}, ("exact", "conv"))], 1: [({"gemm_wreg": 0}, ("split_256", "conv")), ({"wreg_tile": 128}, ("wreg_pipe", "conv")),
                                                         ({}, ("wreg_mt1", "conv"))]},
        M=300, N=256, K=64, epi="conv", act=3, bias_sweep=12.0),
    _mx("gelu_sweep_narrow", {0: [({}, ("exact", "conv"))], 1: [({"gemm_wreg": 0}, ("split_128", "conv")), ({"wreg_tile": 32}, ("wreg_mt1", "conv"))]},
        M=130, N=192, K=32, epi="conv", act=3, bias_sweep=12.0),
    # weights in registers: 128 / 64 / 32-token tiles bitwise equal, the rolled loop, in-place residuals
    _mx("wreg_conv_tiles", {0: [({}, ("exact", "conv"))], 1: [({"wreg_tile": 128}, ("wreg_pipe", "conv")), ({"wreg_tile": 64}, ("wreg_mt2", "conv")),
                                                              ({"wreg_tile": 32}, ("wreg_mt1", "conv"))]},
        M=333, N=320, K=96, epi="conv", act=1, resid=True, bitwise=True),
    _mx("wreg_bias_tiles", {0: [({}, ("exact", "bias"))], 1: [({"wreg_tile": 128}, ("wreg_pipe", "bias")), ({"wreg_tile": 64}, ("wreg_mt2", "bias")),
                                                              ({"wreg_tile": 32}, ("wreg_mt1", "bias"))]},
        M=261, N=576, K=160, epi="bias", alpha=0.37, bitwise=True),
    _mx("wreg_relu_rolled", {0: [({}, ("exact", "relu"))], 1: [({"wreg_pipe": 0}, ("wreg_rolled", "relu")), ({}, ("wreg_pipe", "relu"))]},
        M=200, N=128, K=64, epi="relu"),
    _mx("wreg_conv_rolled_gelu", {0: [({}, ("exact", "conv"))], 1: [({"wreg_pipe": 0}, ("wreg_rolled", "conv"))]}, M=257, N=64, K=96, epi="conv", act=3),
    _mx("resid_in_place", {0: [({}, ("exact", "resid"))], 1: [({"wreg_tile": 128}, ("wreg_pipe", "resid")), ({"wreg_pipe": 0}, ("wreg_rolled", "resid")),
                                                              ({"gemm_wreg": 0}, ("split_128", "resid"))]},
        M=259, N=320, K=64, epi="resid", resid=True),
    _mx("resid_in_place_wide", {0: [({}, ("exact", "resid"))], 1: [({"gemm_wreg": 0}, ("split_256", "resid"))]}, M=131, N=512, K=32, epi="resid", resid=True),
    _mx("conv_resid_aliases_c", {0: [({}, ("exact", "conv"))], 1: [({"gemm_wreg": 0}, ("split_128", "conv")), ({}, ("wreg_mt1", "conv"))]},
        M=150, N=128, K=64, epi="conv", act=2, resid=True),
    _mx("bias_f32b_relu_ldc", {0: [({}, ("exact", "relu"))], 1: [({}, ("split_f32b", "relu"))]}, M=77, N=65, K=64, epi="relu", ldc=72, planes=False),
    _mx("bias_ldc_odd", {0: [({}, ("exact", "bias"))], 1: [({}, ("split_128", "bias"))]}, M=143, N=65, K=96, epi="bias", ldc=67, alpha=0.5),
    # matrix EPI_CONV in the single-product arithmetic (EfficientLoFTR / DUSt3R "fp16"): all four single instantiations
    _mx("single_matrix_wide", {0: [({}, ERR_ARG)], 1: [({"gemm_wreg": 0}, ("split_256_single", "conv")), ({}, ("wreg_pipe_single", "conv")),
                                                       ({"wreg_pipe": 0}, ("wreg_rolled_single", "conv"))]},
        M=300, N=256, K=128, epi="conv", act=3, single=True),
    _mx("single_matrix_narrow", {0: [({}, ERR_ARG)], 1: [({"gemm_wreg": 0}, ("split_128_single", "conv"))]}, M=170, N=96, K=64, epi="conv", act=1, single=True),
    _mx("refuse_single_without_planes", {0: [({}, ERR_ARG)], 1: [({}, ERR_ARG)]}, M=64, N=64, K=32, epi="conv", single=True, planes=False),
    # second K slab
    _mx("a2_k1_32", {0: [({}, ("exact", "bias"))], 1: [({}, ("split_128", "bias"))]}, M=300, N=192, K=256, epi="bias", K1=32, lda=36),
    _mx("a2_k1_k_minus_32", {0: [({}, ("exact", "relu"))], 1: [({}, ("split_256", "relu"))]}, M=133, N=256, K=256, epi="relu", K1=224, lda=228),
    # per-pair weight selection: three weight sets, pairs selecting alternately, wsel_off 0 and 1
    _mx("wsel_off0", {0: [({}, ("exact", "bias"))], 1: [({"gemm_wreg": 0}, ("split_128", "bias")), ({}, ("wreg_mt1", "bias"))]},
        M=768, N=192, K=64, epi="bias", sets=3, R=128, wsel=[0, 1, 0], wsel_off=0),
    _mx("wsel_off1", {0: [({}, ("exact", "conv"))], 1: [({"gemm_wreg": 0}, ("split_256", "conv")), ({"wreg_tile": 128}, ("wreg_pipe", "conv"))]},
        M=768, N=256, K=96, epi="conv", act=1, sets=3, R=128, wsel=[1, 0, 1], wsel_off=1),
    # batched with device-side counts: DISK's descriptor shape (K = 2400, N = 128, shared planes) and per-item f32 operands (ncnt)
    dict(id="batched_disk_descriptors", run=run_batched, routes=_split_exact("split_128", "bias"), batch=3, M=129, N=128, K=2400, mcnt=[0, 1, 129]),
    dict(id="batched_f32b_ragged_n", run=run_batched, routes=_split_exact("split_f32b", "bias"), batch=3, M=257, N=200, K=64, mcnt=[129, 0, 1],
         ncnt=[7, 200, 131], f32b=True, alpha=0.25),
    # EPI_QKV_VIT: heads 4 / 12 / 16, role0 0 (N = 3C) and 1 (N = 2C), ragged counts, two token grids through rope_seq_row0
    dict(id="qkv_vit_h4_role0", run=run_qkv_vit, routes={1: ("wreg_pipe", "qkv_vit"), 0: ERR_ARG}, heads=4, role0=0, R=256, K=96,
         cnt=[200, 128, 0, 77], grids=[(8, 25), (16, 8)]),
    dict(id="qkv_vit_h12_role1", run=run_qkv_vit, routes={1: ("wreg_pipe", "qkv_vit"), 0: ERR_ARG}, heads=12, role0=1, R=128, K=64,
         cnt=[128, 99], grids=[(8, 16), (11, 9)]),
    dict(id="qkv_vit_h16_role0", run=run_qkv_vit, routes={1: ("wreg_pipe", "qkv_vit"), 0: ERR_ARG}, heads=16, role0=0, R=128, K=64,
         cnt=[120, 128], grids=[(10, 12), (8, 16)]),
    # LightGlue / SuperGlue attention-layout projections (the qkv tests of test_gpu_round3_kernels.py compare the kernels; here: float64)
    dict(id="lightglue_qkv", run=run_qkv, routes={1: [({}, ("wreg_mt1", "qkv")), ({"wreg_tile": 64}, ("wreg_mt2", "qkv")),
                                                      ({"wreg_tile": 128}, ("wreg_pipe", "qkv")), ({"gemm_wreg": 0}, ("split_128", "qkv"))],
                                                  0: [({}, ("exact", "qkv"))]}, cross=False, R=256, K=256, cnt=[256, 130, 0, 77]),
    dict(id="lightglue_cross", run=run_qkv, routes={1: [({}, ("wreg_mt1", "cross")), ({"wreg_tile": 128}, ("wreg_pipe", "cross")),
                                                        ({"gemm_wreg": 0}, ("split_128", "cross"))],
                                                    0: [({}, ("exact", "cross"))]}, cross=True, R=128, K=256, cnt=[128, 5, 0, 128]),
    # folded LayerNorm at |mean| / std <= 4 (the sweep beyond is test_layernorm_fold_sweep); ln_stats off the wreg kernel is refused
    _mx("ln_fold_conv_ratio4", {0: [({}, ERR_UNSUPPORTED)], 1: [({"wreg_tile": 128}, ("wreg_pipe", "conv")), ({}, ("wreg_mt1", "conv"))]},
        M=256, N=256, K=256, epi="conv", act=3, ln=True, ln_ratio=4),
    _mx("refuse_ln_off_wreg", {0: [({}, ERR_UNSUPPORTED)], 1: [({"gemm_wreg": 0}, ERR_UNSUPPORTED)]}, M=128, N=128, K=64, epi="conv", ln=True, ln_ratio=0),
    dict(id="qkv_vit_ln_ratio4", run=run_qkv_vit, routes={1: ("wreg_pipe", "qkv_vit"), 0: ERR_ARG}, heads=4, role0=0, R=128, K=256,
         cnt=[128, 60], grids=[(8, 16), (6, 10)], ln_ratio=4),
    # the widths the fold serves: encoder qkv / fc1 K = 1024 (16 heads), decoder qkv / projq / projk / projv / fc1 K = 768 (12 heads)
    _mx("ln_fold_conv_k1024_ratio4", {0: [({}, ERR_UNSUPPORTED)], 1: [({"wreg_tile": 128}, ("wreg_pipe", "conv"))]},
        M=256, N=512, K=1024, epi="conv", act=3, ln=True, ln_ratio=4),
    _mx("ln_fold_conv_k768_ratio4", {0: [({}, ERR_UNSUPPORTED)], 1: [({"wreg_tile": 128}, ("wreg_pipe", "conv"))]},
        M=256, N=256, K=768, epi="conv", ln=True, ln_ratio=4),
    dict(id="qkv_vit_ln_k1024_ratio4", run=run_qkv_vit, routes={1: ("wreg_pipe", "qkv_vit"), 0: ERR_ARG}, heads=16, role0=0, R=128, K=1024,
         cnt=[128, 99], grids=[(8, 16), (11, 9)], ln_ratio=4),
    dict(id="qkv_vit_ln_k768_ratio4", run=run_qkv_vit, routes={1: ("wreg_pipe", "qkv_vit"), 0: ERR_ARG}, heads=12, role0=1, R=128, K=768,
         cnt=[60, 128], grids=[(6, 10), (8, 16)], ln_ratio=4),
    # ---- launches of the networks the gate found without a case once it was keyed on (route, feature) and ran every network
    # one long undilated sum (K >= GEMM_CHUNK_MIN_K; bar max(2e-6 / 4e-6, 2 E), E = float32 CPU torch): 3x3 at cin 512 (K = 4608: D2-Net, VGG,
    # ResNet layer4) on both column tiles, the bottleneck 1x1 as a matrix (K = N = 2048, one 7 x 7 map), a valid 8 x 8 convolution on an
    # 8 x 8 map (M = batch; HardNet's last layer as the architecture states it -- the backend runs that one as a batched matrix product)
    # measured on MI355X, device error / E: split 1.7e-06 / 7.9e-07 (cout 64), 1.9e-06 / 4.5e-07 (cout 512), 1.2e-06 / 3.8e-07 (matrix, both
    # kernels), 1.1e-06 / 7.1e-07 (valid 8 x 8): the 4e-6 bar holds without the 2 E term.  Exact mode, ONE summation chain (a build with the
    # two-level dispatch off): 1.93e-06 (cout 64), 2.74e-06 (cout 512: longk_k3_c512_512_relu MISSES 2e-6 = max(2e-6, 2 E)), 1.99e-06
    # (matrix), 1.42e-06 (valid 8 x 8); the K = 2400 / 2304 cases above 1.25e-06 and less.  Hence gemm_launch gives undilated exact launches
    # the two-level instantiation from K = GEMM_EXACT_CHUNK_MIN_K = 4096 on and only there: K = 4608 then measures 3.1e-07 / 4.4e-07, and
    # K = 2048 .. 2400 keeps one chain, the parent's instantiation and bits (the matrix case stays at 1.99e-06: deterministic, under the bar)
    _conv("longk_k3_c512_64", _split_exact("conv_128"), B=1, H=5, W=7, cin=512, cout=64, k=3, stride=1, long_k_bar=True),
    _conv("longk_k3_c512_512_relu", _split_exact("conv_256"), B=1, H=5, W=7, cin=512, cout=512, k=3, stride=1, act=1, tap_refs=True, long_k_bar=True),
    _mx("longk_matrix_k2048_n2048_m49", {0: [({}, ("exact", "conv"))], 1: [({}, ("wreg_mt1", "conv")), ({"gemm_wreg": 0}, ("split_256", "conv"))]},
        M=49, N=2048, K=2048, epi="conv", act=1, ramp=0.001, long_k_bar=True),  # (ramp: the row offset stays at two sigma at N = 2048)
    _conv("valid_k8_map8_m5", _split_exact("conv_128"), B=5, H=8, W=8, cin=32, cout=128, k=8, stride=1, pad=0, tap_refs=True, long_k_bar=True),
    # ResNet's strided launches: 1x1 stride 2 pad 0 shortcuts on odd and even maps, 3x3 stride 2 on an even map with residual + ReLU, N = 1024
    _conv("k1_s2_p0_even", _split_exact("conv_256"), B=2, H=8, W=12, cin=64, cout=256, k=1, stride=2, tap_refs=True),
    _conv("k1_s2_p0_odd_narrow", _split_exact("conv_128"), B=2, H=9, W=13, cin=64, cout=128, k=1, stride=2, tap_refs=True),
    _conv("k3_s2_even_res_relu_n1024", _split_exact("conv_256"), B=2, H=8, W=12, cin=64, cout=1024, k=3, stride=2, act=1, resid=True, tap_refs=True),
    # EfficientLoFTR's single-product launches: 1x1 with ReLU on 256-column tiles, 3x3 stride 2 on 128-column tiles
    _conv("single_k1_wide_relu", {1: ("conv_256_single", "conv"), 0: ERR_ARG}, B=2, H=9, W=7, cin=256, cout=256, k=1, stride=1, act=1, single=True),
    _conv("single_k3_s2_narrow", {1: ("conv_128_single", "conv"), 0: ERR_ARG}, B=2, H=9, W=12, cin=64, cout=64, k=3, stride=2, act=1, single=True, tap_refs=True),
    # output strides of the extractors: ALIKE / ALIKED residual 3x3 into a channel group of a wider buffer; XFeat's stride-2 3x3 at a padded
    # channel count (24 of 32 stored)
    _conv("ldc_alike_res_k3_n32_into_128_at_64", _split_exact("conv_128"), B=2, H=9, W=11, cin=32, cout=32, k=3, stride=1, act=1, resid=True, ldc=128, col0=64),
    _conv("ldc_xfeat_k3_s2_n24_of_32", _split_exact("conv_128"), B=2, H=10, W=14, cin=32, cout=24, k=3, stride=2, act=1, ldc=32, tap_refs=True),
    # DoG + HardNet / SOSNet: implicit im2col, batched, device-side row counts (none, one, all, inside the second 128-row tile)
    dict(id="conv_batched_mcnt", run=run_conv_batched, routes=_split_exact("conv_128"), batch=4, H=13, W=17, cin=32, cout=64, k=3, stride=1, act=1,
         mcnt=[0, 1, 221, 150]),
    dict(id="conv_batched_mcnt_s2_ldc", run=run_conv_batched, routes=_split_exact("conv_128"), batch=4, H=26, W=30, cin=32, cout=64, k=3, stride=2, act=1,
         ldc=72, mcnt=[195, 0, 129, 1]),
    # second K slab under EPI_CONV: DeDoDe's [features | context] layer (ReLU, K1 = 512 of 544; here N 72 inside ldc 80 and a partial row
    # tile) and MASt3R's on 256-column tiles
    _mx("a2_conv_dedode_ldc", {0: [({}, ("exact", "conv"))], 1: [({}, ("split_128", "conv"))]}, M=77, N=72, K=544, epi="conv", act=1, K1=512, lda=516, ldc=80),
    _mx("a2_conv_wide", {0: [({}, ("exact", "conv"))], 1: [({}, ("split_256", "conv"))]}, M=133, N=256, K=128, epi="conv", act=3, K1=64, lda=64),
    # ragged sequences and inactive pairs under the row-major epilogues (LightGlue / SuperGlue / DUSt3R token layers): 3 pairs of 128-row
    # sequences, the middle pair inactive; counts full, inside a tile, zero, one 32-row tile + 1
    _mx("ragged_bias_no_bias", {0: [({}, ("exact", "bias"))], 1: [({}, ("wreg_mt1", "bias")), ({"gemm_wreg": 0}, ("split_128", "bias"))]},
        M=768, N=192, K=64, epi="bias", alpha=0.5, bias=False, R=128, cnt=[128, 40, 128, 128, 0, 33], active=[1, 0, 1]),
    _mx("ragged_relu", {0: [({}, ("exact", "relu"))], 1: [({}, ("wreg_pipe", "relu"))]},
        M=768, N=256, K=64, epi="relu", R=128, cnt=[128, 40, 128, 128, 0, 33], active=[1, 0, 1]),
    _mx("ragged_resid_in_place", {0: [({}, ("exact", "resid"))], 1: [({}, ("wreg_pipe", "resid"))]},
        M=768, N=256, K=64, epi="resid", resid=True, R=128, cnt=[128, 40, 128, 128, 0, 33], active=[1, 0, 1]),
    _mx("ragged_conv_wsel_resid_gelu", {0: [({}, ("exact", "conv"))], 1: [({}, ("wreg_mt1", "conv"))]},
        M=512, N=192, K=96, epi="conv", act=3, resid=True, sets=3, R=128, wsel=[1, 0], wsel_off=1, cnt=[100, 128, 33, 0]),
    _mx("no_bias_f32b", {0: [({}, ("exact", "bias"))], 1: [({}, ("split_f32b", "bias"))]}, M=77, N=64, K=64, epi="bias", planes=False, bias=False),
    # DUSt3R's single-product token layers: ragged with an in-place residual and GELU; fc2 at K = 2048 on one partial row tile
    _mx("single_ragged_resid_gelu", {0: [({}, ERR_ARG)], 1: [({}, ("wreg_pipe_single", "conv"))]},
        M=256, N=192, K=128, epi="conv", act=3, resid=True, single=True, R=128, cnt=[128, 60]),
    _mx("single_k2048_m49_resid", {0: [({}, ERR_ARG)], 1: [({}, ("wreg_pipe_single", "conv"))]}, M=49, N=192, K=2048, epi="conv", resid=True, single=True),
    # LoFTR's transformer Linears: batched, two K slabs, device-side row counts, no bias, ReLU, on 256-column tiles
    dict(id="batched_a2_relu_no_bias", run=run_batched, routes=_split_exact("split_256", "relu"), batch=3, M=129, N=256, K=128, K1=64, epi="relu", bias=False,
         mcnt=[129, 0, 1]),
    # MASt3R: per-pair weight sets under EPI_QKV_VIT; LightGlue / SuperGlue: inactive pairs under the attention-layout projections
    dict(id="qkv_vit_wsel", run=run_qkv_vit, routes={1: ("wreg_pipe", "qkv_vit"), 0: ERR_ARG}, heads=4, role0=0, R=128, K=64,
         cnt=[128, 99, 60, 80], grids=[(8, 16), (11, 9)], wsel=[1, 0]),
    dict(id="lightglue_qkv_inactive_pair", run=run_qkv, routes={1: [({}, ("wreg_mt1", "qkv"))], 0: [({}, ("exact", "qkv"))]}, cross=False, R=128, K=256,
         cnt=[128, 77, 128, 100], active=[0, 1]),
    dict(id="lightglue_cross_inactive_pair", run=run_qkv, routes={1: [({}, ("wreg_mt1", "cross"))], 0: [({}, ("exact", "cross"))]}, cross=True, R=128, K=256,
         cnt=[90, 128, 128, 5], active=[1, 0]),
]


def _case_routes(c):
    out = set()
    for mode, r in c["routes"].items():
        for item in (r if isinstance(r, list) else [({}, r)]):
            if isinstance(item[1], tuple):
                out.add(item[1])
    return out


def covered_routes() -> set:
    be = _backend()
    return {be.gemm_route(*r) for c in CASES for r in _case_routes(c)}


def pairs_of(route: int, mask: int) -> set:
    """{(route, 0)} and (route, bit) for every GEMM_FEATURES bit of `mask`."""
    return {(route, 0)} | {(route, bit) for bit in _backend().GEMM_FEATURES.values() if mask & bit}


def covered_pairs() -> set:
    """{(route, feature bit or 0)} the launches of the case table record -- every case asserts its mask in _probe -- and those of
    tests/test_gpu_gemm_dilated.py (its table, through its own launch_features)."""
    import test_gpu_gemm_dilated as dil

    be = _backend()
    out = set()
    for c in CASES:
        for kind, epi in _case_routes(c):
            out |= pairs_of(be.gemm_route(kind, epi), FEAT[c["run"]](c, kind))
    for routes, args in dil.table_launches():
        for kind in routes.values():
            out |= pairs_of(be.gemm_route(kind, "conv"), dil.launch_features(kind, *args))
    return out


def pair_names(pairs) -> str:
    be = _backend()
    bit_name = {v: k for k, v in be.GEMM_FEATURES.items()}
    return ", ".join(f"{be.gemm_route_name(r)}+{bit_name[b]}" if b else be.gemm_route_name(r) for r, b in sorted(pairs))


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_gemm_variant(case, precision):
    case["run"](case, precision)


def test_layernorm_fold_sweep():
    """The LayerNorm folded into DUSt3R's layers: the kernel reads the RAW rows x = mean + std z, centres each row while staging it
    (x - mean, exact for x within a factor two of the mean) and scales the accumulator by rstd.  Centring is a decision, not a tuned
    threshold: the uncentred fold rstd (acc - mean rowsum) subtracted two terms of size |mean| |rowsum| after the f32 accumulation; every
    rounding on the way to acc (the f16 hi / lo split of x_k, the f32 accumulation) was relative to |x_k| ~ |mean| and the error grew as
    ratio = |mean| / std: 7e-7 per unit at K = 256, leaving 4e-6 near ratio 6 (K = 256) and 3 (K = 1024 by the sqrt(K) of the
    accumulation).  DUSt3R's pre-norm rows are not known to stay below that.
    Centred, the one rounding still relative to |mean| is that of the f32 mean in ln_stats: |d mean| <= 2^-24 |mean|, an error
    rstd d mean sum_k W_nk in output n.  With random row sums, max_n |sum_k W_nk| stays within ~4 max |reference| / std over a few
    thousand outputs, so
        err <= 4e-6 + ratio * 8 * 2^-24     (_ln_bound; every width), and 4e-6 itself up to ratio 16.
    Measured on MI355X (EPI_CONV / EPI_QKV_VIT), ratio 4: 6.2e-7 / 7.0e-7 (K 256), 8.4e-7 / 9.2e-7 (768), 8.7e-7 / 1.1e-6 (1024);
    ratio 16: 9.4e-7 / 9.4e-7, 1.4e-6 / 1.8e-6, 1.5e-6 / 2.5e-6; ratio 64: 3.8e-6 / 3.8e-6, 3.1e-6 / 5.9e-6, 2.9e-6 / 1.1e-5; ratio 256:
    1.0e-5 / 1.4e-5, 1.3e-5 / 2.5e-5, 1.0e-5 / 3.8e-5.  The uncentred fold measured 2.3e-6, 7.9e-6, 3.2e-5, 1.5e-4 at ratios 4 .. 256
    (K 256, EPI_CONV).
    The errors are printed for both epilogues that fold it (EPI_CONV, EPI_QKV_VIT) at the widths of the layers (768, 1024) and at 256."""
    rows = []
    for K, heads in ((256, 4), (768, 12), (1024, 16)):
        for ratio in (0, 4, 16, 64, 256):
            e1 = run_matrix(_mx(f"ln_sweep_conv_{K}_{ratio}", {1: [({"wreg_tile": 128}, ("wreg_pipe", "conv"))]}, M=256, N=256, K=K, epi="conv",
                                ln=True, ln_ratio=ratio), 1)  # fmt: skip
            e2 = run_qkv_vit(dict(id=f"ln_sweep_qkv_{K}_{ratio}", routes={1: ("wreg_pipe", "qkv_vit")}, heads=heads, role0=0, R=128, K=K,
                                  cnt=[128, 128], grids=[(8, 16), (16, 8)], ln_ratio=ratio), 1)  # fmt: skip
            rows.append((K, ratio, e1, e2))
            if ratio <= 16:
                assert max(e1, e2) < 4e-6, (K, ratio, e1, e2)
    for K, ratio, e1, e2 in rows:
        print(f"[ln-fold] K {K:4d} |mean|/std {ratio:4d}: EPI_CONV err {e1:.2e}  EPI_QKV_VIT err {e2:.2e}  (bound {_ln_bound(ratio, K):.1e}, "
              f"bar 4e-6 {'held' if max(e1, e2) < 4e-6 else 'exceeded'})")


# ------------------------------------------------------------------ the gate: every (route, feature) a network launches has a case above
@functools.lru_cache(maxsize=None)
def _extractor(name, variant=None):
    """The plugins of the sweep that are cheap to keep (seeded weights of imcui_hip/synth_weights.py), built once."""
    from imcui_hip import synth_weights as sw

    if name == "aliked":
        from imcui_hip.hloc.extractors.aliked import ALIKED

        return ALIKED({"state_dict": sw.aliked_state_dict(0), "max_num_keypoints": -1, "detection_threshold": 0.2, "nms_radius": 2}).eval().to(DEV)
    if name == "alike":
        from imcui_hip.hloc.extractors.alike import Alike

        return Alike({"model_name": variant, "state_dict": sw.alike_state_dict(variant, 0), "top_k": -1, "detection_threshold": 0.5,
                      "max_keypoints": 5000, "sub_pixel": False}).eval().to(DEV)  # fmt: skip
    if name == "xfeat":
        from imcui_hip.hloc.extractors.xfeat import XFeat

        return XFeat({"max_keypoints": -1, "state_dict": sw.xfeat_state_dict(0)}).eval().to(DEV)
    if name == "sift":
        from imcui_hip.hloc.extractors.sift import SIFT

        return SIFT({}).eval().to(DEV)
    if name == "r2d2":
        import r2d2_reference
        from imcui_hip.hloc.extractors.r2d2 import R2D2

        return R2D2({**r2d2_reference.DEFAULT_CONF, "state_dict": sw.r2d2_state_dict(0), "min_size": 8, "max_keypoints": 0}).eval().to(DEV)
    if name == "d2net":
        from imcui_hip.hloc.extractors.d2net import D2Net

        return D2Net({"state_dict": sw.d2net_state_dict(0), "use_relu": True, "max_keypoints": 0}).eval().to(DEV)
    if name == "dedode":
        from imcui_hip.hloc.extractors.dedode import DeDoDe

        det, desc = sw.dedode_state_dicts(0)
        return DeDoDe({"state_dict_detector": det, "state_dict_descriptor": desc, "max_keypoints": 64}).eval().to(DEV)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _packed(name, *args):
    from imcui_hip import backend
    from imcui_hip import synth_weights as sw

    if name == "netvlad":
        return backend.pack_netvlad(sw.netvlad_synth_state(0, whiten=args[0])).to(DEV)
    if name == "places":
        return backend.pack_places(sw.places_synth_state(*args, 0), *args).to(DEV)
    return backend.pack_hardnet(sw.hardnet_synth_state(0)).to(DEV)


def _rand(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def networks(mode):
    """[(name, it launches the shared GEMM in this mode, thunk)]: every network of the tree once, at the smallest size its own parity test
    uses, with the seeded weights of imcui_hip/synth_weights.py; a variant of a network is listed when its launches differ in shape.

    SuperPoint + LightGlue, DISK, SuperGlue, LoFTR, EfficientLoFTR (fp32 and fp16), DUSt3R (fp32 and fp16) and MASt3R (split mode only);
    ALIKED (96 x 128, and two images of 480 x 640: the deformable products pick their row tile by the pixel count), SIFT and NetVLAD (no
    launch of the shared GEMM -- NetVLAD's trunk runs on conv.hip, its head on kernels of its own: they are run so that the gates say so
    and for the convolution gate), XFeat, ALIKE-t / -s / -n (32 x 40 and two images of 160 x 224), R2D2 (24 x 40, three pyramid levels),
    D2-Net single-scale (32 x 48) and multi-scale (48 x 64), DeDoDe (detector L and descriptor B in one call, three images of 32 x 48),
    NetVLAD with and without whitening, DoG + HardNet (257, 0 and 33 key-points on three images: ragged device-side counts),
    CosPlace on ResNet-18 / 512 (basic blocks) and ResNet-50 / 2048 (bottlenecks) at 32 x 48.
    Left out, because their launch lists are those of a variant that runs: DoG + SOSNet (the launch list of HardNet -- csrc/dog.hip runs
    both through dg_net with one layer table; run side by side, the recorder showed the same (route, mask) set in both modes), RoRD
    (the D2-Net class and network with other weights),
    EigenPlaces (CosPlace's network), CosPlace on ResNet-101 / -152 (the bottleneck shapes of ResNet-50, more blocks), the other NetVLAD
    checkpoints (one architecture).  test_routes_of_every_network_are_covered prints, per network, the pairs it adds."""
    from imcui_hip import backend
    from imcui_hip.hloc.extractors.disk import DISK
    from imcui_hip.hloc.matchers.duster import Duster
    from imcui_hip.hloc.matchers.eloftr import ELoFTR
    from imcui_hip.hloc.matchers.loftr import LoFTR
    from imcui_hip.hloc.matchers.mast3r import Mast3r
    from imcui_hip.hloc.matchers.superglue import SuperGlue
    from imcui_hip.pipeline import SuperPointLightGluePipeline
    from imcui_hip.synth import make_pair_batch, make_shifted_pair
    from imcui_hip.synth_weights import (disk_state_dict, dust3r_state_dict, eloftr_state_dict, lightglue_state_dict, loftr_state_dict,
                                         superglue_state_dict, superpoint_state_dict)  # fmt: skip

    def superpoint_lightglue():
        img0, img1, _ = make_pair_batch(1, 1, 120, 160, n_blobs=150)
        spc = dict(nms_radius=3, max_keypoints=256, keypoint_threshold=0.005, remove_borders=4)
        pipe = SuperPointLightGluePipeline({**spc, "state_dict": superpoint_state_dict(0)},
                                           {"depth_confidence": 0.95, "width_confidence": 0.99, "match_threshold": 0.1, "state_dict": lightglue_state_dict(0)})
        pipe.eval().to(DEV)(img0.to(DEV), img1.to(DEV))

    def disk():
        DISK({"max_keypoints": 256, "state_dict": disk_state_dict(0)}).eval().to(DEV).forward_batched(torch.rand(1, 3, 480, 640).to(DEV))

    def superglue():
        g = torch.Generator().manual_seed(0)
        n = 200
        k = torch.rand(1, n, 2, generator=g) * torch.tensor([630.0, 470.0]) + 5
        d = F.normalize(torch.randn(1, n, 256, generator=g), dim=-1)
        s = torch.rand(1, n, generator=g)
        nn = torch.tensor([n], dtype=torch.int32)
        sg = SuperGlue({"sinkhorn_iterations": 5, "match_threshold": 0.2, "state_dict": superglue_state_dict(0)}).eval().to(DEV)
        sg.forward_batched(k.to(DEV), k.flip(1).to(DEV), s.to(DEV), s.to(DEV), d.to(DEV), d.flip(1).to(DEV), nn.to(DEV), nn.to(DEV), (640, 480), (640, 480))

    def loftr():
        a, b, _ = make_shifted_pair(3, 96, 160, (16, 8), n_blobs=300)
        LoFTR({"match_threshold": 0.2, "max_keypoints": None, "state_dict": loftr_state_dict(0)}).eval().to(DEV).forward_batched(
            torch.cat([a, a]).to(DEV), torch.cat([b, b]).to(DEV))

    def eloftr():
        a, b, _ = make_shifted_pair(11, 160, 224, (16, 8), n_blobs=300)
        for prec in ("fp32", "fp16") if mode == 1 else ("fp32",):
            ELoFTR({"match_threshold": 0.2, "max_keypoints": None, "state_dict": eloftr_state_dict(0), "precision": prec}).eval().to(DEV).forward_batched(
                torch.cat([a, a]).to(DEV), torch.cat([b, b]).to(DEV))

    small = {"enc_dim": 512, "enc_depth": 2, "dec_dim": 256, "dec_depth": 4}

    def dust3r():  # DUSt3R / MASt3R run the split arithmetic (parity) or the single-product one (fp16)
        du = Duster({"state_dict": dust3r_state_dict(0, small)}).eval().to(DEV)
        imgs = torch.rand(2, 3, 160, 224).to(DEV)
        for arith in ("fp32", "fp16"):
            du.conf["arithmetic"] = arith
            du.forward_pairs(imgs, [[0, 1]])

    def mast3r():
        ma = Mast3r({"state_dict": dust3r_state_dict(2, {**small, "desc_dim": 24})}).eval().to(DEV)
        ma.inference_output({"image0": torch.rand(1, 3, 128, 192).to(DEV), "image1": torch.rand(1, 3, 128, 192).to(DEV)})

    def aliked():
        _extractor("aliked").forward_batched(_rand(1, 3, 96, 128, seed=3))
        _extractor("aliked").forward_batched(_rand(2, 3, 480, 640, seed=0))

    def alike(variant):
        def run():
            _extractor("alike", variant).forward_batched(_rand(1, 3, 32, 40, seed=11))
            _extractor("alike", variant).forward_batched(_rand(2, 3, 160, 224, seed=3))

        return run

    def sift():
        _extractor("sift").forward_batched(_rand(1, 1, 97, 131, seed=0))

    def d2net(ms, hw):
        def run():
            m = _extractor("d2net")
            m.conf.update(multiscale=ms)
            m.forward_batched(_rand(1, 3, *hw, seed=100))

        return run

    def netvlad(whiten):
        return lambda: backend.NetVLADHIP().forward_batched(_packed("netvlad", whiten), _rand(2, 3, 32, 48, seed=32), whiten)

    def places(backbone, dim):
        return lambda: backend.PlacesHIP(backbone, dim).forward_batched(_packed("places", backbone, dim), _rand(2, 3, 32, 48, seed=32048))

    def patchdesc(name):
        def run():
            g = torch.Generator().manual_seed(7)
            cnt = torch.tensor([257, 0, 33], dtype=torch.int32)
            kp = torch.rand(3, 257, 2, generator=g) * torch.tensor([84.0, 95.0]) + torch.tensor([45.0, 0.0])
            sc = 1.2 * 10.0 ** torch.rand(3, 257, generator=g)
            od = torch.rand(3, 257, generator=g) * 360.0 - 180.0
            backend.PatchDescHIP().forward(_packed(name), _rand(3, 1, 96, 130, seed=100), kp.to(DEV), sc.to(DEV), od.to(DEV), cnt.to(DEV), name)

        return run

    nets = [("SuperPoint+LightGlue", True, superpoint_lightglue), ("DISK", True, disk), ("SuperGlue", True, superglue), ("LoFTR", True, loftr),
            ("EfficientLoFTR", True, eloftr)]  # fmt: skip
    if mode == 1:
        nets += [("DUSt3R", True, dust3r), ("MASt3R", True, mast3r)]
    nets += [("ALIKED", True, aliked), ("SIFT", False, sift), ("XFeat", True, lambda: _extractor("xfeat").forward_batched(_rand(1, 3, 64, 64, seed=0))),
             ("ALIKE-t", True, alike("alike-t")), ("ALIKE-s", True, alike("alike-s")), ("ALIKE-n", True, alike("alike-n")),
             ("R2D2", True, lambda: _extractor("r2d2").forward_batched(_rand(1, 3, 24, 40, seed=0), kcap="all")),
             ("D2-Net ss", True, d2net(False, (32, 48))), ("D2-Net ms", True, d2net(True, (48, 64))),
             ("DeDoDe", True, lambda: _extractor("dedode").forward_batched(_rand(3, 3, 32, 48, seed=103))),
             ("NetVLAD", False, netvlad(False)), ("NetVLAD whitened", False, netvlad(True)),
             ("DoG+HardNet", True, patchdesc("hardnet")),
             ("CosPlace ResNet-18", True, places(18, 512)), ("CosPlace ResNet-50", True, places(50, 2048))]  # fmt: skip
    return nets


def _run_networks(mode, after=None):
    """Every network of networks(mode) once in the arithmetic mode `mode`; after(name), when given, runs once the network's work is done."""
    _backend().set_precision(DEV, mode)
    for name, _, run in networks(mode):
        run()
        if after is not None:
            torch.cuda.synchronize()
            after(name)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def network_sweep():
    """ONE pass over every network in both arithmetic modes that collects all four route recorders (shared GEMM, attention, 3x3 convolution,
    fused FFN) per network; the four gates read it.  {(mode, name): {"uses_gemm", "seconds", "gemm": {route: (launches, feature mask)},
    "conv": {route: (launches, feature mask)}, "attn": {route: launches}, "ffn": {route: launches}}}."""
    be = _backend()
    out = {}
    resets = (be.gemm_route_reset, be.attn_route_reset, be.conv_route_reset, be.ffn_route_reset)
    try:
        for mode in (1, 0):
            uses = {name: u for name, u, _ in networks(mode)}
            t0 = [time.perf_counter()]

            def after(name):
                gf, cf = be.gemm_route_features(DEV), be.conv_route_features(DEV)
                out[(mode, name)] = {"uses_gemm": uses[name], "seconds": time.perf_counter() - t0[0],
                                     "gemm": {r: (n, gf.get(r, 0)) for r, n in be.gemm_route_counts(DEV).items()},
                                     "conv": {r: (n, cf.get(r, 0)) for r, n in be.conv_route_counts(DEV).items()},
                                     "attn": be.attn_route_counts(DEV), "ffn": be.ffn_route_counts(DEV)}  # fmt: skip
                for reset in resets:
                    reset(DEV)
                t0[0] = time.perf_counter()

            for reset in resets:
                reset(DEV)
            _run_networks(mode, after)
    finally:
        be.set_precision(DEV, 1)
    return out


def test_routes_of_every_network_are_covered():
    """Every network of the tree (networks()) once in each arithmetic mode it offers, the recorder read and reset after each: every
    (route, feature bit) pair a network launched must be one a case of the table (or of tests/test_gpu_gemm_dilated.py) launches and
    checks against float64, and every network that uses the shared GEMM must have recorded a launch.  A new instantiation, or a known one
    launched with a feature no case runs it with, fails here.  Prints, per network, its launch count and its pairs.
    On the case tables as they stood before the gate was keyed on features and widened (and before undilated exact launches with
    K >= 4096 summed in two levels: those now record `chunk`), it reported these 55 pairs as launched without a case:
    conv_128/conv+conv_batched, conv_128/conv+mcnt, conv_128_single/conv+stride2, conv_256/conv+act1, conv_256/conv+conv_k3,
    conv_256/conv+long_k, conv_256_single/conv+act1, conv_256_single/conv+conv_k1, convd_128/conv+chunk, exact/bias+active,
    exact/bias+cnt, exact/bias+no_bias, exact/conv+a2, exact/conv+conv_batched, exact/conv+mcnt, exact/cross+active,
    exact/qkv+active, exact/relu+active, exact/relu+batch, exact/relu+cnt, exact/relu+mcnt, exact/relu+no_bias, exact/resid+active,
    exact/resid+cnt, exact_dil/conv+chunk, split_128/bias+no_bias, split_128/conv+a2, split_128/conv+act1, split_128/conv+ldc,
    split_128/conv+m_small, split_128/conv+n_mod32, split_256/conv+a2, split_256/relu+batch, split_256/relu+mcnt,
    split_256/relu+no_bias, split_f32b/bias+no_bias, wreg_mt1/bias+active, wreg_mt1/bias+cnt, wreg_mt1/bias+no_bias,
    wreg_mt1/conv+cnt, wreg_mt1/conv+long_k, wreg_mt1/conv+m_small, wreg_mt1/conv+wsel, wreg_mt1/cross+active, wreg_mt1/qkv+active,
    wreg_pipe/qkv_vit+wsel, wreg_pipe/relu+active, wreg_pipe/relu+cnt, wreg_pipe/resid+active, wreg_pipe/resid+cnt,
    wreg_pipe_single/conv+cnt, wreg_pipe_single/conv+long_k, wreg_pipe_single/conv+m_small, wreg_pipe_single/conv+n_mod_tile,
    wreg_pipe_single/conv+resid"""
    be = _backend()
    t0 = time.perf_counter()
    sweep = network_sweep()
    cov = covered_pairs()
    seen, idle = set(), []
    for (mode, name), rec in sweep.items():
        pairs = set()
        for r, (n, mask) in rec["gemm"].items():
            pairs |= pairs_of(r, mask)
        launches = sum(n for n, _ in rec["gemm"].values())
        print(f"[gemm-gate] mode {mode} {name}: {launches} launches in {rec['seconds']:.2f} s; new pairs: {pair_names(pairs - seen) or '-'}"
              + (f"; WITHOUT A CASE: {pair_names(pairs - cov)}" if pairs - cov else ""))  # fmt: skip
        seen |= pairs
        if rec["uses_gemm"] and not launches:
            idle.append(f"{name} (mode {mode})")
    print(f"[gemm-gate] {len(seen)} (route, feature) pairs launched by the networks, {len(cov)} covered by the case tables; the networks of the "
          f"sweep took {sum(rec['seconds'] for rec in sweep.values()):.1f} s (once per session), this gate {time.perf_counter() - t0:.1f} s")  # fmt: skip
    print("[gemm-gate] (route, feature) launched by the networks: " + pair_names(seen))
    assert not idle, "no GEMM launch recorded for: " + ", ".join(idle)
    missing = seen - cov
    assert not missing, "launched without a kernel-level case: " + pair_names(missing)
