"""Every instantiation of the shared GEMM (csrc/gemm.hip, csrc/gemm_wreg.hip) that the networks launch, entered directly through
imcui_hip_gemm_probe_f32 and compared with a plain float64 restatement of the same operation.

One case table (CASES).  Every case names the kernel instantiation it targets per arithmetic mode -- or the refusal it expects -- and
asserts it through the route the launch site recorded (imcui_hip_gemm_last_route).  Every case then checks three things:
  * the result against float64 within the building-block bars, relative to max |reference|: 2e-6 exact f32, 4e-6 otherwise.  The
    single-product variants are compared with float64 on the operands rounded the way gemm.hip documents (nearest-even f16 of the
    scaled weight, saturating nearest-even f16 of the activation), with the same 4e-6 bar;
  * memory the kernel must not write (NaN sentinels with a private payload: columns past N inside ldc, rows past M, rows past the
    device-side row counts, skipped tiles of ragged sequences, plane padding) is bitwise unchanged;
  * a plausible wrong reference for each fused feature misses the bar (the inputs can tell the difference).
test_routes_of_every_network_are_covered runs every network once and fails on a route the table does not cover."""
from __future__ import annotations

import math
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


def _weights(g, N, K, scale=None):
    """Random weights with a row-dependent offset: a transposed or shifted store cannot pass."""
    s = scale if scale is not None else 1.0 / math.sqrt(K)
    return torch.randn(N, K, generator=g) * s + torch.arange(N).float()[:, None] * (0.01 * s)


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


def _probe(expect, **fields):
    """Launch; `expect` is a route (kind, epi) or a negative refusal code.  Returns the route."""
    be = _backend()
    if isinstance(expect, int):
        rc = be.gemm_probe(DEV, check=False, **fields)
        assert rc == expect, f"expected refusal {expect}, got {rc}"
        assert be.get_handle(DEV).lib.imcui_hip_gemm_last_route(be.get_handle(DEV).h) == 0
        return None
    r = be.gemm_probe(DEV, **fields)
    torch.cuda.synchronize()
    assert r == be.gemm_route(*expect), f"route {be.gemm_route_name(r)}, expected {expect}"
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
def run_conv(c, mode):
    be = _backend()
    B, H, W, cin, cout, k, st = c["B"], c["H"], c["W"], c["cin"], c["cout"], c["k"], c["stride"]
    act, use_res, single, planes = c.get("act", 0), c.get("resid", False), c.get("single", False), c.get("planes", True)
    ldc, col0 = c.get("ldc", cout), c.get("col0", 0)
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k) + torch.arange(cout).float()[:, None, None, None] * 1e-3
    b = torch.randn(cout, generator=g) * 0.1
    pad = k // 2
    ho, wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    M = B * ho * wo
    wt = be.GemmWeights.conv([w], DEV)
    res = torch.randn(M, cout, generator=g) if use_res else None
    buf = _sentinel(M + 3, ldc)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    f = dict(epi="conv", A=xd, conv_k=k, conv_stride=st, conv_pad=pad, conv_hin=H, conv_win=W, conv_hout=ho, conv_wout=wo, conv_cin=cin,
             K=k * k * cin, M=M, N=cout, C=buf[:, col0:], ldc=ldc, bias=b.to(DEV), act=act, single=int(single),
             resid=None if res is None else res.to(DEV), ldr=cout, **wt.fields(mode == 1, planes))  # fmt: skip
    route = _probe(c["routes"][mode], **f)
    written = torch.zeros(M + 3, ldc, dtype=torch.bool)
    if route is not None:
        written[:M, col0 : col0 + cout] = True
    _untouched(buf, written)
    if route is None:
        return _report(c["id"], mode, None, 0.0)
    out = buf[:M, col0 : col0 + cout].cpu()
    xs, ws = (x.double(), w.double()) if not single else (_round_act(x), _round_single(w, wt.wscale[0].item()))

    def ref_of(r):
        y = F.conv2d(xs, ws, b.double(), stride=st, padding=pad).permute(0, 2, 3, 1).reshape(M, cout)
        return _act(y + (0 if r is None else r), act)

    ref = ref_of(None if res is None else res.double())
    err = _rel(out, ref)
    wrong = {}
    if res is not None:
        r_row, r_col = res.double().clone(), res.double().clone()
        r_row[-1] = 0
        r_col[:, -1] = 0
        wrong = _discriminates(out, {"residual dropped on the last row": ref_of(r_row), "residual dropped on the last column": ref_of(r_col)}, mode)
    _report(c["id"], mode, route, err, wrong)
    assert err < _bar(mode), err


# ------------------------------------------------------------------ bilinear x2 up-sampled residual (LoFTR / EfficientLoFTR FPN)
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
    route = _probe(c["routes"][mode], **f)
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
def run_matrix(c, mode):
    """Row-major A [M, K] (optionally a second K slab), C = epi(A W^T + bias) with the case's extras."""
    be = _backend()
    M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    nsets = c.get("sets", 1)
    ws = [_weights(g, N, K) for _ in range(nsets)]
    bs = [torch.randn(N, generator=g) * 0.1 for _ in range(nsets)]
    if nsets > 1:
        ws[1] = ws[1] * 8  # a power of two: set 1 packs with its own scale 2^-e (wscale[1] = 8 wscale[0])
    if "bias_sweep" in c:
        ws = [w * 0.01 for w in ws]
        bs = [torch.linspace(-c["bias_sweep"], c["bias_sweep"], N)]
    wt = be.GemmWeights(ws, DEV)
    lda = c.get("lda", K)
    K1 = c.get("K1")
    a = torch.randn(M, K, generator=g)
    ldc = c.get("ldc", N)
    act, single = c.get("act", 0), c.get("single", False)
    buf = _sentinel(M + 2, ldc)
    f = dict(epi=epi, M=M, N=N, K=K, C=buf, ldc=ldc, act=act, single=int(single), alpha=c.get("alpha", 1.0), bias=torch.cat(bs).to(DEV),
             **wt.fields(mode == 1, c.get("planes", True)))  # fmt: skip
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
    if nsets > 1:
        R = c["R"]
        wsel = torch.tensor(c["wsel"], dtype=torch.int32)
        sel = (wsel.long()[torch.arange(M) // R // 2] + c["wsel_off"])
        f.update(rows_per_seq=R, wsel=wsel.to(DEV), wsel_off=c["wsel_off"], b_stride=N)
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
    written = torch.zeros(M + 2, ldc, dtype=torch.bool)
    snapshot = buf.clone()
    route = None
    runs = []
    for opts, expect in c["routes"][mode]:
        buf.copy_(snapshot)
        with be.option(DEV, **opts):
            route = _probe(expect, **f)
        runs.append((route, buf[:M, :N].cpu().clone()))
    if runs[0][0] is not None:
        written[:M, :N] = True
    else:
        written[:M, :N] = res is not None  # the pre-loaded residual
    _untouched(buf, written)
    if runs[0][0] is None:
        return _report(c["id"], mode, None, 0.0)
    a64 = a.double() if not c.get("ln") else F.layer_norm(a.double(), (K,), gam.double(), bet.double(), eps=1e-6)
    wsel_sets = torch.stack([w.double() for w in ws])
    bsel = torch.stack([b.double() for b in bs])
    if single:
        a64 = _round_act(a)
        wsel_sets = torch.stack([_round_single(w, wt.wscale[i].item()) for i, w in enumerate(ws)])

    def ref_of(selv, drop_last_col=False):
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
    bar = _bar(mode) if not c.get("ln") or ratio <= 4 else _ln_bound(ratio, K)
    worst = 0.0
    for route, out in runs:
        err = _rel(out, ref)
        if nsets > 1:  # sets of different magnitude: each pair relative to its own output
            pair = torch.arange(M) // c["R"] // 2
            err = max(_rel(out[pair == p], ref[pair == p]) for p in range(int(pair.max()) + 1))
        errs = _discriminates(out, wrong, mode) if wrong else {}
        _report(c["id"], mode, route, err, errs)
        assert err < bar, (err, bar)
        worst = max(worst, err)
    if c.get("bitwise"):
        for _, out in runs[1:]:
            assert torch.equal(out, runs[0][1]), "the token tiles are documented bitwise equal"
    return worst


# ------------------------------------------------------------------ batched: device-side row / column counts per batch item
def run_batched(c, mode):
    be = _backend()
    Z, M, N, K = c["batch"], c["M"], c["N"], c["K"]
    mc, nc = c["mcnt"], c.get("ncnt")
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    a_bs, c_bs = (M + 5) * K, (M + 3) * N
    a = torch.randn(Z, M + 5, K, generator=g)
    buf = _sentinel(Z, M + 3, N)
    b = torch.randn(N, generator=g) * 0.1
    cnt = torch.tensor([v for pair in zip(mc, nc or mc) for v in pair], dtype=torch.int32)  # (m, n) interleaved: cnt_stride 2
    f = dict(epi="bias", A=a.to(DEV), lda=K, M=M, N=N, K=K, C=buf, ldc=N, c_bs=c_bs, a_bs=a_bs, batch=Z, bias=b.to(DEV),
             mcnt=cnt.to(DEV), cnt_stride=2, alpha=c.get("alpha", 1.0))  # fmt: skip
    if c.get("f32b"):
        w = torch.stack([_weights(g, N, K) for _ in range(Z)])
        f.update(W=w.to(DEV), ldw=K, w_bs=N * K)
        if nc is not None:
            f["ncnt"] = cnt[1:].to(DEV)
    else:
        w = _weights(g, N, K)[None].expand(Z, N, K)
        f.update(be.GemmWeights([w[0]], DEV).fields(mode == 1))
    route = _probe(c["routes"][mode], **f)
    written = torch.zeros(Z, M + 3, N, dtype=torch.bool)
    for z in range(Z):
        written[z, : mc[z], : (nc[z] if nc else N)] = True
    _untouched(buf, written)
    errs = []
    for z in range(Z):
        if mc[z] == 0:
            continue
        n = nc[z] if nc else N
        ref = (a[z, : mc[z]].double() @ w[z, :n].double().t() + b[:n].double()) * c.get("alpha", 1.0)
        errs.append(_rel(buf[z, : mc[z], :n].cpu(), ref))
        # the wrong batch item's operand must miss
        zz = (z + 1) % Z
        _discriminates(buf[z, : mc[z], :n].cpu(), {"operand of the next batch item": (a[zz, : mc[z]].double() @ w[z, :n].double().t() + b[:n].double()) * c.get("alpha", 1.0)}, mode)
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
    ln = c.get("ln_ratio")
    if ln is not None:
        x, w, b, gam, bet, fl = _ln_operands(g, N, M, K, ln, mode)
        f.update(A=x.to(DEV), **fl)
    route = _probe(c["routes"][mode], **f)
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
    y = x.double() @ w.double().t() + b.double()
    for opts, expect in c["routes"][mode]:
        for o in outs:
            o.view(torch.int16 if split else torch.int32).fill_(NAN_F16 if split else NAN_F32)
        with be.option(DEV, **opts):
            route = _probe(expect, **f)
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


# ------------------------------------------------------------------ the gate: every route a network launches has a case above
def _run_networks(mode):
    """Each network once, at the smallest size its parity test uses."""
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

    backend.set_precision(DEV, mode)
    img0, img1, _ = make_pair_batch(1, 1, 120, 160, n_blobs=150)
    spc = dict(nms_radius=3, max_keypoints=256, keypoint_threshold=0.005, remove_borders=4)
    pipe = SuperPointLightGluePipeline({**spc, "state_dict": superpoint_state_dict(0)},
                                       {"depth_confidence": 0.95, "width_confidence": 0.99, "match_threshold": 0.1, "state_dict": lightglue_state_dict(0)})
    pipe.eval().to(DEV)(img0.to(DEV), img1.to(DEV))
    DISK({"max_keypoints": 256, "state_dict": disk_state_dict(0)}).eval().to(DEV).forward_batched(torch.rand(1, 3, 480, 640).to(DEV))
    g = torch.Generator().manual_seed(0)
    n = 200
    k = torch.rand(1, n, 2, generator=g) * torch.tensor([630.0, 470.0]) + 5
    d = F.normalize(torch.randn(1, n, 256, generator=g), dim=-1)
    s = torch.rand(1, n, generator=g)
    nn = torch.tensor([n], dtype=torch.int32)
    sg = SuperGlue({"sinkhorn_iterations": 5, "match_threshold": 0.2, "state_dict": superglue_state_dict(0)}).eval().to(DEV)
    sg.forward_batched(k.to(DEV), k.flip(1).to(DEV), s.to(DEV), s.to(DEV), d.to(DEV), d.flip(1).to(DEV), nn.to(DEV), nn.to(DEV), (640, 480), (640, 480))
    a, b, _ = make_shifted_pair(3, 96, 160, (16, 8), n_blobs=300)
    LoFTR({"match_threshold": 0.2, "max_keypoints": None, "state_dict": loftr_state_dict(0)}).eval().to(DEV).forward_batched(
        torch.cat([a, a]).to(DEV), torch.cat([b, b]).to(DEV))
    a, b, _ = make_shifted_pair(11, 160, 224, (16, 8), n_blobs=300)
    for prec in ("fp32", "fp16") if mode == 1 else ("fp32",):
        ELoFTR({"match_threshold": 0.2, "max_keypoints": None, "state_dict": eloftr_state_dict(0), "precision": prec}).eval().to(DEV).forward_batched(
            torch.cat([a, a]).to(DEV), torch.cat([b, b]).to(DEV))
    if mode == 1:  # DUSt3R / MASt3R run the split arithmetic (parity) or the single-product one (fp16)
        small = {"enc_dim": 512, "enc_depth": 2, "dec_dim": 256, "dec_depth": 4}
        du = Duster({"state_dict": dust3r_state_dict(0, small)}).eval().to(DEV)
        imgs = torch.rand(2, 3, 160, 224).to(DEV)
        for arith in ("fp32", "fp16"):
            du.conf["arithmetic"] = arith
            du.forward_pairs(imgs, [[0, 1]])
        ma = Mast3r({"state_dict": dust3r_state_dict(2, {**small, "desc_dim": 24})}).eval().to(DEV)
        ma.inference_output({"image0": torch.rand(1, 3, 128, 192).to(DEV), "image1": torch.rand(1, 3, 128, 192).to(DEV)})
    torch.cuda.synchronize()


def test_routes_of_every_network_are_covered():
    """Reset the per-handle route counters, run SuperPoint, LightGlue, DISK, SuperGlue, LoFTR, EfficientLoFTR (both arithmetic options),
    DUSt3R (split and single-product) and MASt3R once in each arithmetic mode they offer, and require every GEMM route they launched to be
    one the case table covers.  A new instantiation without a kernel-level case fails here."""
    be = _backend()
    seen = {}
    try:
        for mode in (1, 0):
            be.gemm_route_reset(DEV)
            _run_networks(mode)
            for r, n in be.gemm_route_counts(DEV).items():
                seen[r] = seen.get(r, 0) + n
    finally:
        be.set_precision(DEV, 1)
    cov = covered_routes()
    print("[gemm-gate] routes launched by the networks: " + ", ".join(f"{be.gemm_route_name(r)} x{n}" for r, n in sorted(seen.items())))
    print("[gemm-gate] routes covered by the case table: " + ", ".join(be.gemm_route_name(r) for r in sorted(cov)))
    assert seen, "no GEMM launch recorded"
    missing = sorted(set(seen) - cov)
    assert not missing, "routes without a kernel-level case: " + ", ".join(be.gemm_route_name(r) for r in missing)
