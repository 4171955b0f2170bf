"""Every launch of the fused FFN (csrc/ffn.hip, lg_ffn_kernel<VAR, ACT, MT>) that the networks make, entered directly through
imcui_hip_ffn_probe_f32 and compared with a plain float64 restatement of the same operator.

One case table (CASES), every case with the token tile forced (option ffn_tile; 0 for the cases that test the automatic rule) and the
instantiation asserted through the route ffn_launch recorded (imcui_hip_ffn_last_route).  Every case checks
  * the rows that must be valid against float64 within the FFN bar of tests/test_gpu_kernels.py, 3e-6 of max |reference| over those rows
    (the scaled epsilon cases: max(3e-6, 2 e_emu), see _expect);
  * memory the kernel must not write (NaN sentinels with a private payload: rows from M on, rows of a ragged sequence from
    roundup(cnt, tile) on, every row of an inactive pair) and its inputs x and ctx: bitwise unchanged;
  * the in-place call (out == x, the way all four networks call it) equals the out-of-place one bit for bit;
  * a plausible wrong operator for each constant and each fused step misses the bar by more than 4 x (the inputs can tell).
The references, the wrong references and the ragged rules are plain CPU code: tests/test_ffn_probe_cpu.py runs them without a device.
test_ffn_routes_of_every_network_are_covered runs every network and fails on a route the table does not cover."""
from __future__ import annotations

import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from test_gpu_gemm_variants import NAN_F32, _weights

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ERR_ARG, ERR_UNSUPPORTED = -1, -4
BAR = 3e-6  # tests/test_gpu_kernels.py: test_fused_ffn_*_vs_fp64
TILE_KIND = {128: "t128", 64: "t64", 32: "t32"}
# K order of W2's planes (ffn_permute_k): position 16 kk + 8 h + j holds original feature 16 kk + 8 (j >> 2) + 4 h + (j & 3)
PERM = torch.tensor([16 * (c >> 4) + 8 * ((c & 7) >> 2) + 4 * ((c >> 3) & 1) + (c & 3) for c in range(512)])


def _backend():
    from imcui_hip import backend

    return backend


def auto_tile(M):
    """The rule of ffn_launch: the largest tile that still gives each of the 256 CUs a workgroup."""
    return 128 if M > 256 * 64 else 64 if M > 256 * 32 else 32


# ------------------------------------------------------------------ weights and inputs (host)
_WSETS = {}


def wset(act, name="unit"):
    """One weight set per activation, shared by all its cases: W1 [512, 512], W2 [256, 512] with a row-dependent offset, b1, b2, gamma,
    beta (512 features for act 0 and -- ignored by the kernel -- act 1, 256 for act 2 / 3), and the packed planes.
    name "eps": W2 x 1e-2 (act 2 / 3: the variance before the LayerNorm(256) comes down to the order of its epsilon);
    name "range": b1 (act 1) / W1 (act 3) scaled so that the largest hidden activation is about 3e4."""
    if (act, name) in _WSETS:
        return _WSETS[(act, name)]
    be = _backend()
    g = torch.Generator().manual_seed(zlib.crc32(f"ffn_weights_act{act}".encode()))
    w = {"w1": _weights(g, 512, 512), "w2": _weights(g, 256, 512), "b1": torch.randn(512, generator=g) * (0.3 if act == 1 else 0.1),
         "b2": torch.randn(256, generator=g) * 0.1}  # fmt: skip
    nf = 256 if act >= 2 else 512
    w["gamma"], w["beta"] = 1.0 + 0.3 * torch.randn(nf, generator=g), 0.2 * torch.randn(nf, generator=g)
    if name == "eps" and act >= 2:
        w["w2"] = w["w2"] * 1e-2
    if name == "range" and act == 1:
        k = 2.9e4 / w["b1"].max().item()
        w["b1"], w["b2"] = w["b1"] * k, w["b2"] * k  # (b2 with it: the outputs grow as the hidden activations do)
    if name == "range" and act == 3:
        x, ctx = inputs("range_a3", 160)
        top = (torch.cat([x, ctx], 1).double() @ w["w1"].double().t()).abs().max().item()
        w["w1"] = w["w1"] * 2.0 ** math.floor(math.log2(3e4 / top))  # a power of two: the same planes, another s1
    w["p1"], w["p2"] = be.pack_linear_split(w["w1"]), be.pack_ffn_w2(w["w2"])
    _WSETS[(act, name)] = w
    return w


def inputs(key, M, scale=1.0):
    """x and ctx [M, 256], seeded by the data key; ctx at 0.6 of x's scale."""
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    return torch.randn(M, 256, generator=g) * scale, torch.randn(M, 256, generator=g) * (0.6 * scale)


def unpack_planes(planes, N, K, permuted=False):
    """What the kernel multiplies: (hi + lo) * 2^-e of the fragment-major planes [N / 32][K / 16][2][32][8] (split_weights_frag_host),
    back as a float64 [N, K] matrix in the original K order."""
    hi, lo, sc = planes
    v = hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64)
    v = torch.from_numpy(v.reshape(N // 32, K // 16, 2, 32, 8).transpose(0, 3, 1, 2, 4).reshape(N, K) * sc)
    if permuted:
        o = torch.empty_like(v)
        o[:, PERM] = v
        v = o
    return v


def split2_emu(v):
    """common.h split2: an f32 activation as the kernel multiplies it, hi = round-toward-zero f16 (saturating) plus lo = nearest f16 of
    the exact remainder; float64."""
    a = v.to(torch.float32).numpy()
    with np.errstate(over="ignore"):
        h = a.astype(np.float16)
    away =np.abs(h.astype(np.float32)) > np.abs(a)  # rounded away from zero (an overflow to inf included)
    h = np.where(away, np.nextafter(h, np.float16(0)), h)
    lo = (a - h.astype(np.float32)).astype(np.float16)
    return torch.from_numpy(h.astype(np.float64) + lo.astype(np.float64))


# ------------------------------------------------------------------ the operator in float64, and its wrong variants
def ffn_ref(x, ctx, w, act, form, w1=None, w2=None, operand=None, gelu="none", eps=1e-5, slope=None, drop_b1=False, drop_b2=False, ln_half=False,
            ln_after_resid=False, b2_after_ln=False, resid_ctx=False, swap_slabs=False, w2_permuted=False):  # fmt: skip
    """ffn.h: act 0 x + W2 GELU(LN_512(W1 [x | ctx] + b1)) + b2; act 1 x + W2 ReLU(W1 [x | ctx] + b1) + b2; act 2 / 3
    x + LN_256(W2 act(W1 [x | ctx] + b1) + b2) with LeakyReLU(0.01) / ReLU.  form "net": the arrays the owning network passes (act 2 / 3
    without biases), "full": every array.  `operand` rounds the two matrix operands (the [x | ctx] slab and the hidden activations), w1 /
    w2 replace the weights: the emulation of _expect.  Every other keyword switches one WRONG operator on."""
    x, ctx = x.double(), ctx.double()
    W1 = w["w1"].double() if w1 is None else w1
    W2 = w["w2"].double() if w2 is None else w2
    biased = not (form == "net" and act >= 2)
    b1 = w["b1"].double() if biased and not drop_b1 else 0.0
    b2 = w["b2"].double() if biased and not drop_b2 else 0.0
    gamma, beta = w["gamma"].double(), w["beta"].double()
    a = torch.cat([ctx, x], 1) if swap_slabs else torch.cat([x, ctx], 1)
    if operand is not None:
        a = operand(a)
    h = a @ W1.t() + b1
    if act == 0:
        if ln_half:
            mu, var = h[:, :256].mean(1, keepdim=True), h[:, :256].var(1, unbiased=False, keepdim=True)
            h = (h - mu) / torch.sqrt(var + eps) * gamma + beta
        else:
            h = F.layer_norm(h, (512,), gamma, beta, eps)
        h = F.gelu(h, approximate=gelu)
    else:
        s = slope if slope is not None else (0.01 if act == 2 else 0.0)
        h = torch.where(h > 0, h, s * h)
    if operand is not None:
        h = operand(h)
    y = h @ (W2[:, PERM] if w2_permuted else W2).t()
    r = ctx if resid_ctx else x
    if act < 2:
        return r + y + b2
    if ln_after_resid:
        return F.layer_norm(r + y + b2, (256,), gamma, beta, eps)
    if b2_after_ln:
        return r + F.layer_norm(y, (256,), gamma, beta, eps) + b2
    return r + F.layer_norm(y + b2, (256,), gamma, beta, eps)


def ffn_emu(x, ctx, w, act, form):
    """float64 on the operands as common.h rounds them: x, ctx and the hidden activations as split2's hi + lo pair, the weights as the
    packed planes times their scale.  What it leaves out is the f32 accumulation."""
    return ffn_ref(x, ctx, w, act, form, w1=unpack_planes(w["p1"], 512, 512), w2=unpack_planes(w["p2"], 256, 512, permuted=True), operand=split2_emu)


WRONG = {
    "tanh GELU": dict(gelu="tanh"), "LN eps 1e-6": dict(eps=1e-6), "LN eps 0": dict(eps=0.0), "b1 dropped": dict(drop_b1=True),
    "LN over 256 features": dict(ln_half=True), "LeakyReLU(0.01) for ReLU": dict(slope=0.01), "b2 dropped": dict(drop_b2=True),
    "ReLU for LeakyReLU": dict(slope=0.0), "slope 0.1": dict(slope=0.1), "LN after the residual": dict(ln_after_resid=True),
    "b2 after the LN": dict(b2_after_ln=True), "residual from ctx": dict(resid_ctx=True), "[ctx | x] slabs": dict(swap_slabs=True),
    "W2 K permutation kept": dict(w2_permuted=True),
}  # fmt: skip
_WRONG_ALL = ["residual from ctx", "[ctx | x] slabs", "W2 K permutation kept"]


def wrong_names(act, form, eps_case=False):
    """The wrong operators a case of this activation and form must tell from the right one.  The wrong epsilons are asserted only
    where the inputs are scaled for them (the eps cases): at unit scale the 1e-5 need not move the result by more than the bar."""
    n = {0: ["tanh GELU", "b1 dropped", "LN over 256 features"], 1: ["LeakyReLU(0.01) for ReLU", "b2 dropped"],
         2: ["ReLU for LeakyReLU", "slope 0.1", "LN after the residual"], 3: ["LN after the residual"]}[act] + _WRONG_ALL  # fmt: skip
    if act >= 2 and form == "full":
        n.append("b2 after the LN")
    if eps_case:
        n += ["LN eps 1e-6"] + (["LN eps 0"] if act == 0 else [])
    return n


def ragged_masks(cnt, active, tile, R, rule="right"):
    """(valid, untouched) row masks of a ragged launch: sequence s = row // R, pair = s >> 1; rows below cnt[s] of an active pair are
    valid, rows from roundup(cnt[s], tile) on and every row of an inactive pair are untouched, the rows in between unspecified.
    rule: the WRONG readings "cnt by pair" (cnt[s >> 1]) and "active by sequence" (active[s], the last entry for s past the array)."""
    S = len(cnt)
    valid, untouched = torch.zeros(S * R, dtype=torch.bool), torch.ones(S * R, dtype=torch.bool)
    for s in range(S):
        n = cnt[s >> 1] if rule == "cnt by pair" else cnt[s]
        on = True if active is None else bool(active[min(s, len(active) - 1)] if rule == "active by sequence" else active[s >> 1])
        if on:
            valid[s * R : s * R + n] = True
            untouched[s * R : s * R + min(R, -(-n // tile) * tile)] = False
    return valid, untouched


RAGGED_WRONG_RULES = ("cnt by pair", "active by sequence")


def excluded_rules(cnt, active, tile, R):
    """The wrong ragged rules this case can tell from the right one: they call a valid row untouched or an untouched row valid."""
    v, u = ragged_masks(cnt, active, tile, R)
    out = []
    for rule in RAGGED_WRONG_RULES:
        vw, uw = ragged_masks(cnt, active, tile, R, rule)
        if ((v & uw) | (u & vw)).any():
            out.append(rule)
    return out


# ------------------------------------------------------------------ what a case expects (CPU)
_EXPECT = {}


def case_rows(c):
    """The rows compared with float64: all of them, or (automatic-tile cases) a strided sample plus the last 128."""
    M = c["M"]
    return torch.arange(M) if not c.get("sample") else torch.cat([torch.arange(0, M - 128, 61), torch.arange(M - 128, M)])


def _expect(c):
    """x, ctx, the float64 reference on case_rows, the wrong references and the bar of a case; shared by the cases of one data key (the
    tiles, in place / out of place, the `active` masks).  The bar is BAR, except in the scaled epsilon cases: there the f16 planes' own
    resolution may exceed it (lo parts of 1e-2-sized values are f16 subnormals), so e_emu = |float64 - ffn_emu| / max |float64| is
    computed here and the bar is max(BAR, 2 e_emu): the factor 2 leaves room for the f32 accumulation that ffn_emu leaves out."""
    key = c["data"]
    if key not in _EXPECT:
        _EXPECT.clear()
        w = wset(c["act"], c.get("wset", "unit"))
        x, ctx = inputs(key, c["M"], c.get("xscale", 1.0))
        rows = case_rows(c)
        xr, cr = x[rows], ctx[rows]
        ref = ffn_ref(xr, cr, w, c["act"], c["form"])
        wrong = {n: ffn_ref(xr, cr, w, c["act"], c["form"], **WRONG[n]) for n in wrong_names(c["act"], c["form"], c["kind"] == "eps")}
        e_emu = None
        if c["kind"] == "eps" or c.get("emu"):
            e_emu = ((ffn_emu(xr, cr, w, c["act"], c["form"]) - ref).abs().max() / ref.abs().max()).item()
        bar = max(BAR, 2 * e_emu) if c["kind"] == "eps" else BAR
        _EXPECT[key] = dict(x=x, ctx=ctx, rows=rows, ref=ref, wrong=wrong, bar=bar, e_emu=e_emu, w=w)
    return _EXPECT[key]


def _rel(out, ref):
    return (out.double() - ref).abs().max().item() / ref.abs().max().item()


def wrong_distances(e, rows=None):
    """Distance of every wrong reference from the right one, relative to max |right| over `rows` (default: all the case compares)."""
    ref = e["ref"] if rows is None else e["ref"][rows]
    return {n: _rel(r if rows is None else r[rows], ref) for n, r in e["wrong"].items()}


# ------------------------------------------------------------------ device side
_DEVSETS = {}


def _devset(act, name):
    if (act, name) not in _DEVSETS:
        be, w = _backend(), wset(act, name)
        d = {"W": be.FfnWeights(w["w1"], w["w2"], DEV)}
        d.update({k: w[k].to(DEV) for k in ("b1", "b2", "gamma", "beta")})
        _DEVSETS[(act, name)] = d
    return _DEVSETS[(act, name)]


def _fields(c):
    """Descriptor fields of the case's weights, in the nullable form the owning network uses ("net": SuperGlue without gamma / beta,
    the dense matchers without biases) or with every array present ("full")."""
    d = _devset(c["act"], c.get("wset", "unit"))
    f = dict(d["W"].fields(), b1=d["b1"], b2=d["b2"], gamma=d["gamma"], beta=d["beta"], act=c["act"])
    if c["form"] == "net" and c["act"] == 1:
        f.update(gamma=None, beta=None)
    if c["form"] == "net" and c["act"] >= 2:
        f.update(b1=None, b2=None)
    return f


def _sentinel(rows):
    return torch.full((rows, 256), NAN_F32, dtype=torch.int32, device=DEV).view(torch.float32)


def _bits(t):
    return t.view(torch.int32)


def _probe(c, tile, **f):
    """Launch with the tile forced (0: the automatic rule); asserts the recorded route.  Returns it."""
    be = _backend()
    with be.option(DEV, ffn_tile=tile):
        r = be.ffn_probe(DEV, **f)
    torch.cuda.synchronize()
    want = be.ffn_route(TILE_KIND[tile or auto_tile(f["M"])], c["act"])
    assert r == want, f"route {be.ffn_route_name(r)}, expected {be.ffn_route_name(want)}"
    return r


def _discriminates(got, e, bar, rows=None):
    ref = e["ref"] if rows is None else e["ref"][rows]
    errs = {n: _rel(got, r if rows is None else r[rows]) for n, r in e["wrong"].items()}
    for n, v in errs.items():
        assert v > 4 * bar, f"the wrong reference '{n}' passes ({v:.2e}): the case cannot tell"
    return errs


def _report(c, route, err, bar, wrong=None, extra=""):
    be = _backend()
    w = "" if not wrong else "  wrong refs: " + ", ".join(f"{k} {v:.1e}" for k, v in wrong.items())
    print(f"[ffn] {c['id']} {be.ffn_route_name(route) if route else 'refused'}: err {err:.2e} bar {bar:.1e}{extra}{w}")


def run_dense(c):
    """Out of place into M + 128 sentinel rows, then in place (out == x, M + 128 rows behind x): rows 0 .. M-1 meet the bar and are
    bitwise equal in both, rows from M on and the inputs are untouched."""
    e = _expect(c)
    M, tile, rows = c["M"], c["tile"], e["rows"]
    xd, cd = e["x"].to(DEV), e["ctx"].to(DEV)
    x0, c0 = xd.clone(), cd.clone()
    out = _sentinel(M + 128)
    f = _fields(c)
    route = _probe(c, tile, x=xd, ctx=cd, out=out, M=M, **f)
    assert torch.equal(_bits(xd), _bits(x0)) and torch.equal(_bits(cd), _bits(c0)), "an input was written"
    assert (_bits(out[M:]) == NAN_F32).all(), "rows from M on were written"
    got = out[:M].cpu()
    assert torch.isfinite(got).all()
    err = _rel(got[rows], e["ref"])
    wrong = _discriminates(got[rows], e, e["bar"])
    extra = "" if e["e_emu"] is None else f" e_emu {e['e_emu']:.2e}"
    _report(c, route, err, e["bar"], wrong, extra)
    assert err < e["bar"], (err, e["bar"])
    buf = _sentinel(M + 128)
    buf[:M] = x0
    _probe(c, tile, x=buf, ctx=cd, out=buf, M=M, **f)
    assert torch.equal(_bits(buf[:M]), _bits(out[:M])), "in place differs from out of place"
    assert (_bits(buf[M:]) == NAN_F32).all(), "in place: rows from M on were written"
    assert torch.equal(_bits(cd), _bits(c0))


def run_ragged(c):
    """S sequences of R rows with device-side counts and pair mask, run twice: with the padding rows of x and ctx holding NaN (a valid
    row that read one would show it) and holding zeros (in place, a stray `x + y` onto a NaN row would keep the NaN's bits and pass for
    untouched; onto a zero row it shows).  The valid rows of both runs are bitwise equal.  Out-of-place cases also run every live sequence
    alone (M = cnt[s], same tile): bitwise equal again."""
    e = _expect(c)
    R, cnt, active, tile, inplace = c["R"], c["cnt"], c["active"], c["tile"], c["inplace"]
    S = len(cnt)
    M = S * R
    valid, untouched = ragged_masks(cnt, active, tile, R)
    pad = torch.ones(M, dtype=torch.bool)
    for s in range(S):
        pad[s * R : s * R + cnt[s]] = False
    cntd = torch.tensor(cnt, dtype=torch.int32, device=DEV)
    actd = None if active is None else torch.tensor(active, dtype=torch.int32, device=DEV)
    f = dict(_fields(c), M=M, cnt=cntd, active=actd, rows_per_seq=R)
    results = []
    for fill in ("nan", "zero"):
        xd, cd = e["x"].to(DEV), e["ctx"].to(DEV)
        for t in (xd, cd):
            _bits(t)[pad.to(DEV)] = NAN_F32 if fill == "nan" else 0
        x0, c0 = xd.clone(), cd.clone()
        if inplace:
            out = _sentinel(M + 128)
            out[:M] = xd
            before = out.clone()
            route = _probe(c, tile, x=out, ctx=cd, out=out, **f)
        else:
            out = _sentinel(M + 128)
            before = out.clone()
            route = _probe(c, tile, x=xd, ctx=cd, out=out, **f)
            assert torch.equal(_bits(xd), _bits(x0)), "x was written"
        assert torch.equal(_bits(cd), _bits(c0)), "ctx was written"
        keep = torch.cat([untouched, torch.ones(128, dtype=torch.bool)]).to(DEV)
        assert torch.equal(_bits(out)[keep], _bits(before)[keep]), "a row past roundup(cnt, tile), of an inactive pair or past M was written"
        results.append(out[:M].cpu()[valid])
    got = results[0]
    err, wrong = 0.0, {}
    if valid.any():
        assert torch.isfinite(got).all(), "a valid row is not finite: it read a padding row"
        err = _rel(got, e["ref"][valid])
        wrong = _discriminates(got, e, e["bar"], valid)
    rules = excluded_rules(cnt, active, tile, R)
    _report(c, route, err, e["bar"], wrong, f" valid rows {int(valid.sum())}, wrong rules excluded: {rules or 'none'}")
    assert err < e["bar"], (err, e["bar"])
    assert torch.equal(_bits(results[1]), _bits(got)), "valid rows depend on the padding rows"
    if inplace:
        return
    for s in range(S):
        if cnt[s] == 0 or not valid[s * R]:
            continue
        n = cnt[s]
        xs, cs = e["x"][s * R : s * R + n].to(DEV), e["ctx"][s * R : s * R + n].to(DEV)
        alone = _sentinel(n + 128)
        _probe(c, tile, x=xs, ctx=cs, out=alone, M=n, **_fields(c))
        assert torch.equal(_bits(alone[:n]).cpu(), _bits(got[int(valid[: s * R].sum()) :][:n])), f"sequence {s} alone differs from the ragged launch"


def run_refusal(c):
    """A refused call returns its code, leaves last-route at 0 and writes nothing; M = 0 returns OK and does the same."""
    be = _backend()
    w = dict(id=c["id"], act=c.get("wact", 0), form="full", wset="unit")
    xd, cd = (t.to(DEV) for t in inputs(c["id"], 128))
    x0 = xd.clone()
    out = _sentinel(256)
    f = dict(_fields(w), x=xd, ctx=cd, out=out, M=128)
    f.update(c["fields"])
    be.ffn_route_reset(DEV)
    try:
        be.set_precision(DEV, c.get("precision", 1))
        rc = be.ffn_probe(DEV, check=False, **f)
    finally:
        be.set_precision(DEV, 1)
    torch.cuda.synchronize()
    hd = be.get_handle(DEV)
    assert rc == c["expect"], f"expected {c['expect']}, got {rc}"
    assert hd.lib.imcui_hip_ffn_last_route(hd.h) == 0 and not be.ffn_route_counts(DEV)
    assert (_bits(out) == NAN_F32).all() and torch.equal(_bits(xd), _bits(x0)), "a refused call wrote"
    print(f"[ffn] {c['id']}: status {rc}, route none")


# ------------------------------------------------------------------ the case table
FORMS = {0: ("net",), 1: ("net", "full"), 2: ("net", "full"), 3: ("net", "full")}  # act 0 (LightGlue) passes every array: one form
DENSE_M = (1, 31, 32, 33, 64, 65, 127, 128, 129, 160)
TILES = (128, 64, 32)
RAGGED_CNT = {"a": [256, 129, 1, 0], "b": [128, 128, 97, 33]}
RAGGED_ACTIVE = {"none": None, "11": [1, 1], "10": [1, 0], "01": [0, 1]}

CASES = []
# dense: every M x every forced tile x every activation, in the network's nullable form and with every array present
for _a in range(4):
    for _f in FORMS[_a]:
        for _M in DENSE_M:
            for _t in TILES:
                CASES.append(dict(id=f"dense_a{_a}_{_f}_M{_M}_t{_t}", kind="dense", run=run_dense, act=_a, form=_f, M=_M, tile=_t,
                                  data=f"dense_a{_a}_{_f}_M{_M}", emu=_M == 160))  # fmt: skip
# the automatic tile rule at its two thresholds (256 CUs x 32 / 64 tokens): tile 32, 64, 64, 128
for _a in range(4):
    for _M in (8192, 8193, 16384, 16385):
        CASES.append(dict(id=f"auto_a{_a}_M{_M}", kind="auto", run=run_dense, act=_a, form="net", M=_M, tile=0, sample=True, data=f"auto_a{_a}_M{_M}"))
# ragged: 4 sequences of 256 rows, two pairs; the counts and masks the launch sites pass
for _a in (0, 1):
    for _cn, _cnt in RAGGED_CNT.items():
        for _an, _act in RAGGED_ACTIVE.items():
            for _t in TILES:
                for _ip in (False, True):
                    CASES.append(dict(id=f"ragged_a{_a}_cnt{_cn}_act{_an}_t{_t}_{'inplace' if _ip else 'outofplace'}", kind="ragged", run=run_ragged,
                                      act=_a, form="net", M=1024, R=256, cnt=_cnt, active=_act, tile=_t, inplace=_ip, data=f"ragged_a{_a}_cnt{_cn}"))  # fmt: skip
# the smallest legal sequence
for _a in (0, 1):
    for _t in TILES:
        CASES.append(dict(id=f"ragged_min_a{_a}_t{_t}", kind="ragged", run=run_ragged, act=_a, form="net", M=256, R=128, cnt=[128, 5], active=None,
                          tile=_t, inplace=False, data=f"ragged_min_a{_a}"))  # fmt: skip
# LayerNorm epsilon: inputs scaled so that the variance before the normalisation comes down towards the epsilon.  Bar max(3e-6, 2 e_emu);
# e_emu computed on the CPU (tests/test_ffn_probe_cpu.py prints it).  Measured:
#   eps_a0 (x, ctx x 1e-2): e_emu 1.51e-07      eps_a2 (W2 x 1e-2): e_emu 1.69e-07      eps_a3 (W2 x 1e-2): e_emu 1.52e-07
# so 2 e_emu < 3e-6 and the bar of all three stays 3.0e-06; the wrong epsilons are 6.7e-04 / 7.4e-04 (act 0: 1e-6 / 0), 2.7e-04 (act 2)
# and 2.1e-04 (act 3) away, far beyond 4 x bar, so the scale needs no lowering.
for _a, _kw in ((0, dict(xscale=1e-2)), (2, dict(wset="eps")), (3, dict(wset="eps"))):
    for _t in TILES:
        CASES.append(dict(id=f"eps_a{_a}_t{_t}", kind="eps", run=run_dense, act=_a, form=FORMS[_a][-1], M=160, tile=_t, data=f"eps_a{_a}", **_kw))
# hidden activations up to about 3e4: inside the f16 range, far from unit scale (nothing is asserted above 65504, see ffn.h)
for _a in (1, 3):
    for _t in TILES:
        CASES.append(dict(id=f"range_a{_a}_t{_t}", kind="range", run=run_dense, act=_a, form="net", M=160, tile=_t, data=f"range_a{_a}", wset="range", emu=True))


def _refusal(id_, expect, **kw):
    return dict(id=id_, kind="refusal", run=run_refusal, expect=expect, fields=kw.pop("fields", {}), **kw)


CASES += [
    _refusal("refuse_precision0", ERR_UNSUPPORTED, precision=0),
    _refusal("refuse_act4", ERR_ARG, fields=dict(act=4)),
    _refusal("refuse_act_minus1", ERR_ARG, fields=dict(act=-1)),
    _refusal("refuse_rows_per_seq_96", ERR_ARG, fields=dict(rows_per_seq=96)),
    _refusal("empty_M0", 0, fields=dict(M=0)),
]
CASES += [_refusal(f"refuse_a{_a}_null_{_n}", ERR_ARG, wact=_a, fields={_n: None}) for _a in (0, 2, 3) for _n in ("gamma", "beta")]
CASES += [_refusal(f"refuse_null_{_n}", ERR_ARG, fields={_n: None}) for _n in ("x", "ctx", "out", "w1h", "w1l", "w2h", "w2l", "s1", "s2")]


def case_route(c):
    """(kind, act) of the instantiation a case launches; None for a refusal."""
    return None if c["kind"] == "refusal" else (TILE_KIND[c["tile"] or auto_tile(c["M"])], c["act"])


def covered_routes() -> set:
    be = _backend()
    return {be.ffn_route(*case_route(c)) for c in CASES if case_route(c)}


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_ffn_variant(case):
    _backend().set_precision(DEV, 1)
    case["run"](case)


# ------------------------------------------------------------------ the gate: every route a network launches has a case above
def _run_lightglue():
    from imcui_hip.pipeline import SuperPointLightGluePipeline
    from imcui_hip.synth import make_pair_batch
    from imcui_hip.synth_weights import lightglue_state_dict, superpoint_state_dict

    img0, img1, _ = make_pair_batch(1, 1, 120, 160, n_blobs=150)
    pipe = SuperPointLightGluePipeline({"nms_radius": 3, "max_keypoints": 256, "keypoint_threshold": 0.005, "remove_borders": 4, "state_dict": superpoint_state_dict(0)},
                                       {"depth_confidence": 0.95, "width_confidence": 0.99, "match_threshold": 0.1, "state_dict": lightglue_state_dict(0)})  # fmt: skip
    pipe.eval().to(DEV)(img0.to(DEV), img1.to(DEV))
    torch.cuda.synchronize()


def test_ffn_routes_of_every_network_are_covered():
    """The fused-FFN routes of every network of the tree in the split arithmetic (the sweep of the GEMM gate,
    test_gpu_gemm_variants.network_sweep: one cached pass that reads all four route recorders per network; LightGlue act 0, SuperGlue
    act 1, EfficientLoFTR act 2, LoFTR act 3; no launch in the exact mode, which the gate also asserts), and LightGlue again with the 128- and 64-token tiles forced, and require every fused-FFN route
    they launched to be one the case table covers.  A new instantiation or a changed tile rule without a kernel-level case fails here.
    (The rolled 128-token variant is reachable only through the IMCUI_FFN_VARIANT=0 environment switch and has no case: were anything to
    launch it, this gate would say so.)"""
    from test_gpu_gemm_variants import network_sweep

    be = _backend()
    seen = {}
    try:
        for (mode, name), rec in network_sweep().items():
            if rec["ffn"]:
                print(f"[ffn-gate] mode {mode} {name}: " + ", ".join(f"{be.ffn_route_name(r)} x{n}" for r, n in sorted(rec["ffn"].items())))
            assert mode == 1 or not rec["ffn"], f"{name}: a fused-FFN launch in the exact mode"
            for r, n in rec["ffn"].items():
                seen[r] = seen.get(r, 0) + n
        be.ffn_route_reset(DEV)
        be.set_precision(DEV, 1)
        for tile in (128, 64):
            with be.option(DEV, ffn_tile=tile):
                _run_lightglue()
        for r, n in be.ffn_route_counts(DEV).items():
            seen[r] = seen.get(r, 0) + n
    finally:
        be.set_precision(DEV, 1)
    cov = covered_routes()
    print("[ffn-gate] routes launched by the networks: " + ", ".join(f"{be.ffn_route_name(r)} x{n}" for r, n in sorted(seen.items())))
    print("[ffn-gate] routes covered by the case table: " + ", ".join(be.ffn_route_name(r) for r in sorted(cov)))
    assert seen, "no fused-FFN launch recorded"
    acts = {(r - 1) % 4 for r in seen}
    assert acts == {0, 1, 2, 3}, f"activations seen: {sorted(acts)}"
    missing = sorted(set(seen) - cov)
    assert not missing, "routes without a kernel-level case: " + ", ".join(be.ffn_route_name(r) for r in missing)
