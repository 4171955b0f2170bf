"""Every launch of the patch-staging 3x3 convolutions (csrc/conv.hip) that the networks make, entered directly through
imcui_hip_conv_probe_f32 and compared with torch.nn.functional.conv2d in float64 followed by the documented epilogue in float64.

One case table (CASES).  Every case names the kernel instantiation it expects -- or the refusal code -- and asserts it through the
route the launch site recorded (imcui_hip_conv_last_route) together with the feature mask (imcui_hip_conv_route_features).  Every
case then checks:
  * the result against float64, relative to max |reference|: 2e-6 for the exact f32 kernels (conv3x3_kernel, conv1a_kernel), 4e-6 for
    the split kernels, 4e-6 for the single-product kernels against float64 on operands rounded as conv.h documents (nearest-even f16
    of w * 2^e; saturating nearest-even f16 of the activation, taken after the input ReLU);
  * every output buffer (out, pts, conf, raw) sits between two guard bands of GUARD floats holding a NaN payload, inside the same
    allocation: the bands are bitwise unchanged and no element between them still holds the payload;
  * with cin_stride > Cin the unused channels of every input pixel are NaN and must not reach the output;
  * a plausible wrong reference for each fused feature misses the bar by the margin of _discriminates: activation before the
    residual, resid2 dropped, input ReLU dropped, ReLU for LeakyReLU, dy / dx swapped, channel c + 32 in place of c (and, for the
    head, the second 64-channel half multiplied with the first half's head weights).
The point-map head is compared in two steps: `raw` with the float64 1x1 convolution of the float64 feature map (4e-6), and pts / conf
with xyz / max(|xyz|, 1e-8) * expm1(|xyz|) and 1 + exp(c) evaluated in float64 on the DEVICE's raw, per pixel relative to |pts| and to
conf (HEAD_BAR_PTS, HEAD_BAR_CONF), which separates the transcendental error from the convolution's.
test_conv_routes_of_every_network_are_covered reads the one sweep over every network of the tree (test_gpu_gemm_variants.network_sweep;
NETWORKS below names those that launch conv.hip: SuperPoint, LoFTR, EfficientLoFTR, DUSt3R, MASt3R, D2-Net, DeDoDe, NetVLAD) and fails on a
(route, feature) pair the table does not cover.

Errors measured on MI355X against float64 (max over the cases of the variant) and the bar each is held to:
  variant                        cases  measured   bar
  f32 (conv3x3_kernel)               4   1.3e-06   2e-6
  conv1a (conv1a_kernel)             1   1.2e-07   2e-6
  split_n2                          19   1.2e-06   4e-6   (the maximum at Cin 224 of 256 stored)
  split_n4                          17   9.4e-07   4e-6
  split_n2_single                    3   5.6e-07   4e-6   (against float64 on the rounded operands)
  split_n4_single                    3   4.1e-07   4e-6
  tall / tall_single               4 / 4 1.2e-06 / 6.1e-07  4e-6
  fused_tall / fused_8row          2 / 2 5.5e-07 / 6.9e-07  4e-6
  head, 128-channel map / raw        6   7.0e-07 / 4.2e-07  4e-6  (split and single-product layers)
  head, pts | device raw             6   1.44e-07  5.7e-7  = 4 x measured (1.2 ulp of f32; |xyz| 0.001 .. 5.3)
  head, conf | device raw            6   9.26e-08  3.7e-7  = 4 x measured (0.8 ulp)
The head's own error is one to two f32 ulp, as expected of sqrtf, expm1f, a division and a product; with |xyz| up to 15 it measured
7.0e-07, the |xyz| 2^-24 that the rounding of |xyz| contributes to expm1.
"""
from __future__ import annotations

import math
import zlib

import pytest
import torch
import torch.nn.functional as F
from test_gpu_gemm_variants import DEV, NAN_F32, _discriminates, _round_act, _round_single, _sentinel, _untouched

pytestmark = pytest.mark.gpu

ERR_ARG = -1
GUARD = 4096  # floats on either side of every output buffer
HEAD_BAR_PTS, HEAD_BAR_CONF = 5.7e-7, 3.7e-7  # against the float64 formula on the device's raw: 4 x the measured maxima (module docstring)
FEATURES = {"pool": 1, "resid": 2, "resid2": 4, "leaky": 8, "relu_in": 16, "cin_stride": 32, "cout_live": 64, "head": 128, "head_no_out": 256,
            "head_raw": 512}  # fmt: skip
TAPS = torch.arange(9.0).reshape(3, 3)  # a ramp over the taps: a swapped dy / dx cannot pass


def _backend():
    from imcui_hip import backend

    return backend


def _bar(route):
    return 2e-6 if route in ("f32", "conv1a") else 4e-6


def _rel(out, ref):
    return (out.double() - ref).abs().max().item() / ref.abs().max().item()


def _guarded(n):
    """(allocation, view of n floats between two guard bands)"""
    buf = _sentinel(2 * GUARD + n)
    return buf, buf[GUARD : GUARD + n]


def _check_guards(buf, written):
    """The guard bands are bitwise unchanged; the span between them was written completely (or, refused / absent, not at all)."""
    n = buf.numel() - 2 * GUARD
    mask = torch.zeros(buf.numel(), dtype=torch.bool)
    mask[GUARD : GUARD + n] = written
    _untouched(buf, mask)
    if written:
        left = (buf[GUARD : GUARD + n].view(torch.int32) == NAN_F32).sum().item()
        assert left == 0, f"{left} output elements were never written"


def _weights(g, cout, cin):
    """Random OIHW weights with an offset per output channel and a ramp over the taps."""
    s = 1.0 / math.sqrt(9 * cin)
    return torch.randn(cout, cin, 3, 3, generator=g) * s + torch.arange(cout).float()[:, None, None, None] * (0.01 * s) + TAPS * (0.05 * s)


def _act(y, code):
    return torch.relu(y) if code == 1 else F.leaky_relu(y, 0.01) if code == 2 else y


def case_options(c) -> dict:
    """Handle options of a case: its own, else the ones that reach the route it names."""
    if "opts" in c:
        return c["opts"]
    r = c.get("route") or ""
    if r.startswith("split_n4"):
        return {"conv_narrow": 2, "conv_tall": 1}
    if r.startswith("split_n2"):
        return {"conv_narrow": 1, "conv_tall": 1}
    if r.startswith("tall"):
        return {"conv_narrow": 1, "conv_tall": 2}
    if r == "fused_8row":
        return {"conv_tall": 0}
    return {"conv_tall": 1}


def case_features(c) -> int:
    """ConvFeature mask the launch of a case records (csrc/conv.h)."""
    f = 0
    if c.get("pool"):
        f |= FEATURES["pool"]
    if c["entry"] != "split":
        return f
    f |= FEATURES["resid"] if c.get("resid") else 0
    f |= FEATURES["resid2"] if c.get("resid2") else 0
    f |= FEATURES["leaky"] if c.get("act", 0) == 2 else 0
    f |= FEATURES["relu_in"] if c.get("relu_in") else 0
    f |= FEATURES["cin_stride"] if c.get("cin_stride", 0) not in (0, c["cin"]) else 0
    f |= FEATURES["cout_live"] if 0 < c.get("cout_live", 0) < c["cout"] else 0
    if c.get("head"):
        f |= FEATURES["head"] | (0 if c.get("head_out", True) else FEATURES["head_no_out"]) | (FEATURES["head_raw"] if c.get("head_raw", True) else 0)
    return f


def _probe(c, **fields):
    """Launch under the case's options; asserts the route (and feature mask) or the refusal.  Returns the route name or None."""
    be = _backend()
    hd = be.get_handle(DEV)
    be.conv_route_reset(DEV)
    with be.option(DEV, **case_options(c)):
        if c.get("refusal"):
            rc = be.conv_probe(DEV, check=False, **fields)
            torch.cuda.synchronize()
            assert rc == c["refusal"], f"expected refusal {c['refusal']}, got {rc}"
            assert hd.lib.imcui_hip_conv_last_route(hd.h) == 0
            assert be.conv_route_counts(DEV) == {}
            return None
        r = be.conv_probe(DEV, **fields)
    torch.cuda.synchronize()
    assert r == be.conv_route(c["route"]), f"route {be.conv_route_name(r)}, expected {c['route']}"
    assert be.conv_route_counts(DEV) == {r: 1}
    assert be.conv_route_features(DEV).get(r, 0) == case_features(c), (be.conv_feature_names(be.conv_route_features(DEV).get(r, 0)), case_features(c))
    return c["route"]


def _report(c, route, err, wrong=None, extra=""):
    w = "" if not wrong else "  wrong refs: " + ", ".join(f"{k} {v:.1e}" for k, v in wrong.items())
    print(f"[conv] {c['id']} {route or 'refused'}: err {err:.2e}{extra}{w}")


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.get("seed", c["id"]).encode()))


def _ceil_to(n, m):
    return -(-n // m) * m


# ------------------------------------------------------------------ conv3x3_launch / conv3x3_split_launch without a head
def run_conv(c):
    be = _backend()
    B, H, W, cin, cout = c["B"], c["H"], c["W"], c["cin"], c["cout"]
    split = c["entry"] == "split"
    act, relu_in, pool, single = c.get("act", 0), c.get("relu_in", False), c.get("pool", False), c.get("single", False)
    live = c.get("cout_live", 0) or cout
    cs = c.get("cin_stride", 0)
    refused = bool(c.get("refusal"))
    g = _gen(c)
    x = torch.randn(B, cin, H, W, generator=g)
    # a refused shape cannot be packed: its (never read) weights have the next valid shape
    wcin, wlive, wcout = (_ceil_to(cin, 32), min(live, _ceil_to(cout, 64)), _ceil_to(cout, 64)) if refused else (cin, live, cout)
    w = _weights(g, wlive, wcin)
    b = torch.randn(wlive, generator=g) * 0.1
    wt = be.ConvWeights(w, b, DEV, cout_pad=wcout)
    ho, wo = (H // 2, W // 2) if pool else (H, W)
    r1 = torch.randn(B, cout, H, W, generator=g) if c.get("resid") else None
    r2 = torch.randn(B, cout, H, W, generator=g) if c.get("resid2") else None
    xd = x.permute(0, 2, 3, 1).contiguous()
    if cs > cin:  # the map stores more channels than the layer uses: poison the rest
        full = torch.full((B, H, W, cs), float("nan"))
        full[..., :cin] = xd
        xd = full
    buf, out = _guarded(B * ho * wo * cout)
    nhwc = lambda t: None if t is None else t.permute(0, 2, 3, 1).contiguous().to(DEV)  # noqa: E731
    f = dict(entry=c["entry"], inp=xd.to(DEV), out=None if c.get("null_out") else out, B=B, H=H, W=W, Cin=cin, Cout=cout, pool=int(pool), **wt.fields(split))
    if split:
        f.update(relu=act | (4 if relu_in else 0), resid=nhwc(r1), resid2=nhwc(r2), cin_stride=cs, cout_live=c.get("cout_live", 0), single=int(single))
    else:
        f.update(relu=act)
    route = _probe(c, **f)
    _check_guards(buf, route is not None)
    if route is None:
        return _report(c, None, 0.0)
    got = out.view(B, ho, wo, cout).cpu()
    assert torch.isfinite(got).all()
    if live < cout:
        assert (got[..., live:] == 0).all(), "the padded output channels must be stored as exact zeros"
    ws_true = w.double() if not single else _round_single(w, wt.scale)

    def ref_of(swap=False, act_first=False, drop_r2=False, drop_relu_in=False, code=act):
        xi = x.double()
        if relu_in and not drop_relu_in:
            xi = torch.relu(xi)
        if single:
            xi = _round_act(xi)
        y = F.conv2d(xi, ws_true.transpose(-1, -2) if swap else ws_true, b.double(), padding=1)
        if r1 is not None:
            rsum = r1.double()[:, :live] + (0 if r2 is None or drop_r2 else r2.double()[:, :live])
            y = _act(y, code) + rsum if act_first else _act(y + rsum, code)
        else:
            y = _act(y, code)
        if pool:
            y = F.max_pool2d(y, 2, 2)
        return y.permute(0, 2, 3, 1)

    ref = ref_of()
    gl = got[..., :live]
    err = _rel(gl, ref)
    wrong = {"dy / dx swapped": ref_of(swap=True)}
    if live > 32:
        wrong["channel c + 32"] = ref.roll(-32, -1)
    if r1 is not None and act:
        wrong["activation before the residual"] = ref_of(act_first=True)
    if r2 is not None:
        wrong["resid2 dropped"] = ref_of(drop_r2=True)
    if relu_in:
        wrong["input ReLU dropped"] = ref_of(drop_relu_in=True)
    if act == 2:
        wrong["ReLU for LeakyReLU"] = ref_of(code=1)
    errs = _discriminates(gl, wrong, 0 if route == "f32" else 1)
    _report(c, route, err, errs)
    assert err < _bar(route), (err, _bar(route))
    return got


# ------------------------------------------------------------------ the point-map head in the epilogue of a 128-channel ReLU layer
def _head_formula(raw64):
    xyz, cf = raw64[:, :3], raw64[:, 3]
    dn = xyz.norm(dim=1, keepdim=True)
    return xyz / dn.clamp_min(1e-8) * torch.expm1(dn), 1 + torch.exp(cf)


def run_head(c):
    be = _backend()
    B, H, W, cin, cout = c["B"], c["H"], c["W"], c["cin"], c["cout"]
    single, zero, refused = c.get("single", False), c.get("zero", False), bool(c.get("refusal"))
    g = _gen(c)
    # |xyz| follows the input: columns scaled from 0.004 to 1.2 give |xyz| from below 0.01 to about 3
    x = torch.randn(B, cin, H, W, generator=g) * torch.exp(torch.linspace(math.log(0.004), math.log(1.2), W))
    wcout = _ceil_to(cout, 64)
    w = _weights(g, wcout, cin) * (0.0 if zero else 1.0)
    b = torch.randn(wcout, generator=g) * (0.0 if zero else 1e-3)
    hw = torch.randn(4, 128, generator=g) * (0.0 if zero else 1.2 / math.sqrt(128))
    hb = torch.randn(4, generator=g) * (0.0 if zero else 1e-3)
    wt = be.ConvWeights(w, b, DEV)
    n = B * H * W
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    hwd, hbd = hw.contiguous().to(DEV), hb.to(DEV)
    r1 = torch.randn(n * cout, generator=g).to(DEV) if c.get("resid") else None

    def launch(case, with_out, with_raw, missing=None):
        bufs = {"out": _guarded(n * cout), "pts": _guarded(n * 3), "conf": _guarded(n), "raw": _guarded(n * 4)}
        f = dict(entry="split", inp=xd, B=B, H=H, W=W, Cin=cin, Cout=cout, relu=case.get("act", 1), pool=int(case.get("pool", False)), single=int(single),
                 resid=r1, cout_live=case.get("cout_live", 0), head=1, head_w=hwd, head_b=hbd, head_pts=bufs["pts"][1], head_conf=bufs["conf"][1],
                 head_raw=bufs["raw"][1] if with_raw else None, out=bufs["out"][1] if with_out else None, **wt.fields(True))  # fmt: skip
        if missing:
            f[missing] = None
        route = _probe(case, **f)
        for k, (buf, _) in bufs.items():
            _check_guards(buf, route is not None and {"out": with_out, "raw": with_raw}.get(k, True))
        return route, {k: v[1].cpu() for k, v in bufs.items()}

    if refused:
        launch(c, True, True, c.get("missing"))
        return _report(c, None, 0.0)
    # the full variant: the device's own raw, from which pts / conf follow
    full = dict(c, head_out=True, head_raw=True)
    _, base = launch(full, True, True)
    with_out, with_raw = c.get("head_out", True), c.get("head_raw", True)
    route, got = launch(c, with_out, with_raw)
    raw_dev = base["raw"].view(n, 4)
    if with_raw:
        assert torch.equal(got["raw"].view(n, 4), raw_dev), "raw must not depend on which outputs are asked for"
    pts, conf = got["pts"].view(n, 3), got["conf"]
    assert torch.isfinite(pts).all() and torch.isfinite(conf).all()
    if zero:
        assert (pts == 0).all() and (conf == 2).all() and (raw_dev == 0).all()
        if with_out:
            assert (got["out"] == 0).all()
        return _report(c, route, 0.0, extra="  pts exactly 0, conf exactly 2")
    xs, ws = (x.double(), w.double()) if not single else (_round_act(x), _round_single(w, wt.scale))
    feat = torch.relu(F.conv2d(xs, ws, b.double(), padding=1)).permute(0, 2, 3, 1).reshape(n, cout)
    err = 0.0
    if with_out:
        err = _rel(got["out"].view(n, cout), feat)
        swapped = torch.relu(F.conv2d(xs, ws.transpose(-1, -2), b.double(), padding=1)).permute(0, 2, 3, 1).reshape(n, cout)
        _discriminates(got["out"].view(n, cout), {"dy / dx swapped": swapped, "channel c + 32": feat.roll(-32, -1)}, 1)
    raw_ref = feat @ hw.double().t() + hb.double()
    err_raw = _rel(raw_dev, raw_ref)
    wrong = _discriminates(raw_dev, {"second half with the first half's head weights": (feat[:, :64] + feat[:, 64:]) @ hw.double()[:, :64].t() + hb.double(),
                                     "head output c + 1": raw_ref.roll(-1, -1)}, 1)  # fmt: skip
    norm = raw_dev.double()[:, :3].norm(dim=1)
    assert norm.min() < 0.02 and norm.max() > 2.0, (norm.min().item(), norm.max().item())
    pts_ref, conf_ref = _head_formula(raw_dev.double())
    err_pts = ((pts.double() - pts_ref).abs().max(1).values / pts_ref.norm(dim=1)).max().item()
    err_conf = ((conf.double() - conf_ref).abs() / conf_ref).max().item()
    _report(c, route, err, wrong, extra=f"  raw {err_raw:.2e}  pts {err_pts:.2e}  conf {err_conf:.2e} (measured 1.44e-07 / 9.26e-08, bars {HEAD_BAR_PTS:.1e} / {HEAD_BAR_CONF:.1e}, |xyz| {norm.min():.3f} .. {norm.max():.2f})")
    assert err < 4e-6 and err_raw < 4e-6, (err, err_raw)
    assert err_pts < HEAD_BAR_PTS and err_conf < HEAD_BAR_CONF, (err_pts, err_conf)


# ------------------------------------------------------------------ SuperPoint's first layer: conv1a alone, and fused into conv1b
def _first_layers(c):
    g = _gen(c)
    B, H, W = c["B"], c["H"], c["W"]
    img = torch.rand(B, H, W, generator=g)
    w1a = torch.randn(64, 1, 3, 3, generator=g) / 3 + torch.arange(64.0)[:, None, None, None] * 0.01 + TAPS * 0.02
    b1a = torch.randn(64, generator=g) * 0.1
    w1b = _weights(g, 64, 64)
    b1b = torch.randn(64, generator=g) * 0.1
    return img, w1a, b1a, w1b, b1b


def run_first(c):
    be = _backend()
    B, H, W, pool = c["B"], c["H"], c["W"], c.get("pool", False)
    img, w1a, b1a, w1b, b1b = _first_layers(c)
    wt = be.ConvWeights(w1b, b1b, DEV)
    ho, wo = (H // 2, W // 2) if pool else (H, W)
    buf, out = _guarded(B * ho * wo * 64)
    f = dict(entry=c["entry"], inp=img.to(DEV), w1a=be.ConvWeights.first_layer(w1a).to(DEV), b1a=b1a.to(DEV), out=out, B=B, H=H, W=W, pool=int(pool))
    if c["entry"] == "fused":
        f.update(wt.fields(True))
    route = _probe(c, **f)
    _check_guards(buf, route is not None)
    if route is None:
        return _report(c, None, 0.0)
    got = out.view(B, ho, wo, 64).cpu()

    def ref_of(swap_a=False, swap_b=False):
        a = torch.relu(F.conv2d(img.double()[:, None], w1a.double().transpose(-1, -2) if swap_a else w1a.double(), b1a.double(), padding=1))
        if c["entry"] == "conv1a":
            return a.permute(0, 2, 3, 1)
        y = torch.relu(F.conv2d(a, w1b.double().transpose(-1, -2) if swap_b else w1b.double(), b1b.double(), padding=1))
        return (F.max_pool2d(y, 2, 2) if pool else y).permute(0, 2, 3, 1)

    ref = ref_of()
    err = _rel(got, ref)
    wrong = {"dy / dx of the first layer swapped": ref_of(swap_a=True), "channel c + 32": ref.roll(-32, -1)}
    if c["entry"] == "fused":
        wrong["dy / dx of the second layer swapped"] = ref_of(swap_b=True)
    errs = _discriminates(got, wrong, 0 if route == "conv1a" else 1)
    _report(c, route, err, errs)
    assert err < _bar(route), (err, _bar(route))
    return got


# ------------------------------------------------------------------ the case table
def _s(id_, route, **kw):
    """conv3x3_split_launch without a head; defaults B 2, 19 x 37 (3 x 2 tiles of 8 x 32, ragged both ways), 64 -> 128 channels."""
    return {**dict(id=id_, run=run_conv, entry="split", route=route, B=2, H=19, W=37, cin=64, cout=128), **kw}


def _f(id_, **kw):
    return {**dict(id=id_, run=run_conv, entry="f32", route="f32", B=2, H=19, W=37, cin=64, cout=128), **kw}


def _h(id_, route, **kw):
    return {**dict(id=id_, run=run_head, entry="split", route=route, head=True, act=1, B=2, H=19, W=37, cin=64, cout=128, seed="head"), **kw}


def _first(id_, entry, route, **kw):
    return {**dict(id=id_, run=run_first, entry=entry, route=route, B=2, H=19, W=37, seed="first"), **kw}


def _refuse(id_, rule, **kw):
    base = _h if kw.get("head") else _s
    return {**base(id_, None, **kw), "refusal": ERR_ARG, "rule": rule, "opts": kw.get("opts", {"conv_narrow": 2, "conv_tall": 1})}


def _both_widths():
    """The rows the 64-channel (NC = 2) and the 128-channel (NC = 4, conv_narrow = 2) tiling of conv3x3_split_kernel both get."""
    out = []
    for nc, route, narrow, wide in ((2, "split_n2", 64, 192), (4, "split_n4", 128, 256)):
        p = f"n{nc}_"
        out += [
            _s(p + "act0_c32", route, cin=32, cout=narrow, act=0),
            _s(p + "act1_h17_w33_b3", route, B=3, H=17, W=33, cin=64, cout=wide, act=1),  # H % 8 = 1, W % 32 = 1
            _s(p + "act2_h23_w63_c96", route, H=23, W=63, cin=96, cout=128, act=2),  # H % 8 = 7, W % 32 = 31
            _s(p + "pool_relu", route, H=18, W=38, cin=64, cout=narrow, act=1, pool=True),
            _s(p + "pool_leaky_c32", route, B=3, H=18, W=38, cin=32, cout=wide, act=2, pool=True),
            _s(p + "resid_relu", route, cin=64, cout=wide, act=1, resid=True),
            _s(p + "resid_resid2_leaky", route, cin=96, cout=128, act=2, resid=True, resid2=True),
            _s(p + "resid_resid2_act0", route, B=3, cin=32, cout=wide, act=0, resid=True, resid2=True),
            _s(p + "relu_in_code4", route, cin=32, cout=128, act=0, relu_in=True),
            _s(p + "relu_in_code5", route, cin=64, cout=wide, act=1, relu_in=True),
            _s(p + "relu_in_code6", route, cin=96, cout=narrow, act=2, relu_in=True),
            _s(p + "cin_stride_224_of_256", route, cin=224, cout=narrow, act=1, cin_stride=256),
            _s(p + "cout_live_224_of_256", route, cin=64, cout=256, act=1, cout_live=224),
            _s(p + "cout_live_200_of_256", route, cin=32, cout=256, act=2, cout_live=200),
            _s(p + "cout_live_240_of_256", route, B=3, cin=32, cout=256, act=0, cout_live=240),  # live channels inside the last fragment
            _s(p + "smaller_than_a_tile", route, B=3, H=3, W=5, cin=64, cout=narrow, act=1),
        ]
    return out


CASES = [
    # the exact f32 kernel (8 x 16 tiles): ReLU on / off, pool on / off
    _f("f32_relu", cin=64, cout=128, act=1),
    _f("f32_plain_c96", B=3, H=17, W=33, cin=96, cout=64, act=0),
    _f("f32_pool_relu", H=18, W=38, cin=32, cout=192, act=1, pool=True),
    _f("f32_pool_plain", H=18, W=38, cin=64, cout=256, act=0, pool=True),
    *_both_widths(),
    # the default routing rule: fewer than 256 workgroups of 128 channels -> 64-channel tiles although Cout % 128 == 0 (one seed: the
    # three results are compared bitwise by test_channel_tiles_are_bitwise_equal)
    _s("rule_default_narrow0", "split_n2", seed="rule", cin=64, cout=256, act=1, resid=True, opts={"conv_narrow": 0, "conv_tall": 1}),
    _s("rule_always_narrow1", "split_n2", seed="rule", cin=64, cout=256, act=1, resid=True, opts={"conv_narrow": 1, "conv_tall": 1}),
    _s("rule_never_narrow2", "split_n4", seed="rule", cin=64, cout=256, act=1, resid=True, opts={"conv_narrow": 2, "conv_tall": 1}),
    # one f16 product per element pair
    _s("n2_single_resid_relu_in", "split_n2_single", cin=96, cout=192, act=1, resid=True, relu_in=True, single=True),
    _s("n4_single_resid_relu_in", "split_n4_single", B=3, H=17, W=33, cin=64, cout=256, act=1, resid=True, relu_in=True, single=True),
    _s("n2_single_leaky_pool", "split_n2_single", H=18, W=38, cin=32, cout=64, act=2, pool=True, single=True),
    _s("n2_single_resid_resid2_act0", "split_n2_single", cin=32, cout=128, act=0, resid=True, resid2=True, single=True),
    _s("n4_single_leaky", "split_n4_single", cin=96, cout=128, act=2, single=True),
    _s("n4_single_resid2_cin_stride", "split_n4_single", cin=224, cout=128, act=0, resid=True, resid2=True, cin_stride=256, single=True),
    # 16-row tiles for plain layers (conv_tall = 2): Cout 64 and 192, Cin 96 = three pairs of 16-channel stages
    _s("tall_pool", "tall", H=18, W=38, cin=96, cout=64, act=1, pool=True),
    _s("tall_resid_resid2", "tall", B=3, H=23, W=63, cin=64, cout=192, act=2, resid=True, resid2=True),
    _s("tall_relu_in", "tall", H=17, W=33, cin=96, cout=192, act=1, relu_in=True),
    _s("tall_cin_stride", "tall", cin=224, cout=64, act=0, cin_stride=256),
    _s("tall_single_pool", "tall_single", H=18, W=38, cin=32, cout=192, act=2, pool=True, single=True),
    _s("tall_single_resid_resid2", "tall_single", cin=96, cout=64, act=1, resid=True, resid2=True, single=True),
    _s("tall_single_relu_in", "tall_single", B=3, H=3, W=5, cin=64, cout=64, act=0, relu_in=True, single=True),
    _s("tall_single_cin_stride", "tall_single", H=23, W=63, cin=224, cout=192, act=1, cin_stride=256, single=True),
    _s("tall_falls_back_for_cout_live", "split_n2", cin=64, cout=192, act=1, cout_live=160, opts={"conv_narrow": 1, "conv_tall": 2}),
    # the point-map head: out / raw given or not, both arithmetic options, all-zero layer
    _h("head_out_raw", "split_n4"),
    _h("head_no_out", "split_n4", head_out=False),
    _h("head_no_raw", "split_n4", head_raw=False),
    _h("head_single_out_raw", "split_n4_single", single=True),
    _h("head_single_no_out", "split_n4_single", single=True, head_out=False),
    _h("head_single_no_raw", "split_n4_single", single=True, head_raw=False, B=3, H=17, W=33),
    _h("head_all_zero", "split_n4", zero=True, H=9, W=33),
    # SuperPoint's first layer alone and fused into conv1b (16-row tiles by default, 8-row tiles with conv_tall = 0)
    _first("conv1a_alone", "conv1a", "conv1a"),
    _first("fused_tall", "fused", "fused_tall"),
    _first("fused_tall_pool", "fused", "fused_tall", H=18, W=38, pool=True),
    _first("fused_8row", "fused", "fused_8row"),
    _first("fused_8row_pool", "fused", "fused_8row", H=18, W=38, pool=True, seed="first_pool"),
    # refusals of conv3x3_split_launch: nothing launched, nothing written
    _refuse("refuse_pool_with_resid", "pool_resid", H=18, W=38, pool=True, resid=True),
    _refuse("refuse_resid2_without_resid", "resid2_alone", resid2=True),
    _refuse("refuse_cin_48", "cin_mod_32", cin=48),
    _refuse("refuse_cout_96", "cout_mod_64", cout=96),
    _refuse("refuse_pool_odd_h", "pool_odd", H=19, W=38, pool=True),
    _refuse("refuse_pool_odd_w", "pool_odd", H=18, W=37, pool=True),
    _refuse("refuse_cin_stride_below_cin", "cin_stride_small", cin=64, cin_stride=32),
    _refuse("refuse_cin_stride_66", "cin_stride_mod_4", cin=64, cin_stride=66),
    _refuse("refuse_null_out", "null_out", null_out=True),
    _refuse("refuse_head_cout_256", "head_cout", head=True, cout=256),
    _refuse("refuse_head_pool", "head_pool", head=True, H=18, W=38, pool=True),
    _refuse("refuse_head_resid", "head_resid", head=True, resid=True),
    _refuse("refuse_head_act0", "head_act", head=True, act=0),
    _refuse("refuse_head_leaky", "head_act", head=True, act=2),
    _refuse("refuse_head_cout_live", "head_cout_live", head=True, cout_live=96),
    _refuse("refuse_head_narrow1", "head_narrow", head=True, opts={"conv_narrow": 1, "conv_tall": 1}),
    _refuse("refuse_head_no_pts", "head_pointer", head=True, missing="head_pts"),
    _refuse("refuse_head_no_conf", "head_pointer", head=True, missing="head_conf"),
    _refuse("refuse_head_no_w", "head_pointer", head=True, missing="head_w"),
    _refuse("refuse_head_no_b", "head_pointer", head=True, missing="head_b"),
]


def covered_pairs() -> set:
    """{(route name, feature bit or 0)} the launched cases of the table record."""
    out = set()
    for c in CASES:
        if c.get("refusal"):
            continue
        f = case_features(c)
        out.add((c["route"], 0))
        out |= {(c["route"], bit) for bit in FEATURES.values() if f & bit}
        if c["run"] is run_head:  # (run_head also launches the variant with out and raw)
            out |= {(c["route"], FEATURES["head"]), (c["route"], FEATURES["head_raw"])}
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_conv_variant(case):
    case["run"](case)


def _by_id(cid):
    return next(c for c in CASES if c["id"] == cid)


def test_channel_tiles_are_bitwise_equal():
    """conv_narrow 0 (the default rule, which picks 64-channel tiles at this size), 1 and 2: the same arithmetic per output, residual included."""
    outs = [run_conv(_by_id(i)) for i in ("rule_default_narrow0", "rule_always_narrow1", "rule_never_narrow2")]
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2])


def test_fused_first_layer_equals_the_two_launches_bitwise():
    """conv.hip: 'the arithmetic of conv1a is the same fmaf chain as conv1a_kernel, so the fused and unfused paths agree bit for bit':
    conv1a_kernel followed by conv3x3_split_kernel<false, 2> against conv3x3_split_kernel<true, 2>, with and without the pool."""
    be = _backend()
    for cid in ("fused_8row", "fused_8row_pool"):
        c = _by_id(cid)
        fused = run_first(c)
        B, H, W, pool = c["B"], c["H"], c["W"], c.get("pool", False)
        img, w1a, b1a, w1b, b1b = _first_layers(c)
        a1 = torch.empty(B, H, W, 64, device=DEV)
        with be.option(DEV, conv_tall=0, conv_narrow=1):
            r = be.conv_probe(DEV, entry="conv1a", inp=img.to(DEV), w1a=be.ConvWeights.first_layer(w1a).to(DEV), b1a=b1a.to(DEV), out=a1, B=B, H=H, W=W)
            assert r == be.conv_route("conv1a")
            two = torch.empty_like(fused, device=DEV)
            r = be.conv_probe(DEV, entry="split", inp=a1, out=two, B=B, H=H, W=W, Cin=64, Cout=64, relu=1, pool=int(pool), **be.ConvWeights(w1b, b1b, DEV).fields(True))
            assert r == be.conv_route("split_n2")
        torch.cuda.synchronize()
        assert torch.equal(two.cpu(), fused), cid


# ------------------------------------------------------------------ the gate: every (route, feature) a network launches has a case above
# Networks of the sweep (test_gpu_gemm_variants.networks) that launch kernels of conv.hip in the split mode: True when they do in the
# exact f32 mode too.  SuperPoint, D2-Net, NetVLAD (their VGG-16 trunks) and DeDoDe (its VGG-19 encoder) call conv3x3_launch or
# conv3x3_split_launch by the handle's mode; the dense matchers' 3x3 layers run on the GEMM in the exact mode.  A network of the sweep
# that is not named here must launch none (the gate asserts that too).
NETWORKS = {
    "SuperPoint+LightGlue": True,
    "LoFTR": False,
    "EfficientLoFTR": False,
    "DUSt3R": False,
    "MASt3R": False,
    "D2-Net ss": True,
    "D2-Net ms": True,
    "DeDoDe": True,
    "NetVLAD": True,
    "NetVLAD whitened": True,
}


def test_conv_routes_of_every_network_are_covered():
    """Every network of the tree once in each arithmetic mode (the sweep of the GEMM gate, test_gpu_gemm_variants.network_sweep: one
    cached pass that reads all four route recorders per network): every (route, feature bit) pair they launched must be one a case of the
    table launches; a network of NETWORKS must have recorded a convolution launch (the split mode: all; the exact mode: those flagged),
    and a network that is not in NETWORKS none."""
    from test_gpu_gemm_variants import network_sweep

    be = _backend()
    seen_counts, seen_pairs = {}, set()
    unknown = set(NETWORKS) - {name for _, name in network_sweep()}
    assert not unknown, f"NETWORKS names no network of the sweep: {sorted(unknown)}"
    for (mode, name), rec in network_sweep().items():
        launches = sum(n for n, _ in rec["conv"].values())
        if name in NETWORKS:
            if mode == 1 or NETWORKS[name]:
                assert launches > 0, f"{name}: no convolution launch recorded in mode {mode}"
        else:
            assert launches == 0, f"{name} launches conv.hip in mode {mode} ({launches} launches): add it to NETWORKS"
        if launches:
            print(f"[conv-gate] mode {mode} {name}: {launches} launches, " + ", ".join(
                f"{be.conv_route_name(r)} [{' '.join(be.conv_feature_names(m)) or '-'}]" for r, (n, m) in sorted(rec["conv"].items())))  # fmt: skip
        for r, (n, mask) in rec["conv"].items():
            seen_counts[r] = seen_counts.get(r, 0) + n
            rname = be.conv_route_name(r)
            seen_pairs.add((rname, 0))
            seen_pairs |= {(rname, bit) for bit in FEATURES.values() if mask & bit}
    cov = covered_pairs()
    bit_name = {v: k for k, v in FEATURES.items()}
    fmt = lambda pairs: ", ".join(f"{r}+{bit_name[b]}" if b else r for r, b in sorted(pairs))  # noqa: E731
    print("[conv-gate] routes launched by the networks: " + ", ".join(f"{be.conv_route_name(r)} x{n}" for r, n in sorted(seen_counts.items())))
    print("[conv-gate] (route, feature) launched by the networks: " + fmt(seen_pairs))
    print("[conv-gate] (route, feature) covered by the case table: " + fmt(cov))
    assert seen_counts, "no convolution launch recorded"
    missing = seen_pairs - cov
    assert not missing, "launched without a kernel-level case: " + fmt(missing)
