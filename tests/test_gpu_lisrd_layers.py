"""The stages of the LISRD forward (csrc/lisrd.hip) one at a time through their test entries, against float64 torch (GPU box only).

Bars: the project's layer rule (tests/test_gpu_sfd2_layers.py).  Errors are relative to the largest magnitude of the float64 result.  Every
bar is 3 x the error of the SAME operation in float32 torch on the CPU against float64 on the same input, floored at half a float32 ulp
of that magnitude (3 x 6e-8 = 1.8e-07); a stage whose values come out of the shared GEMM adds that GEMM's own bar, 2e-6 (exact f32) /
4e-6 (3 x f16 split).  Every test prints its figures before it asserts."""
import functools

import pytest
import torch
import torch.nn.functional as F

import lisrd_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1.8e-07


@functools.lru_cache(maxsize=None)
def _sd():
    from imcui_hip.synth_weights import lisrd_synth_state

    return lisrd_synth_state(0)


@functools.lru_cache(maxsize=None)
def _net(double=False):
    net = R.LisrdNet().eval()
    net.load_state_dict(_sd())
    return net.double() if double else net


@functools.lru_cache(maxsize=None)
def _packed():
    from imcui_hip import backend

    return backend.pack_lisrd(_sd()).to(DEV)


def _impl():
    from imcui_hip import backend

    return backend.LisrdHIP()


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rel(a, ref):
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def own_bar(r32, r64, extra=0.0):
    """(3 x the float32 restatement's own relative error against float64, floored at 1.8e-07, + extra; that own error)"""
    own = rel(r32, r64)
    return max(3.0 * own, FLOOR) + extra, own


def gemm_term(precision):
    return 4e-6 if precision == 1 else 2e-6


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("h,w", [(24, 24), (33, 70)])
def test_stem_reads_times_255_over_255(precision, h, w):
    x = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(h))
    bb32, bb64 = _net()._backbone, _net(True)._backbone
    trip = (x * 255.0) / 255.0  # two float32 roundings
    assert not torch.equal(trip, x)
    with torch.no_grad():
        r32, plain = bb32._bn1_1(F.relu(bb32._conv1_1(trip))), bb32._bn1_1(F.relu(bb32._conv1_1(x)))
        r64 = bb64._bn1_1(F.relu(bb64._conv1_1(trip.double())))
    assert not torch.equal(r32, plain)  # (a reference without the round trip differs in bits: the case shows something)
    got = _impl().layers_probe(_packed(), x.to(DEV), 0, 0).cpu()
    bar, own = own_bar(nhwc(r32), nhwc(r64))
    err = rel(got, nhwc(r64))
    print(f"stem {h}x{w}: error {err:.3g}, the restatement's own {own:.3g}, bar {bar:.3g}; without the round trip the reference moves by {float((r32 - plain).abs().max()):.3g}")
    assert err <= bar
    # The round trip moves an input by at most one ulp, which is below the bar above.  One pixel tells the two reads apart beyond any bar:
    # 2e36 * 255 overflows float32, so the wrapper's read of that pixel is inf and, at the pixel itself (its only infinite tap), every
    # channel whose centre weight for that input channel is positive leaves the ReLU as inf; read without the round trip, everything stays finite.
    big = x.clone()
    cy, cx = h // 2, w // 2
    big[1, 0, cy, cx] = 2e36  # (one channel: a single infinite tap, so no inf - inf)
    with torch.no_grad():
        t32 = bb32._bn1_1(F.relu(bb32._conv1_1((big * 255.0) / 255.0)))[1, :, cy, cx]
        p32 = bb32._bn1_1(F.relu(bb32._conv1_1(big)))
    centre = _impl().layers_probe(_packed(), big.to(DEV), 0, 0).cpu()[1, cy, cx]
    print(f"stem {h}x{w}: overflowing pixel: {int(torch.isinf(t32).sum())} of 64 channels infinite in the reference, {int(torch.isinf(centre).sum())} on the device")
    assert bool(torch.isfinite(p32).all()) and 0 < int(torch.isinf(t32).sum()) < 64
    assert torch.equal(torch.isinf(centre), torch.isinf(t32)) and not bool(torch.isnan(centre).any())


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("h,w", [(2, 2), (3, 5), (33, 70)])
def test_affine_and_pool(precision, C, h, w):
    x = rnd(3, h, w, C, seed=C + h)
    a = rnd(C, seed=1) * 1.5  # (negative entries among them)
    a[0] = -2.0
    b = rnd(C, seed=2)
    impl = _impl()
    for pool in (False, True):
        got = impl.affine_probe(x.to(DEV), a.to(DEV), b.to(DEV), pool).cpu()
        ref = lambda t: (nhwc(F.avg_pool2d(t.permute(0, 3, 1, 2), 2, 2)) if pool else t) * a.to(t.dtype) + b.to(t.dtype)
        r32, r64 = ref(x), ref(x.double())
        assert got.shape == r64.shape == (3, h // 2 if pool else h, w // 2 if pool else w, C)
        bar, own = own_bar(r32, r64)
        err = rel(got, r64)
        print(f"affine C={C} {h}x{w} pool={pool}: error {err:.3g}, own {own:.3g}, bar {bar:.3g}")
        assert err <= bar
        solo = impl.affine_probe(x[1:2].to(DEV), a.to(DEV), b.to(DEV), pool).cpu()
        assert torch.equal(solo[0], got[1])  # an image alone and inside a batch: the same bits
        if pool and (h % 2 or w % 2):  # the last row / column of an odd map is not read
            x2 = x.clone()
            if h % 2:
                x2[:, h - 1] = float("nan")
            if w % 2:
                x2[:, :, w - 1] = float("nan")
            assert torch.equal(impl.affine_probe(x2.to(DEV), a.to(DEV), b.to(DEV), True).cpu(), got)


def test_fused_heads_and_a_1x1_layer(precision):
    """the N = 2048 launch of the eight hidden head layers and a head's 1x1 layer, through the forward's own launch list, on a 3x4 map"""
    n32, n64 = _net(), _net(True)
    x = rnd(2, 256, 3, 4, seed=5)
    names = [("", v) for v in R.VARIANCES] + [("_meta", v) for v in R.VARIANCES]
    hid = lambda n, t: torch.cat([getattr(n, f"bn{p}_{v}_1")(F.relu(getattr(n, f"conv{p}_{v}_1")(t))) for p, v in names], 1)
    with torch.no_grad():
        h32, h64 = hid(n32, x), hid(n64, x.double())
    got = _impl().layers_probe(_packed(), nhwc(x).to(DEV), 8, 8).cpu()
    bar, own = own_bar(nhwc(h32), nhwc(h64), gemm_term(precision))
    err = rel(got, nhwc(h64))
    print(f"fused head launch: error {err:.3g}, own {own:.3g}, bar {bar:.3g}; largest magnitude {float(h64.abs().max()):.3g}")
    assert got.shape == (2, 3, 4, 2048) and err <= bar
    for j in (0, 6):  # descriptor head of variance 0, meta head of variance 2
        p, v = names[j]
        with torch.no_grad():
            r32 = getattr(n32, f"conv{p}_{v}_2")(h32[:, 256 * j : 256 * (j + 1)])
            r64 = getattr(n64, f"conv{p}_{v}_2")(h32.double()[:, 256 * j : 256 * (j + 1)])
        got = _impl().layers_probe(_packed(), nhwc(h32).to(DEV), 9 + j, 9 + j).cpu()
        bar, own = own_bar(nhwc(r32), nhwc(r64), gemm_term(precision))
        err = rel(got, nhwc(r64))
        print(f"1x1 layer {9 + j}: error {err:.3g}, own {own:.3g}, bar {bar:.3g}")
        assert got.shape == (2, 3, 4, 128) and err <= bar


@functools.lru_cache(maxsize=None)
def _underflow():
    """weights whose cluster 3 takes or loses everything: its assignment weights are 4000 x the drawn ones (logits of several hundred)"""
    from imcui_hip import backend

    sd = dict(_sd())
    w = sd["vlad_rot_invar_illum_var.conv.weight"].clone()
    w[3] *= 4000.0
    sd["vlad_rot_invar_illum_var.conv.weight"] = w
    n32 = R.LisrdNet().eval()
    n32.load_state_dict(sd)
    n64 = R.LisrdNet().double().eval()
    n64.load_state_dict(sd)
    return backend.pack_lisrd(sd).to(DEV), n32, n64


@pytest.mark.parametrize("hc,wc", [(3, 3), (6, 8), (12, 16)])
def test_regional_netvlad(precision, hc, wc):
    packed, n32, n64 = _underflow()
    impl = _impl()
    for vi in (0, 1):  # variance 1 carries the underflowing cluster
        v = R.VARIANCES[vi]
        m = rnd(2, 128, hc, wc, seed=hc + vi)
        m[0, :, 1, 1] = 0.0  # a cell of all zeros
        with torch.no_grad():
            r32, r64 = n32.regional_vlad(m, v), n64.regional_vlad(m.double(), v)
            a = F.softmax(getattr(n64, f"vlad_{v}").conv(F.normalize(m.double(), dim=1)), dim=1)
        got = impl.vlad_probe(packed, vi, nhwc(m).to(DEV)).cpu()  # [B, 3, 3, 1024]
        bar, own = own_bar(nhwc(r32), nhwc(r64))
        err = rel(got, nhwc(r64))
        print(f"regional NetVLAD {hc}x{wc} variance {vi}: error {err:.3g}, own {own:.3g}, bar {bar:.3g}; smallest assignment {float(a.min()):.3g}")
        assert err <= bar and bool(torch.isfinite(got).all())
        if vi == 1:
            assert float(a.min()) < 1e-30  # (the case is what it says)
        # dropped cells do not matter: NaN in them leaves the bits
        th, tw = hc // 3, wc // 3
        if 3 * th < hc or 3 * tw < wc:
            m2 = m.clone()
            m2[:, :, 3 * th :], m2[:, :, :, 3 * tw :] = float("nan"), float("nan")
            assert torch.equal(impl.vlad_probe(packed, vi, nhwc(m2).to(DEV)).cpu(), got)
        solo = impl.vlad_probe(packed, vi, nhwc(m[1:2]).to(DEV)).cpu()
        assert torch.equal(solo[0], got[1])


@pytest.mark.parametrize("count", [1, 63, 64, 65, 200])
def test_sparse_sampling(precision, count):
    from imcui_hip import backend

    hc, wc, H, W = 5, 7, 40, 59  # W is no multiple of 8: the map is 7 cells wide, 3 pixels are past its last cell
    B, K = 2, count + 2
    dm = rnd(4, B, 128, hc, wc, seed=count)
    vl = F.normalize(rnd(B, 4, 1024, 3, 3, seed=count + 1), dim=2)
    g = torch.Generator().manual_seed(count)
    kp = torch.rand(B, K, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])
    # the image corners (three of a cell's four corners lie outside the map), a position near the border, the centre of cell (1, 2)
    # (i = 2, 1 up to float32 rounding), an integer position
    special = torch.tensor([[0.0, 0.0], [W - 1.0, H - 1.0], [W - 1.0, 0.0], [0.5, H - 1.25], [W / wc * 2.5, H / hc * 1.5], [20.0, 12.0]])
    kp[:, : min(count, len(special))] = special[: min(count, len(special))]
    cnt = torch.tensor([count, max(count - 1, 0)], dtype=torch.int32)
    out = backend.LisrdHIP.sample_probe(dm.permute(0, 1, 3, 4, 2).to(DEV), vl.permute(0, 1, 3, 4, 2).to(DEV), (H, W), kp.to(DEV), cnt)
    out = {k: t.cpu() for k, t in out.items()}
    for b in range(B):
        n = int(cnt[b])
        if n == 0:
            continue
        maps = lambda dt: {"descriptors": {v: dm[i, b : b + 1].to(dt) for i, v in enumerate(R.VARIANCES)},
                           "meta_descriptors": {v: vl[b : b + 1, i].to(dt) for i, v in enumerate(R.VARIANCES)}}  # fmt: skip
        d32, m32 = R.extract_descriptors(kp[b, :n], maps(torch.float32), (H, W))
        d64, m64 = R.extract_descriptors(kp[b, :n].double(), maps(torch.float64), (H, W), torch.float64)
        for name, got, r32, r64, D in (("desc", out["desc"][b], d32, d64, 128), ("meta", out["meta"][b], m32, m64, 1024)):
            bar, own = own_bar(r32, r64)
            err = rel(got[:n], r64)
            nerr = float((got[:n].double().norm(dim=-1) - 1).abs().max())
            print(f"sampling count={count} b={b} {name}: error {err:.3g}, own {own:.3g}, bar {bar:.3g}; norms off by {nerr:.3g}")
            assert err <= bar and nerr <= bar
            assert bool((got[n:] == 0).all())  # rows past the count
