"""The kernels DarkFeat adds (csrc/darkfeat.hip), each alone against the float64 restatement (tests/darkfeat_reference.py).

Every bar is 3 x the error of the SAME operation in float32 torch on the CPU against float64 on the same input, computed here (relative
to the largest magnitude of the float64 result, floored at half a float32 ulp of that magnitude, 6e-8), the project's layer rule.  A
launch that goes through the shared GEMM adds that GEMM's own bar, 2e-6 exact / 4e-6 split (tests/test_gpu_gemm_dilated.py).

  statistics + layer 0   16x16 and 33x70, B = 2: mean / unbiased std per image, the raw layer-0 map; a reference without the
                         normalisation and one padded in raw units must both miss by orders more than the bar
  InstanceNorm           C = 32 / 64 / 128 on 1x1 (variance 0: the output is 0 through eps), 3x5, 33x70 (2310 pixels: three statistics
                         chunks of 1024) maps, B = 2, one constant channel; the same image alone gives the same bits
  stride-2 layers        33x70 -> 17x35 -> 9x18 through the forward's own launch list (conv2, conv4), both arithmetic modes
  peakiness              (C, d) = (32, 3), (64, 2), (128, 1) on maps of d + 1 rows and columns, 5x7 and 33x70; inputs beyond +-20
                         exercise the softplus threshold; zero padding instead of reflect, and d = 1 instead of d, must both miss
  score assembly         16x16, 18x22 (1/2 and 1/4 maps of 9x11 and 5x6) and 50x70
  describe               on given maps: integer and fractional quarter positions, the clamped last row / column, rows past the count

Measured on one MI355X: layer 0 2.0e-07 / 2.2e-07 (bars 6.1e-07 / 6.6e-07), mean / std within 4.8e-08, the wrong references off by 1.17 .. 1.31
(padding in raw units) and 1.01 .. 1.11 (no normalisation); InstanceNorm exactly 0 on 1x1, 6.5e-08 .. 1.3e-07 on 3x5 (bars 3.8e-07 ..
1.7e-06), 7.6e-08 .. 8.4e-08 on 33x70 (bars 3.6e-07 .. 8.6e-07); conv2 5.0e-07 split / 5.2e-07 exact, conv4 7.8e-07 / 7.7e-07 raw and 8.9e-07 /
8.5e-07 normalised (bars 5.1e-06 .. 5.9e-06 split, 3.1e-06 .. 3.9e-06 exact); peakiness 8.5e-09 .. 1.1e-07 (bars 1.8e-07 .. 3.3e-07), zero
padding off by 1.7e-03 .. 2.1 and d = 1 by 7.2e-03 .. 2.1; score assembly 2.2e-07 / 2.5e-07 / 7.1e-07 (bars 1.2e-06 / 9.8e-07 / 2.3e-06);
describe 1.3e-07 / 8.7e-08 (bars 3.8e-07 / 2.9e-07), norms 1 within 8.3e-08.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import darkfeat_reference as R
from test_darkfeat_cpu import image, net, state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ULP_HALF = 6e-8
GEMM_BAR = {0: 2e-6, 1: 4e-6}  # exact / split


def rel(a, ref):
    return ((a.double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max().clamp_min(1e-30)).item()


def _bar(f32, ref):
    """3 x the float32 restatement's own error against float64."""
    return 3 * max(rel(f32, ref), ULP_HALF)


@functools.lru_cache(maxsize=None)
def _impl():
    from imcui_hip import backend

    return backend.pack_darkfeat(state()).to(DEV), backend.DarkFeatHIP()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------ image statistics + layer 0
@pytest.mark.parametrize("hw", [(16, 16), (33, 70)])
def test_image_statistics_and_layer0(hw):
    packed, impl = _impl()
    img = image(*hw, seed=1, batch=2)
    img[1] = img[1] * 3.0 + 0.7  # the two images of the batch have different statistics
    got = impl.stem_probe(packed, img.to(DEV))
    torch.cuda.synchronize()
    m64, m32 = net(double=True), net()
    d = img.double()
    with torch.no_grad():
        ref, f32 = nhwc(m64.conv0(R.normalise_image(d))), nhwc(m32.conv0(R.normalise_image(img)))
        wrong_norm = nhwc(m64.conv0(d))
        mean, std = d.mean(dim=(1, 2, 3), keepdim=True), d.std(dim=(1, 2, 3), keepdim=True)
        wrong_pad = nhwc(F.conv2d((F.pad(d, (1, 1, 1, 1)) - mean) / std, m64.conv0[0].weight))  # the border padded in RAW units
    stat_ref = torch.stack([mean.flatten(), std.flatten()], dim=1)
    serr = ((got["imstat"].cpu().double() - stat_ref).abs() / stat_ref.abs()).max().item()
    err, bar = rel(got["raw"], ref), _bar(f32, ref)
    miss = (rel(wrong_pad, ref), rel(wrong_norm, ref))
    print(f"layer 0 at {hw}: {err:.2e} (bar {bar:.2e}); mean / std {serr:.2e}; padded in raw units misses by {miss[0]:.2e}, without the normalisation by {miss[1]:.2e}")
    assert got["raw"].shape == ref.shape and err <= bar and serr <= 3e-7 and int(got["status"][0]) == 0
    assert min(miss) > 1000 * bar


# ------------------------------------------------------------------ InstanceNorm
@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (33, 70)])
def test_instance_norm(C, hw):
    _, impl = _impl()
    g = torch.Generator().manual_seed(100 * C + hw[0])
    x = torch.randn(2, C, *hw, generator=g) * 1.7 + 0.4 * torch.randn(1, C, 1, 1, generator=g)
    x[:, 3] = 2.5  # a constant channel
    x[1, 5] += 30.0  # a channel far from zero
    out, stat = impl.inorm_probe(nhwc(x).to(DEV))
    solo, _ = impl.inorm_probe(nhwc(x[1:]).to(DEV))
    torch.cuda.synchronize()
    ref, f32 = nhwc(R.inorm_relu(x.double())), nhwc(R.inorm_relu(x))
    err, bar = rel(out, ref), _bar(f32, ref)
    mean_err = (stat[..., 0].cpu().double() - x.double().mean(dim=(2, 3))).abs().max().item()
    print(f"InstanceNorm C={C} map {hw} ({hw[0] * hw[1]} pixels): {err:.2e} (bar {bar:.2e}); channel means {mean_err:.2e}")
    assert torch.equal(out[1], solo[0]), "bits are independent of the batch"
    assert not out[..., 3].any(), "a constant channel is 0 through eps"
    if hw == (1, 1):
        assert not out.any(), "one pixel: variance 0, output 0"
        assert torch.equal(stat[..., 0].cpu(), x[:, :, 0, 0])
    else:
        assert err <= bar and bool((out > 0).any())


# ------------------------------------------------------------------ the stride-2 layers through the forward's launch list
def test_stride2_layers_through_the_forward(precision):
    from imcui_hip.hloc.extractors.darkfeat import DarkFeat

    m = DarkFeat({"state_dict": state()}).eval().to(DEV)
    img = image(33, 70, seed=2, batch=2)
    with torch.no_grad():
        o64, o32 = net(double=True).parts(img.double()), net().parts(img)
    for layer, shape in ((2, (17, 35)), (4, (9, 18))):
        out = m.forward_batched(img.to(DEV), layer=layer)
        torch.cuda.synchronize()
        assert R.LAYERS[layer][3] == 2 and tuple(out["layer_raw"].shape[1:3]) == shape == tuple(o64["raw"][layer].shape[-2:])
        for key in ("raw", "norm"):
            ref, f32 = nhwc(o64[key][layer]), nhwc(o32[key][layer])
            err, bar = rel(out[f"layer_{key}"], ref), _bar(f32, ref) + GEMM_BAR[precision]
            print(f"{R.LAYERS[layer][0]} {key} at 33x70 -> {shape}, precision {precision}: {err:.2e} (bar {bar:.2e})")
            assert err <= bar


# ------------------------------------------------------------------ peakiness
@pytest.mark.parametrize("C,d", [(32, 3), (64, 2), (128, 1)])
@pytest.mark.parametrize("hw", ["smallest", (5, 7), (33, 70)])
def test_peakiness(C, d, hw):
    _, impl = _impl()
    h, w = (d + 1, d + 1) if hw == "smallest" else hw
    g = torch.Generator().manual_seed(10 * C + h)
    x = torch.randn(2, C, h, w, generator=g) * 1.3
    x[0, 1, h // 2, w // 2] = 45.0  # softplus beyond +20 ...
    x[1, 2, 0, 0] = -60.0  # ... and far below -20
    x[1, 4, h - 1, w - 1] = 31.0
    mavg = 0.8125  # (exact in float32)
    got = impl.peak_probe(nhwc(x).to(DEV), d, mavg)
    torch.cuda.synchronize()
    ref, f32 = R.peakiness(x.double(), d, mavg), R.peakiness(x, d, torch.tensor(mavg))
    err, bar = rel(got, ref), _bar(f32, ref)
    miss = [rel(R.peakiness(x.double(), d, mavg, pad_mode="constant"), ref)]
    if d > 1:
        miss.append(rel(R.peakiness(x.double(), 1, mavg), ref))
    print(f"peakiness C={C} d={d} map {h}x{w}: {err:.2e} (bar {bar:.2e}); zero padding misses by {miss[0]:.2e}" + (f", d = 1 by {miss[1]:.2e}" if d > 1 else ""))
    assert got.shape == ref.shape and err <= bar
    assert min(miss) > 1000 * bar
    assert float(ref.max()) > 20.0, "the softplus threshold is exercised"


def test_peakiness_refuses_a_map_without_reflect_padding():
    from imcui_hip import backend

    _, impl = _impl()
    with pytest.raises(backend.ImcuiHipError, match="reflect"):
        impl.peak_probe(torch.zeros(1, 3, 9, 32, device=DEV), 3, 1.0)
    with pytest.raises(backend.ImcuiHipError, match="built for"):
        impl.peak_probe(torch.zeros(1, 9, 9, 32, device=DEV), 2, 1.0)


# ------------------------------------------------------------------ score assembly
@pytest.mark.parametrize("hw", [(16, 16), (18, 22), (50, 70)])
def test_score_assembly(hw):
    from imcui_hip import backend

    packed, impl = _impl()
    H, W = hw
    h2, w2, h4, w4 = backend.darkfeat_map_sizes(H, W)
    if hw == (18, 22):
        assert (h2, w2, h4, w4) == (9, 11, 5, 6)
    g = torch.Generator().manual_seed(H)
    pk = [torch.rand(2, *s, generator=g) * 4.0 for s in ((H, W), (h2, w2), (h4, w4))]
    dmap = torch.randn(2, 128, h4, w4, generator=g) * 1.5
    got = impl.score_probe(packed, *[p.to(DEV) for p in pk], nhwc(dmap).to(DEV))
    torch.cuda.synchronize()
    m64, m32 = net(double=True), net()
    with torch.no_grad():
        ref = R.assemble([p.double() for p in pk], dmap.double(), m64.clf.weight, m64.clf.bias, H, W)
        f32 = R.assemble(pk, dmap, m32.clf.weight, m32.clf.bias, H, W)
        prob = R.clf_prob(dmap.double(), m64.clf.weight, m64.clf.bias)
    err, bar = rel(got, ref), _bar(f32, ref)
    print(f"score assembly at {hw}: {err:.2e} (bar {bar:.2e}); classifier probability {prob.min():.3f} .. {prob.max():.3f}")
    assert got.shape == ref.shape and err <= bar and float(prob.max() - prob.min()) > 0.02


# ------------------------------------------------------------------ describe
def test_describe_on_given_maps():
    _, impl = _impl()
    g = torch.Generator().manual_seed(9)
    H, W = 50, 70
    h4, w4 = 13, 18
    dmap = torch.randn(2, 128, h4, w4, generator=g)
    kp = torch.stack([torch.randint(0, W, (2, 40), generator=g), torch.randint(0, H, (2, 40), generator=g)], dim=2).float()
    kp[0, :6] = torch.tensor([[0.0, 0.0], [69.0, 49.0], [68.0, 48.0], [4.0, 8.0], [67.0, 3.0], [1.0, 47.0]])  # corners, an exact map pixel, clamped ceil
    nk = torch.tensor([40, 17])
    got = impl.describe_probe(nhwc(dmap).to(DEV), kp.to(DEV), nk)
    torch.cuda.synchronize()
    for b in range(2):
        n = int(nk[b])
        ref, f32 = R.describe(dmap[b].double(), kp[b, :n].double()), R.describe(dmap[b], kp[b, :n])
        err, bar = rel(got[b, :n], ref), _bar(f32, ref)
        norm = (got[b, :n].double().norm(dim=1) - 1).abs().max().item()
        print(f"describe image {b}: {n} key-points {err:.2e} (bar {bar:.2e}), |norm - 1| {norm:.1e}")
        assert err <= bar and norm < 1e-5 and not got[b, n:].any()
    assert rel(got[0, 3], F.normalize(dmap[0, :, 2, 1].double(), dim=0)) < 2e-7, "(4, 8) / 4 is the map pixel (1, 2) itself"
