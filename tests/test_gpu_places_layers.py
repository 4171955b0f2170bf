"""The kernels CosPlace / EigenPlaces add (csrc/places.hip), each alone against the float64 restatement (tests/places_reference.py), and
single trunk blocks through the forward's own launch code.

New kernels -- the stem with its pool, L2Norm + GeM, Linear + L2Norm: the bar is 3 x the error of the SAME operation in float32 torch on
the CPU against float64 on the same input, computed here (relative to the largest magnitude of the float64 result, floored at half a
float32 ulp of that magnitude, 6e-8), the project's layer rule.

  stem + pool   1x1, 5x7, 32x48, 50x70 and 67x131 (34x66 -> 17x33: tiles of 4 x 8 pooled pixels crossed in both directions, odd Hc and
                Hp) at B = 2, with bn1's shift raised so that every real conv output is positive: then a conv position outside the map
                that is evaluated over the padding would win pool windows.  Three wrong references must miss by orders of magnitude.
  GeM           F = 512 and 2048 at 1, 2, 6, 63, 99 and 768 pixels (chunks of 64 pixels: 99 crosses into a second, 768 fills twelve),
                p = 3 and 2.7, a pixel of all zeros and a channel that is zero everywhere; a row alone against inside B = 3, bitwise.
  head          512 -> 32, 2048 -> 128, 2048 -> 2048 at B = 1, 3, 16: rows bitwise independent of B, unit norm.

Trunk blocks (shared GEMM kernels, K <= 2304 per launch): the project's shared-GEMM bars per launch, 2e-6 exact / 4e-6 split
(tests/test_gpu_gemm_dilated.py), summed over the block's launches.  A block whose 3x3 has K = 4608 (ResNet-18 layer4.1) is measured
and printed, not held to a float64 bar: the shared kernels sum K in one chain (README), and the end-to-end map bar covers it.

Measured on one MI355X: stem + pool 1.1e-07 .. 1.6e-07 (bars 3.7e-07 .. 4.2e-07), the wrong references off by 0.17 .. 0.20 (padding in raw
units), 0.015 .. 0.21 (no Normalize), 0.031 .. 0.073 (out-of-map positions pooled); GeM 1.0e-07 .. 2.2e-07 (bars 2.9e-07 .. 1.4e-06), the
zero channel 9.9999943e-07 .. 1.0000002e-06; head 8.5e-08 .. 1.7e-07 (bars 7.6e-07 .. 1.2e-06); blocks, split / exact: ResNet-18 layer1.0
6.9e-08 / 1.0e-07, layer2.0 2.0e-07 / 2.1e-07, ResNet-50 layer1.0 2.1e-07 / 1.8e-07, layer2.0 3.5e-07 / 3.7e-07 (bars 8e-06 .. 1.6e-05 /
4e-06 .. 8e-06); the K = 4608 block 8.5e-08 / 7.7e-08 (float32 torch on the same input: 3.6e-08)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import places_reference as R
from test_places_cpu import rel, state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ULP_HALF = 6e-8


def _bar(f32, ref):
    """3 x the float32 restatement's own error against float64."""
    return 3 * max(rel(f32, ref), ULP_HALF)


def _backend():
    from imcui_hip import backend

    return backend


@functools.lru_cache(maxsize=None)
def _impl(backbone, dim):
    return _backend().PlacesHIP(backbone, dim)


@functools.lru_cache(maxsize=None)
def _packed(backbone, dim, p=None, stem_shift=0.0):
    """The shared weights packed on the device; p: another GeM exponent; stem_shift: added to bn1's bias."""
    sd = state(backbone, dim)
    if p is not None or stem_shift:
        sd = dict(sd)
        if p is not None:
            sd["aggregation.1.p"] = torch.tensor([p], dtype=torch.float32)
        sd["backbone.1.bias"] = sd["backbone.1.bias"] + stem_shift
    return _backend().pack_places(sd, backbone, dim).to(DEV)


@functools.lru_cache(maxsize=None)
def _net64(backbone, dim):
    return R.build(state(backbone, dim), backbone, dim, torch.float64)


@functools.lru_cache(maxsize=None)
def _net32(backbone, dim):
    return R.build(state(backbone, dim), backbone, dim, torch.float32)


# ------------------------------------------------------------------ stem + pool
STEM_SHIFT = 40.0


def _stem(x, sd, dtype, conv_pad=3, pool_pad=1):
    """conv1 + bn1 (bias raised by STEM_SHIFT) + ReLU + MaxPool2d(3, 2, pool_pad) on an already normalised / padded image, NHWC."""
    t = lambda k: sd[k].to(dtype)  # noqa: E731
    y = F.conv2d(x.to(dtype), t("backbone.0.weight"), stride=2, padding=conv_pad)
    y = F.batch_norm(y, t("backbone.1.running_mean"), t("backbone.1.running_var"), t("backbone.1.weight"), t("backbone.1.bias") + STEM_SHIFT, False, 0.0, 1e-5)
    return y, F.max_pool2d(F.relu(y), 3, 2, pool_pad).permute(0, 2, 3, 1)


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (32, 48), (50, 70), (67, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_stem_and_pool_against_float64(hw):
    be, sd = _backend(), state(18, 32)
    img = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(hw[0] * hw[1]))
    out = _impl(18, 32).layer_probe("stem", img.to(DEV), _packed(18, 32, None, STEM_SHIFT))
    torch.cuda.synchronize()
    (hc, wc), (hp, wp) = be.places_map_size(*hw)[:2]
    pre, ref = _stem(R.normalize_rgb(img, torch.float64), sd, torch.float64)
    _, f32 = _stem(R.normalize_rgb(img, torch.float32), sd, torch.float32)
    assert pre.shape[2:] == (hc, wc) and out.shape == ref.shape == (2, hp, wp, 64)
    assert pre.min().item() > 1.0, "bn1's shift does not keep every real conv output positive: the case cannot tell padding from data"
    # wrong reference 1: the zero padding in RAW units (zeros normalised with the image)
    raw_pad = _stem(R.normalize_rgb(F.pad(img, (3, 3, 3, 3)), torch.float64), sd, torch.float64, conv_pad=0)[1]
    # 2: no Normalize
    no_norm = _stem(img.double(), sd, torch.float64)[1]
    # 3: conv positions -1 and Hc / Wc evaluated over the zero padding and pooled (5 = 3 + 2 zeros around: one more conv position each side)
    wide = _stem(F.pad(R.normalize_rgb(img, torch.float64), (5, 5, 5, 5)), sd, torch.float64, conv_pad=0, pool_pad=0)[1][:, :hp, :wp]
    err, bar = rel(out, ref), _bar(f32, ref)
    wrong = {"padding in raw units": rel(out, raw_pad), "no Normalize": rel(out, no_norm), "out-of-map conv positions pooled": rel(out, wide)}
    print(f"[places-layers] stem + pool {hw} -> {hc}x{wc} -> {hp}x{wp}: err {err:.2e}, bar {bar:.2e}; wrong references: "
          + ", ".join(f"{k} {v:.1e}" for k, v in wrong.items()))  # fmt: skip
    assert not torch.isnan(out).any().item() and err < bar, (err, bar)
    assert all(v > 1e-3 for v in wrong.values()), wrong


# ------------------------------------------------------------------ GeM
@functools.lru_cache(maxsize=None)
def _gem_input(F_, h, w):
    """A post-ReLU map [3, h, w, F] (half zeros) with image 1's first pixel all zero and channel 7 zero everywhere (read-only)."""
    x = torch.relu(torch.randn(3, h, w, F_, generator=torch.Generator().manual_seed(F_ + h * w))) * 3.0
    x[1, 0, 0] = 0.0
    x[..., 7] = 0.0
    return x


@pytest.mark.parametrize("p", [3.0, 2.7], ids=["p3", "p2.7"])
@pytest.mark.parametrize("hw", [(1, 1), (1, 2), (2, 3), (7, 9), (9, 11), (24, 32)], ids=lambda s: f"N{s[0] * s[1]}")
@pytest.mark.parametrize("cfg", [(18, 32), (50, 128)], ids=["F512", "F2048"])
def test_gem_against_float64(cfg, hw, p):
    impl, F_ = _impl(*cfg), 512 if cfg[0] == 18 else 2048
    x = _gem_input(F_, *hw)
    packed = _packed(*cfg, p)
    out = impl.layer_probe("gem", x.to(DEV), packed)
    solo = impl.layer_probe("gem", x[1:2].to(DEV), packed)
    torch.cuda.synchronize()
    xc = x.permute(0, 3, 1, 2)
    ref, f32 = R.gem(xc, p, torch.float64), R.gem(xc, p, torch.float32)
    err, bar = rel(out, ref), _bar(f32, ref)
    print(f"[places-layers] GeM F={F_} N={hw[0] * hw[1]} p={p}: err {err:.2e}, bar {bar:.2e}; zero channel {out[0, 7].item():.7e}")
    assert out.shape == (3, F_) and not torch.isnan(out).any().item()
    assert torch.allclose(out[:, 7].cpu(), torch.full((3,), 1e-6), rtol=1e-5, atol=0), "a channel that is zero everywhere is 1e-6 up to the root"
    assert torch.equal(solo[0], out[1]), "a row's bits depend on the batch it rides in"
    assert err < bar, (err, bar)


# ------------------------------------------------------------------ head
@pytest.mark.parametrize("cfg", [(18, 32), (50, 128), (50, 2048)], ids=["512to32", "2048to128", "2048to2048"])
def test_head_against_float64_and_rows_independent_of_the_batch(cfg):
    impl, sd = _impl(*cfg), state(*cfg)
    F_ = 512 if cfg[0] == 18 else 2048
    g = torch.rand(16, F_, generator=torch.Generator().manual_seed(cfg[1])) * 0.05  # GeM vectors: positive, of a unit vector's entries
    w, b = sd["aggregation.3.weight"], sd["aggregation.3.bias"]
    ref, f32 = R.head(w, b, g, torch.float64), R.head(w, b, g, torch.float32)
    outs = {}
    for B in (1, 3, 16):
        outs[B] = impl.layer_probe("head", g[:B].to(DEV), _packed(*cfg))
        torch.cuda.synchronize()
        err, bar = rel(outs[B], ref[:B]), _bar(f32[:B], ref[:B])
        print(f"[places-layers] head {F_} -> {cfg[1]} B={B}: err {err:.2e}, bar {bar:.2e}")
        assert outs[B].shape == (B, cfg[1]) and err < bar, (B, err, bar)
        assert torch.allclose(outs[B].norm(dim=1).cpu(), torch.ones(B), atol=1e-5)
    assert torch.equal(outs[1][0], outs[16][0]) and torch.equal(outs[3], outs[16][:3]), "a row's bits depend on the batch it rides in"


# ------------------------------------------------------------------ trunk blocks
# (backbone, fc_output_dim, layer, block, input h x w, launches): a stride-1 and a stride-2 BasicBlock, a stride-1 bottleneck with a
# downsample (layer1.0) and a stride-2 bottleneck
BLOCKS = [(18, 32, 1, 0, (8, 12), 2), (18, 32, 2, 0, (7, 9), 3), (50, 128, 1, 0, (8, 12), 4), (50, 128, 2, 0, (13, 18), 4)]


def _block_case(backbone, dim, layer, block, hw):
    blk64, blk32 = _net64(backbone, dim).backbone[3 + layer][block], _net32(backbone, dim).backbone[3 + layer][block]
    cin = blk64.conv1.in_channels
    x = torch.relu(torch.randn(2, cin, *hw, generator=torch.Generator().manual_seed(100 * layer + block + hw[0])))  # as a block leaves it
    with torch.no_grad():
        return x, blk64(x.double()).permute(0, 2, 3, 1), blk32(x.clone()).permute(0, 2, 3, 1), blk64


@pytest.mark.parametrize("case", BLOCKS, ids=lambda c: f"resnet{c[0]}-layer{c[2]}.{c[3]}-{c[4][0]}x{c[4][1]}")
def test_trunk_block_against_float64(case, precision):
    backbone, dim, layer, block, hw, launches = case
    x, ref, f32, blk = _block_case(backbone, dim, layer, block, hw)
    be = _backend()
    be.gemm_route_reset(DEV)
    out = _impl(backbone, dim).layer_probe("block", x.permute(0, 2, 3, 1).contiguous().to(DEV), _packed(backbone, dim), layer, block)
    torch.cuda.synchronize()
    routes = be.gemm_route_counts(DEV)  # every launch of the block is a launch of the shared GEMM, recorded by the launch site itself
    stride = 2 if (block == 0 and layer > 1) else 1
    assert launches == (2 if backbone == 18 else 3) + (blk.downsample is not None) == sum(routes.values()), routes
    assert all(be.gemm_route_name(r).endswith("/conv") for r in routes), routes
    kinds = {be.gemm_route_name(r).split("/")[0] for r in routes}
    assert kinds <= ({"exact"} if precision == 0 else {"conv_128", "conv_256", "wreg_pipe", "wreg_mt2", "wreg_mt1"}), routes
    assert out.shape == ref.shape == (2, (hw[0] - 1) // stride + 1, (hw[1] - 1) // stride + 1, blk.bn3.num_features if backbone != 18 else blk.bn2.num_features)
    err, bar = rel(out, ref), launches * (4e-6 if precision == 1 else 2e-6)
    no_resid = rel(out, torch.relu(ref - (blk.downsample(x.double()) if blk.downsample is not None else x.double()).permute(0, 2, 3, 1)))
    print(f"[places-layers] ResNet-{backbone} layer{layer}.{block} {hw} mode {precision}: err {err:.2e}, bar {bar:.1e} ({launches} launches), "
          f"float32 torch {rel(f32, ref):.2e}; without the shortcut {no_resid:.1e}")  # fmt: skip
    assert not torch.isnan(out).any().item() and no_resid > 1e-3 and err < bar, (err, bar)


def test_long_k_block_is_measured(precision):
    """ResNet-18 layer4.1: two 512 -> 512 3x3 convolutions, K = 4608, each ONE chain in the shared kernels.  Printed for the README;
    held only to the end-to-end bar of 1e-4, which the map comparison of tests/test_gpu_places.py asserts as well."""
    x, ref, f32, _ = _block_case(18, 32, 4, 1, (2, 3))
    out = _impl(18, 32).layer_probe("block", x.permute(0, 2, 3, 1).contiguous().to(DEV), _packed(18, 32), 4, 1)
    torch.cuda.synchronize()
    err = rel(out, ref)
    print(f"[places-layers] ResNet-18 layer4.1 (K = 4608) 2x3 mode {precision}: err {err:.2e} against float64, float32 torch {rel(f32, ref):.2e}")
    assert out.shape == ref.shape and err < 1e-4
