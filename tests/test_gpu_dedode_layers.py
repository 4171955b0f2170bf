"""The kernels DeDoDe adds (csrc/dedode.hip), each alone against float64 torch: the depth-wise 5x5 + bias + ReLU (C = 32, 64, 512 on
maps of 4 x 6 -- smaller than the filter and than the 8 x 16 tile --, 5 x 7 and 33 x 70), the bilinear and the bicubic x2 up-sampling,
the per-image soft-max statistics, the separable 51-tap filter (maps narrower than the filter, and 96 x 128) and layer 0 with
transforms.Normalize applied as the image is read.

Every bar is 3 x the error of the SAME operation in float32 torch on the CPU against float64 on the same input, computed here (relative
to the largest magnitude of the float64 result; floored at half a float32 ulp of that magnitude, 6e-8, for operations torch evaluates
exactly).

Measured on one MI355X: depth-wise 8.6e-08 .. 2.5e-07 (bars 3.8e-07 .. 6.0e-07), bilinear x2 7.1e-08 .. 1.1e-07 (bars 1.8e-07 ..
3.1e-07), bicubic x2 1.1e-07 .. 1.3e-07 (bars 1.8e-07 .. 4.6e-07), soft-max statistics 7.6e-09 .. 1.6e-08 (bar 1.8e-07), 51-tap filter
1.1e-07 .. 4.4e-07 (bars 4.1e-07 .. 1.5e-06), layer 0 2.4e-07 / 1.5e-07 (bars 1.0e-06 / 6.1e-07)."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from test_dedode_cpu import image, sds

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ULP_HALF = 6e-8


def _be():
    from imcui_hip import backend

    return backend


def _rel(out, ref):
    return (out.double().cpu() - ref).abs().max().item() / ref.abs().max().item()


def _bar(f32, ref):
    """3 x the float32 restatement's own error against float64."""
    return 3 * max(_rel(f32, ref), ULP_HALF)


@pytest.mark.parametrize("hw", [(4, 6), (5, 7), (33, 70)], ids=["4x6", "5x7", "33x70"])
@pytest.mark.parametrize("C", [32, 64, 512])
def test_depthwise_5x5(C, hw):
    be = _be()
    B, (H, W) = 2, hw
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, 1, 5, 5, generator=g) * 0.2
    b = torch.randn(C, generator=g) * 0.1
    wts = torch.cat([w.reshape(C, 25).t().reshape(-1), b])  # [25 taps][C], then the bias
    out = be.DeDoDeHIP.layer_probe("depthwise", x.permute(0, 2, 3, 1).contiguous().to(DEV), wts)
    torch.cuda.synchronize()
    ref = torch.relu(F.conv2d(x.double(), w.double(), b.double(), padding=2, groups=C)).permute(0, 2, 3, 1)
    f32 = torch.relu(F.conv2d(x, w, b, padding=2, groups=C)).permute(0, 2, 3, 1)
    unpadded = torch.relu(F.conv2d(F.pad(x.double(), (2, 2, 2, 2), mode="replicate"), w.double(), b.double(), groups=C)).permute(0, 2, 3, 1)
    err, bar = _rel(out, ref), _bar(f32, ref)
    print(f"[dedode-layers] depth-wise 5x5 C={C} {H}x{W}: err {err:.2e}, bar {bar:.2e} (replicate-padded reference {_rel(out, unpadded):.1e})")
    assert out.shape == (B, H, W, C) and err < bar and _rel(out, unpadded) > 1e-3


@pytest.mark.parametrize("shape", [(2, 4, 6, 32), (1, 5, 7, 256), (3, 33, 70, 64)], ids=lambda s: "x".join(map(str, s)))
def test_bilinear_x2(shape):
    be = _be()
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[1]))
    out = be.DeDoDeHIP.layer_probe("bilinear2", x.to(DEV))
    torch.cuda.synchronize()
    up = lambda t: F.interpolate(t.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)  # noqa: E731
    ref = up(x.double())
    aligned = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    err, bar = _rel(out, ref), _bar(up(x), ref)
    print(f"[dedode-layers] bilinear x2 {shape}: err {err:.2e}, bar {bar:.2e} (align_corners=True reference {_rel(out, aligned):.1e})")
    assert err < bar and _rel(out, aligned) > 1e-3


@pytest.mark.parametrize("shape", [(2, 4, 6), (1, 5, 7), (3, 33, 70)], ids=lambda s: "x".join(map(str, s)))
def test_bicubic_x2(shape):
    be = _be()
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[1]))
    out = be.DeDoDeHIP.layer_probe("bicubic2", x.to(DEV))
    torch.cuda.synchronize()
    up = lambda t, mode="bicubic": F.interpolate(t[:, None], scale_factor=2, mode=mode, align_corners=False)[:, 0]  # noqa: E731
    ref = up(x.double())
    err, bar = _rel(out, ref), _bar(up(x), ref)
    print(f"[dedode-layers] bicubic x2 {shape}: err {err:.2e}, bar {bar:.2e} (bilinear reference {_rel(out, up(x.double(), 'bilinear')):.1e})")
    assert err < bar and _rel(out, up(x.double(), "bilinear")) > 1e-3


@pytest.mark.parametrize("hw", [(4, 6), (40, 56), (96, 128), (130, 257)], ids=lambda s: "x".join(map(str, s)))
def test_softmax_statistics(hw):
    """(max, log sum exp(l - max)) per image over one chunk, a partial chunk and several chunks of 4096; batch-independent bits."""
    be = _be()
    B = 3
    x = torch.randn(B, *hw, generator=torch.Generator().manual_seed(hw[0])) * 3
    out = be.DeDoDeHIP.layer_probe("softmax_stats", x.to(DEV))
    one = be.DeDoDeHIP.layer_probe("softmax_stats", x[1:2].to(DEV))
    torch.cuda.synchronize()
    flat = x.reshape(B, -1)
    assert torch.equal(out[:, 0].cpu(), flat.max(dim=1).values) and torch.equal(one, out[1:2])
    ref = torch.logsumexp(flat.double(), dim=1)
    f32 = torch.logsumexp(flat, dim=1)
    got = out[:, 0].double().cpu() + out[:, 1].double().cpu()
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    bar = 3 * max((f32.double() - ref).abs().max().item() / ref.abs().max().item(), ULP_HALF)
    print(f"[dedode-layers] soft-max statistics {hw}: err {err:.2e}, bar {bar:.2e}")
    assert err < bar


@pytest.mark.parametrize("hw", [(4, 6), (20, 28), (96, 128)], ids=lambda s: "x".join(map(str, s)))
def test_separable_51_tap_filter(hw):
    be = _be()
    B, (H, W) = 2, hw
    x = torch.rand(B, H, W, generator=torch.Generator().manual_seed(H)) * 5
    taps = be.dedode_density_taps()
    out = be.DeDoDeHIP.layer_probe("filter51", x.to(DEV), taps)
    torch.cuda.synchronize()

    def conv(t):
        w = taps.to(t)[None, None]
        return F.conv2d(F.conv2d(t[:, None], w[..., None, :], padding=(0, 25)), w[..., None], padding=(25, 0))[:, 0]

    ref = conv(x.double())
    w = taps.double()[None, None]
    replicate = F.conv2d(F.conv2d(F.pad(x.double()[:, None], (25, 25, 25, 25), mode="replicate"), w[..., None, :]), w[..., None])[:, 0]
    err, bar = _rel(out, ref), _bar(conv(x), ref)
    print(f"[dedode-layers] 51-tap filter {H}x{W}: err {err:.2e}, bar {bar:.2e} (replicate-padded reference {_rel(out, replicate):.1e})")
    assert err < bar and _rel(out, replicate) > 1e-3


@pytest.mark.parametrize("model", ["detector", "descriptor"])
def test_layer0_applies_normalize_as_the_image_is_read(model):
    """encoder.layers.0 + BatchNorm + ReLU on (x - mean) / std with ZERO padding in normalised units; a reference without the
    normalisation, or with the padding in raw units, must miss."""
    be = _be()
    h, w = 13, 19
    img = torch.cat([image(h, w, seed=1), image(h, w, seed=2)])
    sd = sds()[be.DEDODE_MODELS.index(model)]
    packed, dims = be.pack_dedode(*sds())
    out = be.DeDoDeHIP.layer_probe("conv0", img.to(DEV), packed=packed.to(DEV), dims=dims, model=model)
    torch.cuda.synchronize()
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)

    def layer(x, pad=1):
        y = F.conv2d(x, sd["encoder.layers.0.weight"].to(x), sd["encoder.layers.0.bias"].to(x), padding=pad)
        p = "encoder.layers.1."
        y = F.batch_norm(y, sd[p + "running_mean"].to(x), sd[p + "running_var"].to(x), sd[p + "weight"].to(x), sd[p + "bias"].to(x), False, 0.0, 1e-5)
        return torch.relu(y).permute(0, 2, 3, 1)

    x32 = (img - mean) / std  # transforms.Normalize: two float32 roundings
    ref = layer(x32.double())
    raw = layer(img.double())
    raw_pad = layer((F.pad(img.double(), (1, 1, 1, 1)) - mean.double()) / std.double(), pad=0)
    err, bar = _rel(out, ref), _bar(layer(x32), ref)
    print(f"[dedode-layers] layer 0 ({model}): err {err:.2e}, bar {bar:.2e}; wrong references: no Normalize {_rel(out, raw):.1e}, padding in raw units {_rel(out, raw_pad):.1e}")
    assert err < bar and _rel(out, raw) > 1e-3 and _rel(out, raw_pad) > 1e-3
