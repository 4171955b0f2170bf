"""The launches D2-Net makes that the case tables of tests/test_gpu_conv_variants.py and tests/test_gpu_gemm_dilated.py do not enter at
its shapes, each against float64 torch: the dilation-2 implicit GEMM at K = 4608, N = 512 on a 7 x 11 and an 11 x 16 map, the 64 -> 64
patch-staging convolution pooled (even map) and un-pooled (odd map), layer 0 with the wrapper's normalisation, the flooring max-pool and
the stride-1 average pool.  Bars are those files' own, relative to max |reference|: 2e-6 exact f32, 4e-6 split.

Measured on one MI355X: layer 0 2.1e-07, average pool 7e-08, max-pool exact, the 64 -> 64 launches under their bars, the dilation-2 GEMM
2.6e-07 .. 3.4e-07 in both modes.  With one summation chain over K = 4608 it was 2.0e-06 .. 3.3e-06 in the exact mode (over the bar)
and 1.5e-06 .. 2.0e-06 in the split mode, growing with K whether the taps were dilated or not (7.7e-07 at K = 576, 1.0e-06 .. 1.3e-06
at 1152, 1.5e-06 .. 2.3e-06 at 2304); the dilated instantiations sum K >= 2048 in two levels since (csrc/gemm.hip)."""
from __future__ import annotations

import math

import pytest
import torch
import torch.nn.functional as F

import test_gpu_conv_variants as tc
from test_d2net_cpu import image, sd

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN_F32 = 0x7FC00ABC


def _backend():
    from imcui_hip import backend

    return backend


def _rel(out, ref):
    return (out.double().cpu() - ref).abs().max().item() / ref.abs().max().item()


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("hw", [(7, 11), (11, 16)], ids=["7x11", "11x16"])
def test_dilation2_gemm_at_d2net_shapes(hw, relu, precision):
    """conv4_2 / conv4_3: 512 -> 512, 3x3, dilation 2, padding 2; B = 2, so that M = 154 / 352 rows end in a partial 128-row tile."""
    be = _backend()
    B, (H, W), cin, cout = 2, hw, 512, 512
    g = torch.Generator().manual_seed(1000 + H)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin) + torch.arange(cout).float()[:, None, None, None] * 1e-4
    b = torch.randn(cout, generator=g) * 0.1
    M, ldc = B * H * W, cout + 4
    wt = be.GemmWeights.conv([w], DEV)
    buf = torch.full((M + 3, ldc), NAN_F32, dtype=torch.int32, device=DEV).view(torch.float32)
    route = be.gemm_probe(DEV, epi="conv", A=x.permute(0, 2, 3, 1).contiguous().to(DEV), conv_k=3, conv_stride=1, conv_pad=2, conv_hin=H, conv_win=W,
                          conv_hout=H, conv_wout=W, conv_cin=cin, conv_dil=2, K=9 * cin, M=M, N=cout, C=buf, ldc=ldc, bias=b.to(DEV), act=int(relu),
                          **wt.fields(precision == 1, True))  # fmt: skip
    torch.cuda.synchronize()
    allowed = {be.gemm_route("exact_dil", "conv")} if precision == 0 else {be.gemm_route("convd_128", "conv"), be.gemm_route("convd_256", "conv")}
    assert route in allowed, be.gemm_route_name(route)
    bits = buf.view(torch.int32).cpu()
    written = torch.zeros(bits.shape, dtype=torch.bool)
    written[:M, :cout] = True
    assert (bits[~written] == NAN_F32).all() and not torch.isnan(buf[:M, :cout]).any().item()
    y = F.conv2d(x.double(), w.double(), b.double(), padding=2, dilation=2)
    ref = (torch.relu(y) if relu else y).permute(0, 2, 3, 1).reshape(M, cout)
    undilated = F.conv2d(x.double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(M, cout)
    err, wrong = _rel(buf[:M, :cout], ref), _rel(buf[:M, :cout], torch.relu(undilated) if relu else undilated)
    bar = 2e-6 if precision == 0 else 4e-6
    print(f"[d2net-layers] dilation-2 GEMM {H}x{W} K=4608 N=512 relu={relu} mode {precision} {be.gemm_route_name(route)}: err {err:.2e} (undilated reference {wrong:.1e})")
    assert wrong > 4 * bar and err < bar, (err, bar)


CONV_CASES = [
    tc._s("d2net_c64_unpooled_odd", "split_n2", B=2, H=25, W=35, cin=64, cout=64, act=1, opts={}),
    tc._s("d2net_c64_pooled_even", "split_n2", B=2, H=24, W=34, cin=64, cout=64, act=1, pool=True, opts={}),
    tc._f("d2net_c64_unpooled_odd_f32", B=2, H=25, W=35, cin=64, cout=64, act=1, opts={}),
    tc._f("d2net_c64_pooled_even_f32", B=2, H=24, W=34, cin=64, cout=64, act=1, pool=True, opts={}),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c["id"] for c in CONV_CASES])
def test_conv1_2_launches(case):
    """conv1_2 as D2-Net launches it (default handle options): un-pooled at an odd size, with the fused pool at an even one."""
    tc.run_conv(case)


def test_layer0_applies_the_normalisation_as_the_image_is_read():
    """model.0 + ReLU on flip(RGB) * 255 - mean with ZERO padding in normalised units (a bias fold would pad with -mean)."""
    be = _backend()
    h, w = 13, 19
    img = torch.cat([image(h, w, seed=1), image(h, w, seed=2)])
    packed = be.pack_d2net(sd()).to(DEV)
    out = be.D2NetHIP.layer_probe("conv0", img.to(DEV), packed)
    torch.cuda.synchronize()
    x32 = img.flip(1) * 255 - torch.tensor([103.939, 116.779, 123.68]).view(1, 3, 1, 1)  # the wrapper's two float32 roundings
    wt, bs = sd()["dense_feature_extraction.model.0.weight"].double(), sd()["dense_feature_extraction.model.0.bias"].double()
    ref = torch.relu(F.conv2d(x32.double(), wt, bs, padding=1)).permute(0, 2, 3, 1)
    folded = torch.relu(F.conv2d(F.pad(img.flip(1).double() * 255, (1, 1, 1, 1)) - torch.tensor([103.939, 116.779, 123.68]).double().view(1, 3, 1, 1), wt, bs)).permute(0, 2, 3, 1)
    unflipped = torch.relu(F.conv2d(img.double() * 255 - torch.tensor([103.939, 116.779, 123.68]).double().view(1, 3, 1, 1), wt, bs, padding=1)).permute(0, 2, 3, 1)
    err, e_fold, e_flip = _rel(out, ref), _rel(out, folded), _rel(out, unflipped)
    print(f"[d2net-layers] layer 0: err {err:.2e}; wrong references: padding in raw units {e_fold:.1e}, no BGR flip {e_flip:.1e}")
    assert err < 2e-6 and e_fold > 1e-3 and e_flip > 1e-3


@pytest.mark.parametrize("shape", [(2, 25, 35, 64), (1, 12, 17, 128), (3, 5, 4, 256)], ids=lambda s: "x".join(map(str, s)))
def test_flooring_max_pool_and_stride1_average_pool(shape):
    be = _backend()
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[1]))
    nchw = x.permute(0, 3, 1, 2).double()
    mp = be.D2NetHIP.layer_probe("maxpool", x.to(DEV))
    ap = be.D2NetHIP.layer_probe("avgpool", x.to(DEV))
    torch.cuda.synchronize()
    assert mp.shape == (shape[0], shape[1] // 2, shape[2] // 2, shape[3]) and ap.shape == (shape[0], shape[1] - 1, shape[2] - 1, shape[3])
    assert torch.equal(mp.cpu().double(), F.max_pool2d(nchw, 2, 2).permute(0, 2, 3, 1)), "a maximum is exact"
    err = _rel(ap, F.avg_pool2d(nchw, 2, 1).permute(0, 2, 3, 1))
    print(f"[d2net-layers] pools {shape}: average pool err {err:.2e}")
    assert err < 2e-6
