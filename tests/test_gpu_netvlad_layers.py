"""The kernels NetVLAD adds (csrc/netvlad.hip) and the launches it makes that no other case table enters, each alone against float64 torch:
layer 0 with the wrapper's clamp(x * 255, 0, 255) - mean applied as the image is read, conv5_3 (512 -> 512, no ReLU) on a 3 x 4 map, the
NetVLAD layer (pre-normalisation, soft assignment, aggregation, both normalisations) on maps of 1, 6, 63, 257 and 3072 pixels -- with a
pixel of all zeros (the 1e-12 clamp) and a cluster that receives no weight --, and the whitening's split-K skinny GEMM with its fold at
(1024 -> 256) and at the true (32768 -> 4096) for B = 1, 3 and 16, whose rows must not depend on B bit for bit.

Every bar is 3 x the error of the SAME operation in float32 torch on the CPU against float64 on the same input, computed here (relative
to the largest magnitude of the float64 result; floored at half a float32 ulp of that magnitude, 6e-8), as tests/test_gpu_dedode_layers.py
does.  The aggregation forms the residual AS WRITTEN in the reference, sum_n a (x^ - c); it met its bars, so the other form
(sum a x^ - c sum a) was not built.

Measured on one MI355X: layer 0 1.9e-07 (bar 5.8e-07); the NetVLAD layer 1.4e-07 (N = 1), 1.2e-06, 1.4e-06, 1.2e-06, 9.3e-07 (N = 3072)
against bars of 1.3e-06 .. 3.0e-06; the skinny GEMM 8.6e-08 .. 1.5e-07 against bars of 8.5e-07 .. 2.4e-06; conv5_3 3.6e-07 (split) / 3.8e-07 (exact) against 6.8e-07."""
import functools

import pytest
import torch
import torch.nn.functional as F

import netvlad_reference as R
import test_gpu_conv_variants as tc
from test_netvlad_cpu import rel, state

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
def _impl():
    return _backend().NetVLADHIP()


def test_layer0_applies_the_normalisation_as_the_image_is_read():
    """backbone.0 + ReLU on clamp(RGB * 255, 0, 255) - mean with ZERO padding in normalised units (a bias fold would pad with -mean)."""
    be, sd = _backend(), state(False)
    img = torch.rand(2, 3, 13, 19, generator=torch.Generator().manual_seed(13))
    out = _impl().layer_probe("conv0", img.to(DEV), be.pack_netvlad(sd).to(DEV))
    torch.cuda.synchronize()
    w, b, mean = sd["backbone.0.weight"], sd["backbone.0.bias"], sd["preprocess.mean"].view(1, 3, 1, 1)
    layer = lambda x, pad=1: torch.relu(F.conv2d(x, w.to(x.dtype), b.to(x.dtype), padding=pad)).permute(0, 2, 3, 1)  # noqa: E731
    x32 = R.preprocess(sd, img)  # the wrapper's float32 roundings
    ref = layer(x32.double())
    no_mean = layer(torch.clamp(img.double() * 255, 0, 255))
    raw_pad = layer(F.pad(torch.clamp(img.double() * 255, 0, 255), (1, 1, 1, 1)) - mean.double(), pad=0)
    flipped = layer(x32.flip(1).double())
    err, bar = rel(out, ref), _bar(layer(x32), ref)
    print(f"[netvlad-layers] layer 0: err {err:.2e}, bar {bar:.2e}; wrong references: no mean {rel(out, no_mean):.1e}, padding in raw units "
          f"{rel(out, raw_pad):.1e}, BGR {rel(out, flipped):.1e}")  # fmt: skip
    assert out.shape == (2, 13, 19, 64) and err < bar
    assert rel(out, no_mean) > 1e-3 and rel(out, raw_pad) > 1e-3 and rel(out, flipped) > 1e-3


def test_conv5_3_without_relu(precision):
    """conv5_3 as NetVLAD launches it (the probe runs the forward's own launch list in the handle's arithmetic mode): 512 -> 512, K = 4608,
    no activation, a 3 x 4 map (smaller than any tile), the layer's own weights, on a ReLU'd input as conv5_2 leaves it.

    The patch-staging kernels sum K in ONE chain per output (the exact mode is bitwise an fmaf chain).  At K = 4608 a single launch
    measured 1.07e-06 (split) and 1.80e-06 (exact) against this test's bar of 6.83e-07 (3 x torch's float32 error of 2.28e-07), so
    NetVLAD sums its 512-input-channel layers in two levels: 8 launches over 64 input channels each (K = 576), added in group order
    (csrc/netvlad.hip, nv_conv_grouped).  The single-launch figure is printed next to the asserted one."""
    be = _backend()
    B, H, W, C = 2, 3, 4, 512
    x = torch.relu(torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(53)))
    # the layer's own (zero-mean) weights: half of the outputs are negative, so a ReLU'd reference misses
    w, b = state(False)["backbone.28.weight"], state(False)["backbone.28.bias"]
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    got = _impl().layer_probe("conv5_3", xd, be.pack_netvlad(state(False)).to(DEV))
    # the same layer as ONE launch of the shared kernel (measured, not asserted)
    entry = "split" if precision == 1 else "f32"
    wt = be.ConvWeights(w, b, DEV, cout_pad=C)
    buf, one = tc._guarded(B * H * W * C)
    f = dict(entry=entry, inp=xd, out=one, B=B, H=H, W=W, Cin=C, Cout=C, pool=0, relu=0, **wt.fields(entry == "split"))
    if entry == "split":
        f.update(resid=None, resid2=None, cin_stride=0, cout_live=0, single=0)
    be.conv_probe(DEV, **f)
    torch.cuda.synchronize()
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    f32 = F.conv2d(x, w, b, padding=1).permute(0, 2, 3, 1)
    err, bar, relu_err = rel(got, ref), _bar(f32, ref), rel(got, torch.relu(ref))
    print(f"[netvlad-layers] conv5_3 (no ReLU) 3x4 mode {precision}: err {err:.2e}, bar {bar:.2e}; ReLU'd reference {relu_err:.1e}; "
          f"as one launch of the shared kernel {rel(one.view(B, H, W, C), ref):.2e}")  # fmt: skip
    assert got.shape == (B, H, W, C) and not torch.isnan(got).any().item()
    assert relu_err > 1e-3 and err < bar, (err, bar)


@functools.lru_cache(maxsize=None)
def _vlad_state():
    """The shared weights with cluster 5's score row at -50 in every channel: on non-negative maps its score is hundreds below the
    others and its soft-max weight underflows to exactly 0 (the cluster receives no weight; its column is 0 / max(0, 1e-12) = 0)."""
    sd = dict(state(False))
    s = sd["netvlad.score_proj.weight"].clone()
    s[5] = -50.0
    sd["netvlad.score_proj.weight"] = s
    return sd


@functools.lru_cache(maxsize=None)
def _vlad_packed():
    return _backend().pack_netvlad(_vlad_state()).to(DEV)


@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (7, 9), (1, 257), (48, 64)], ids=lambda s: f"N{s[0] * s[1]}")
def test_netvlad_layer_against_float64(hw):
    h, w = hw
    B, sd = 2, _vlad_state()
    x = torch.randn(B, h, w, 512, generator=torch.Generator().manual_seed(h * w)).abs() * 30.0
    x[1, 0, 0] = 0.0  # image 1: a pixel of all zeros (x^ = 0 / 1e-12 = 0, uniform assignment); for N = 1 it is the whole map: V = -c / 64
    out = _impl().layer_probe("vlad", x.to(DEV), _vlad_packed())
    torch.cuda.synchronize()
    d = x.permute(0, 3, 1, 2).reshape(B, 512, h * w)
    ref, a = R.vlad_layer(sd, d, torch.float64, return_assignment=True)
    f32 = R.vlad_layer(sd, d, torch.float32)
    err, bar = rel(out, ref), _bar(f32, ref)
    col5 = out.view(B, 512, 64)[0, :, 5].abs().max().item()  # image 0: no zero pixel, cluster 5 starves
    print(f"[netvlad-layers] NetVLAD layer N={h * w}: err {err:.2e}, bar {bar:.2e}; largest weight of the starved cluster {a[0, 5].max().item():.1e}, "
          f"its column {col5:.1e}")  # fmt: skip
    assert a[0, 5].max().item() < 1e-30 and col5 == 0.0 and a[1, :, 0].min().item() == 1.0 / 64
    assert not torch.isnan(out).any().item() and torch.allclose(out.norm(dim=1).cpu(), torch.ones(B), atol=1e-5)
    assert err < bar, (err, bar)


@functools.lru_cache(maxsize=None)
def _whiten_case(in_dim, out_dim):
    """weight, bias, 16 unit rows and their float64 / float32 results (computed once, read-only)."""
    if (in_dim, out_dim) == (32768, 4096):
        w, b = state(True)["whiten.weight"], state(True)["whiten.bias"]
    else:
        g = torch.Generator().manual_seed(in_dim)
        w, b = torch.randn(out_dim, in_dim, generator=g) / in_dim**0.5, torch.randn(out_dim, generator=g) * 0.01
    x = F.normalize(torch.randn(16, in_dim, generator=torch.Generator().manual_seed(out_dim)), dim=1)
    ref = torch.cat([F.normalize(F.linear(x[i : i + 4].double(), w.double(), b.double()), dim=1) for i in range(0, 16, 4)])
    f32 = F.normalize(F.linear(x, w, b), dim=1)
    return w.to(DEV), b.to(DEV), x, ref, f32


@pytest.mark.parametrize("shape", [(1024, 256), (32768, 4096)], ids=lambda s: f"{s[0]}to{s[1]}")
def test_skinny_gemm_against_float64_and_rows_independent_of_the_batch(shape):
    w, b, x, ref, f32 = _whiten_case(*shape)
    outs = {}
    for B in (1, 3, 16):
        outs[B] = _impl().whiten_probe(w, b, x[:B].to(DEV))
        torch.cuda.synchronize()
        err, bar = rel(outs[B], ref[:B]), _bar(f32[:B], ref[:B])
        print(f"[netvlad-layers] skinny GEMM {shape[0]} -> {shape[1]} B={B}: err {err:.2e}, bar {bar:.2e}")
        assert outs[B].shape == (B, shape[1]) and err < bar, (B, err, bar)
    assert torch.equal(outs[1][0], outs[16][0]) and torch.equal(outs[3], outs[16][:3]), "a row's bits depend on the batch it rides in"
    again = _impl().whiten_probe(w, b, x[:16].to(DEV))
    assert torch.equal(again, outs[16])
