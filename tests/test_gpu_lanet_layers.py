"""The kernels LANet adds (csrc/lanet.hip), each alone against the float64 restatement (tests/lanet_reference.py).

Every bar is 3 x the error of the SAME operation in float32 torch on the CPU against float64 on the same input, computed here (relative
to the largest magnitude of the float64 result, floored at half a float32 ulp of that magnitude, 6e-8), the project's layer rule.  A
launch that goes through the shared GEMM adds that GEMM's own bar, 2e-6 exact / 4e-6 split (tests/test_gpu_gemm_dilated.py).

  layer 0       conv1a with Normalize at 8x8 and 33x70, B = 2 (VALU kernel); a reference padded in raw units and one without Normalize
                must miss by orders more than the bar.  The LeakyReLU route (padded image + shared GEMM) at 33x70, both arithmetic modes.
  tail + decode 1x1, 3x3, 4x6, 6x8 cells of images that are no multiples of 8: score, level weights and tanh against float64; border
                cells score exactly 0; the coordinate arithmetic applied to the device's OWN tanh values is bit-exact (clamps included:
                a second run saturates the tanh so that the clamps at 0 and W - 1 / H - 1 are hit).
  sparse head   imcui_hip_lanet_desc_probe at k = 1 and 3, with and without bias (and once behind a BatchNorm), on 4x6 / 12x17 / 25x35
                level-2 maps with 1, 31, 32, 33 and 200 key-points: (0, 0), (W - 1, H - 1), exact pixel centres, all weight on one level.
  dense levels  the sparse head equals sampling imcui_hip_lanet_dense_levels' maps (the form the forward never runs) within the
                GEMM's bars, both arithmetic modes.

Measured on one MI355X: layer 0 1.0e-07 / 1.9e-07 (bars 3.7e-07 / 5.5e-07), the wrong references off by 0.93 .. 1.09 (padding in raw units)
and 0.80 .. 0.87 (no Normalize); the LeakyReLU route 2.7e-07 split / 1.9e-07 exact (bars 4.6e-06 / 2.6e-06); tail + decode: score at most
1.3e-07 (bars 1.8e-07 .. 1.2e-06), level weights 1.1e-07 (bars 2.0e-07 .. 3.7e-07), tanh 8.5e-07 with the saturating inputs (bars 3.0e-07
.. 3.6e-06), coordinates bit-exact, every clamp hit; the sparse head 1.0e-07 .. 7.3e-07 over its 75 cases (bars 3.3e-07 .. 1.9e-06), 2.8e-07
with 32-channel chunks; the dense level maps 2.2e-07 .. 8.6e-07 and the sparse head against their samples 2.4e-07 .. 6.6e-07 (bars
2.5e-06 .. 5.2e-06).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import lanet_reference as R
from test_lanet_cpu import image, lib_state, net, probe_points, state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ULP_HALF = 6e-8
GEMM_BAR = {0: 2e-6, 1: 4e-6}  # exact / split


def rel(a, ref):
    return ((a.double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max().clamp_min(1e-30)).item()


def _bar(f32, ref):
    """3 x the float32 restatement's own error against float64."""
    return 3 * max(rel(f32, ref), ULP_HALF)


def _backend():
    from imcui_hip import backend

    return backend


@functools.lru_cache(maxsize=None)
def _packed(k=3, bias=True, bn=False, activation="relu", widths=R.WIDTHS):
    packed, cfg = _backend().pack_lanet(lib_state(state(0, k, bias, bn, widths)), activation)
    return packed.to(DEV), _backend().LanetHIP(cfg)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------ layer 0
@pytest.mark.parametrize("hw", [(8, 8), (33, 70)])
def test_layer0_with_normalize(hw):
    packed, impl = _packed()
    img = image(*hw, seed=1, batch=2)
    got = impl.stem_probe(packed, img.to(DEV))
    with torch.no_grad():
        ref = nhwc(net(double=True).parts(img.double())["x1a"])
        f32 = nhwc(net().parts(img)["x1a"])
        m = net(double=True).interestpoint_module
        raw_pad = (F.pad(img.double(), (1, 1, 1, 1)) - R.MEAN) / R.STD  # the border padded in RAW units: -0.5 / 0.225 after Normalize
        wrong_pad = nhwc(F.relu(m.bn1a(F.conv2d(raw_pad, m.conv1a.weight))))
        wrong_norm = nhwc(F.relu(m.bn1a(m.conv1a(img.double()))))
    err, bar = rel(got, ref), _bar(f32, ref)
    miss = (rel(wrong_pad, ref), rel(wrong_norm, ref))
    print(f"layer 0 at {hw}: {err:.2e} (bar {bar:.2e}); padded in raw units misses by {miss[0]:.2e}, without Normalize by {miss[1]:.2e}")
    assert got.shape == ref.shape and err <= bar
    assert min(miss) > 1000 * bar


def test_layer0_leaky_route_on_the_shared_gemm(precision):
    packed, impl = _packed(activation="leaky_relu")
    img = image(33, 70, seed=1, batch=2)
    got = impl.stem_probe(packed, img.to(DEV))
    with torch.no_grad():
        ref = nhwc(net(double=True, leaky=True).parts(img.double())["x1a"])
        f32 = nhwc(net(leaky=True).parts(img)["x1a"])
    err, bar = rel(got, ref), _bar(f32, ref) + GEMM_BAR[precision]
    print(f"layer 0, LeakyReLU on the GEMM, precision {precision}: {err:.2e} (bar {bar:.2e}); negative outputs {(got < 0).float().mean().item():.2f}")
    assert err <= bar and bool((got < 0).any())


# ------------------------------------------------------------------ head tail + decode
@pytest.mark.parametrize("hw", [(8, 8), (29, 30), (37, 53), (50, 70)])
@pytest.mark.parametrize("saturate", [False, True])
def test_tail_and_decode(hw, saturate):
    H, W = hw
    Hc, Wc = H // 8, W // 8
    packed, impl = _packed()
    g = torch.Generator().manual_seed(7 + H)
    s1 = F.relu(torch.randn(2, 256, Hc, Wc, generator=g))
    p1 = F.relu(torch.randn(2, 256, Hc, Wc, generator=g)) * (60.0 if saturate else 1.0)
    got = impl.tail_probe(packed, nhwc(s1).to(DEV), nhwc(p1).to(DEV), H, W)
    torch.cuda.synchronize()
    with torch.no_grad():
        m64, m32 = net(double=True).interestpoint_module, net().interestpoint_module
        ref = R.decode(m64.convDb(s1.double()), m64.convPb(p1.double()), H, W)
        f32 = R.decode(m32.convDb(s1), m32.convPb(p1), H, W)
    score = got["cell_score"].cpu().view(2, 1, Hc, Wc)
    aware = got["cell_aware"].cpu().view(2, Hc, Wc, 3).permute(0, 3, 1, 2)
    tanh = got["cell_tanh"].cpu().view(2, Hc, Wc, 2).permute(0, 3, 1, 2).contiguous()
    coord = got["cell_coord"].cpu().view(2, Hc, Wc, 2).permute(0, 3, 1, 2)
    for name, a, i in (("score", score, 0), ("aware", aware, 2), ("tanh", tanh, 3)):
        err, bar = rel(a, ref[i]), _bar(f32[i], ref[i])
        print(f"{hw} saturate={saturate} {name}: {err:.2e} (bar {bar:.2e})")
        if name != "score" or Hc > 2 and Wc > 2:  # (all-border maps: the score is exactly 0 everywhere, checked below)
            assert err <= bar, name
    border = torch.ones(Hc, Wc, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert bool((score[:, 0][:, border] == 0).all()), "border cells score exactly 0"
    if Hc > 2 and Wc > 2:
        assert bool((score[:, 0][:, ~border] > 0).all())
    # the coordinate arithmetic on the device's own tanh values, bit for bit
    assert torch.equal(coord, R.coord_from_tanh(tanh, H, W))
    assert coord[:, 0].min() >= 0 and coord[:, 0].max() <= W - 1 and coord[:, 1].min() >= 0 and coord[:, 1].max() <= H - 1
    if saturate:
        hit = [bool((coord[:, 0] == 0).any()), bool((coord[:, 0] == W - 1).any()), bool((coord[:, 1] == 0).any()), bool((coord[:, 1] == H - 1).any())]
        print(f"{hw}: clamps hit (x = 0, x = W - 1, y = 0, y = H - 1): {hit}")
        assert any(hit[:2]) and any(hit[2:])


# ------------------------------------------------------------------ the sparse level-aware head
def _levels(h, w, seed, c2=64, c3=128):
    """Seeded level maps of one image (NCHW, ReLU-like), the image size they belong to and 200 positions with their level weights."""
    g = torch.Generator().manual_seed(seed)
    H, W = 2 * h + 1, 2 * w + 1
    x2 = F.relu(torch.randn(1, c2, h, w, generator=g))
    x3 = F.relu(torch.randn(1, c3, max(h // 2, 1), max(w // 2, 1), generator=g))
    x4 = F.relu(torch.randn(1, 256, max(h // 4, 1), max(w // 4, 1), generator=g))
    pts = probe_points(W, H, 200, seed)
    centres = torch.tensor([[(j + 0.5) * (W - 1) / w, (i + 0.5) * (H - 1) / h] for i, j in ((0, 0), (h - 1, w - 1), (1, 2), (h // 2, w // 2))])
    pts[8:12] = centres  # exact pixel centres of the level-2 map (up to the float32 rounding of the normalisation)
    aware = torch.softmax(torch.randn(200, 3, generator=g), dim=1)
    aware[12:15] = torch.eye(3)  # all weight on one level
    aware[0] = torch.tensor([1.0, 0.0, 0.0])  # ... at (0, 0)
    return H, W, x2, x3, x4, pts, aware


def _dense_desc(m, x2, x3, x4, pts, aware, H, W, d23=None):
    """Convolve-then-sample in the dtype of the inputs: [n,256]."""
    grid = R.normalised_grid(pts, H, W).view(1, 1, -1, 2)
    d2, d3 = m.level_maps(x2, x3) if d23 is None else d23
    return R.blend_levels(d2, d3, x4, grid, aware.t().reshape(1, 3, 1, -1))[0, :, 0].t()


@pytest.mark.parametrize("k,bias,bn", [(3, True, False), (3, False, False), (1, True, False), (1, False, False), (3, True, True)])
@pytest.mark.parametrize("hw", [(4, 6), (12, 17), (25, 35)])
def test_sparse_head_against_float64(k, bias, bn, hw):
    packed, impl = _packed(k, bias, bn)
    H, W, x2, x3, x4, pts, aware = _levels(*hw, seed=11)
    m64, m32 = net(0, k, bias, bn, True).interestpoint_module, net(0, k, bias, bn).interestpoint_module
    dx = [nhwc(t)[0].to(DEV) for t in (x2, x3, x4)]
    for n in (1, 31, 32, 33, 200):
        got = impl.desc_probe(packed, *dx, H, W, pts[:n].to(DEV), aware[:n].to(DEV))
        with torch.no_grad():
            ref = _dense_desc(m64, x2.double(), x3.double(), x4.double(), pts[:n].double(), aware[:n].double(), H, W)
            f32 = _dense_desc(m32, x2, x3, x4, pts[:n], aware[:n], H, W)
        err, bar = rel(got, ref), _bar(f32, ref)
        norm = (got.double().norm(dim=1) - 1).abs().max().item()
        print(f"sparse head k={k} bias={bias} bn={bn} map {hw} n={n}: {err:.2e} (bar {bar:.2e}), |norm - 1| {norm:.1e}")
        assert got.shape == (n, 256) and err <= bar and norm < 1e-5


def test_sparse_head_with_widths_that_are_no_multiple_of_64():
    """c2 = 96, c3 = 160: the head stages 32 channels per chunk instead of 64."""
    widths = (32, 96, 160, 256)
    packed, impl = _packed(3, True, False, widths=widths)
    H, W, x2, x3, x4, pts, aware = _levels(12, 17, seed=13, c2=96, c3=160)
    m64, m32 = net(0, 3, True, False, True, widths=widths).interestpoint_module, net(0, 3, True, False, widths=widths).interestpoint_module
    got = impl.desc_probe(packed, *[nhwc(t)[0].to(DEV) for t in (x2, x3, x4)], H, W, pts.to(DEV), aware.to(DEV))
    with torch.no_grad():
        ref = _dense_desc(m64, x2.double(), x3.double(), x4.double(), pts.double(), aware.double(), H, W)
        f32 = _dense_desc(m32, x2, x3, x4, pts, aware, H, W)
    err, bar = rel(got, ref), _bar(f32, ref)
    print(f"sparse head, widths {widths}: {err:.2e} (bar {bar:.2e})")
    assert err <= bar


@pytest.mark.parametrize("k", [1, 3])
def test_sparse_head_equals_sampling_the_dense_levels(k, precision):
    packed, impl = _packed(k, True, False)
    H, W, x2, x3, x4, pts, aware = _levels(12, 17, seed=12)
    m64, m32 = net(0, k, True, False, True).interestpoint_module, net(0, k, True, False).interestpoint_module
    sparse = impl.desc_probe(packed, *[nhwc(t)[0].to(DEV) for t in (x2, x3, x4)], H, W, pts.to(DEV), aware.to(DEV))
    d2, d3 = impl.dense_levels(packed, nhwc(x2).to(DEV), nhwc(x3).to(DEV))
    with torch.no_grad():
        ref2, ref3 = m64.level_maps(x2.double(), x3.double())
        f2, f3 = m32.level_maps(x2, x3)
        d2c, d3c = d2.cpu().permute(0, 3, 1, 2), d3.cpu().permute(0, 3, 1, 2)
        e2, e3 = rel(d2c, ref2), rel(d3c, ref3)
        b2, b3 = _bar(f2, ref2) + GEMM_BAR[precision], _bar(f3, ref3) + GEMM_BAR[precision]
        dense = _dense_desc(m64, x2.double(), x3.double(), x4.double(), pts.double(), aware.double(), H, W, (d2c.double(), d3c.double()))
        ref = _dense_desc(m64, x2.double(), x3.double(), x4.double(), pts.double(), aware.double(), H, W)
        f32 = _dense_desc(m32, x2, x3, x4, pts, aware, H, W)
    err, bar = rel(sparse, dense), _bar(f32, ref) + GEMM_BAR[precision]
    print(f"k={k} precision {precision}: dense des_conv2 {e2:.2e} (bar {b2:.2e}), des_conv3 {e3:.2e} (bar {b3:.2e}); sparse head against the sampled dense maps {err:.2e} (bar {bar:.2e})")
    assert e2 <= b2 and e3 <= b3 and err <= bar
