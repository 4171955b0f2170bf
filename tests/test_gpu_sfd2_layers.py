"""The stages SFD2 adds (csrc/sfd2.hip), each alone against the float64 restatement (tests/sfd2_reference.py).

Every bar is 3 x the error of the SAME operation in float32 torch on the CPU against float64 on the same input, computed here (relative
to the largest magnitude of the float64 result, floored at half a float32 ulp of that magnitude: 3 x 6e-8 = 1.8e-07), the project's layer
rule.  A launch that goes through the shared GEMM adds that GEMM's own bar, 2e-6 exact / 4e-6 split (tests/test_gpu_gemm_dilated.py).

  grouped convolution    C = 256 / 32 groups at 1x1, 3x5, 9x18 and 33x70 (crosses the 16 x 16 tile in both directions), B = 2; C = 64 / 8
                         groups at 5x7; with and without ReLU; against float64 F.conv2d(groups=...).  A reference with the groups
                         rotated by one and one with the taps transposed must miss by orders of magnitude; an image alone gives the
                         same bits as inside the batch
  one bottleneck         1x1, grouped 3x3, 1x1 + identity + ReLU through the forward's own launch list at 9x18, both arithmetic modes
  strided layers         conv1b and conv2b, 33x70 -> 17x35 -> 9x18, through the launch list, both modes
  layer 0                with the Normalize, 16x16 / 33x70; a reference padded in raw units and one without the normalisation must miss
  score decode           1x1, 3x5 and 9x18 cells with logits of +-40: values within the bar, the layout c = 4 dy + dx exact (a transposed
                         depth-to-space must miss)
  describe               on given maps at 4x6 and 12x17 cells: key-points at (0, 0), (W - 1, H - 1), exact cell centres, random ones;
                         norms 1 within the bar; rows past the count zero
  crafted score maps     tests/test_sfd2_cpu.py `crafted_cases` through imcui_hip_sfd2_select_probe: count, order, key-points and scores
                         equal the restated rule bit for bit

Measured on one MI355X: grouped convolution 7.0e-08 .. 3.3e-07 (bars 1.8e-07 .. 1.1e-06), rotated groups off by 0.80 .. 1.59, transposed taps
by 0.84 .. 1.53; bottleneck 2.1e-07 split / 2.3e-07 exact (bars 4.7e-06 / 2.7e-06); conv1b 5.6e-07 / 5.9e-07, conv2b 6.2e-07 / 8.6e-07 (bars
4.7e-06 / 2.7e-06); layer 0 2.3e-07 / 2.6e-07 (bars 6.6e-07 / 8.1e-07), padded in raw units off by 0.48, without the normalisation by 0.68 ..
0.70; score decode 8.3e-08 .. 8.6e-08 (bar 2.5e-07), transposed depth-to-space off by 0.99 .. 1.0; describe 3.3e-07 .. 6.7e-07 (bars 9.6e-07 ..
1.9e-06), norms 1 within 8.5e-08.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import sfd2_reference as R
from test_sfd2_cpu import crafted_cases, image, net, state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ULP_HALF = 6e-8
GEMM_BAR = {0: 2e-6, 1: 4e-6}  # exact / split


def rel(a, ref):
    return ((a.double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max().clamp_min(1e-30)).item()


def _bar(f32, ref):
    """3 x the float32 restatement's own error against float64, floored at 1.8e-07."""
    return 3 * max(rel(f32, ref), ULP_HALF)


@functools.lru_cache(maxsize=None)
def _impl():
    from imcui_hip import backend

    packed, cfg = backend.pack_sfd2({k: v for k, v in state().items()})
    return packed.to(DEV), backend.Sfd2HIP(cfg)


def _index(impl, name):
    from imcui_hip import backend

    return [L["name"] for L in backend.sfd2_layers(impl.cfg)].index(name)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------ grouped convolution
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("C,groups,hw", [(256, 32, (1, 1)), (256, 32, (3, 5)), (256, 32, (9, 18)), (256, 32, (33, 70)), (64, 8, (5, 7))])
def test_grouped_convolution(C, groups, hw, relu):
    _, impl = _impl()
    cg = C // groups
    g = torch.Generator().manual_seed(1000 * C + 10 * hw[0] + relu)
    x = torch.randn(2, C, *hw, generator=g)
    w = torch.randn(C, cg, 3, 3, generator=g) / (3.0 * cg**0.5)
    shift = 0.3 * torch.randn(C, generator=g)
    out = impl.gconv_probe(nhwc(x).to(DEV), w, shift.to(DEV), relu)
    solo = impl.gconv_probe(nhwc(x[1:]).to(DEV), w, shift.to(DEV), relu)
    torch.cuda.synchronize()

    def ref_of(x_, w_, s_):
        y = F.conv2d(x_, w_, s_, padding=1, groups=groups)
        return nhwc(F.relu(y) if relu else y)

    ref, f32 = ref_of(x.double(), w.double(), shift.double()), ref_of(x, w, shift)
    rotated = ref_of(x.double(), torch.roll(w.double(), cg, 0), shift.double())  # group g convolved with the weights of group g - 1
    transposed = ref_of(x.double(), w.double().transpose(2, 3), shift.double())
    err, bar = rel(out, ref), _bar(f32, ref)
    miss = (rel(rotated, ref), rel(transposed, ref))
    print(f"grouped 3x3 C={C} groups={groups} map {hw} relu={relu}: {err:.2e} (bar {bar:.2e}); rotated groups miss by {miss[0]:.2e}, transposed taps by {miss[1]:.2e}")
    assert out.shape == ref.shape and err <= bar
    assert torch.equal(out[1], solo[0]), "bits are independent of the batch"
    assert miss[0] > 1000 * bar
    if hw != (1, 1):  # (one pixel reads the centre tap only: the transpose is invisible)
        assert miss[1] > 1000 * bar


# ------------------------------------------------------------------ one bottleneck, the strided layers (the forward's own launch list)
def test_bottleneck(precision):
    packed, impl = _impl()
    first, last = _index(impl, "conv4.1.conv1"), _index(impl, "conv4.1.conv3")
    x = torch.randn(2, 256, 9, 18, generator=torch.Generator().manual_seed(41)).relu()
    out = impl.layers_probe(packed, nhwc(x).to(DEV), first, last)
    torch.cuda.synchronize()
    with torch.no_grad():
        ref, f32 = nhwc(net(double=True).conv4[1](x.double())), nhwc(net().conv4[1](x))
        no_identity = ref - nhwc(x.double())
    err, bar = rel(out, ref), _bar(f32, ref) + GEMM_BAR[precision]
    print(f"bottleneck conv4.1 at 9x18 (precision {precision}): {err:.2e} (bar {bar:.2e}); without the identity off by {rel(no_identity, ref):.2e}")
    assert out.shape == ref.shape and err <= bar and rel(no_identity, ref) > 1000 * bar


def test_strided_layers(precision):
    packed, impl = _impl()
    g = torch.Generator().manual_seed(42)
    for name, cin, hw, hw_out in (("conv1b", 64, (33, 70), (17, 35)), ("conv2b", 128, (17, 35), (9, 18))):
        x = torch.randn(2, cin, *hw, generator=g).relu()
        i = _index(impl, f"{name}.0")
        out = impl.layers_probe(packed, nhwc(x).to(DEV), i, i)
        torch.cuda.synchronize()
        with torch.no_grad():
            ref, f32 = nhwc(getattr(net(double=True), name)(x.double())), nhwc(getattr(net(), name)(x))
        err, bar = rel(out, ref), _bar(f32, ref) + GEMM_BAR[precision]
        print(f"{name} {hw} -> {hw_out} (precision {precision}): {err:.2e} (bar {bar:.2e})")
        assert tuple(out.shape) == (2, *hw_out, cin) and err <= bar


# ------------------------------------------------------------------ layer 0
@pytest.mark.parametrize("hw", [(16, 16), (33, 70)])
def test_layer0_with_normalize(hw):
    packed, impl = _impl()
    img = image(*hw, seed=1, batch=2)
    out = impl.layers_probe(packed, img.to(DEV), 0, 0)
    torch.cuda.synchronize()
    m64, m32 = net(double=True), net()
    d = img.double()
    with torch.no_grad():
        ref, f32 = nhwc(m64.conv1a(R.normalise_image(d))), nhwc(m32.conv1a(R.normalise_image(img)))
        wrong_norm = nhwc(m64.conv1a(d))
        mean, std = torch.tensor(R.MEAN).double().view(1, 3, 1, 1), torch.tensor(R.STD).double().view(1, 3, 1, 1)
        padded_raw = (F.pad(d, (1, 1, 1, 1)) - mean) / std  # the border padded in RAW units
        c = m64.conv1a
        wrong_pad = nhwc(F.relu(c[1](F.conv2d(padded_raw, c[0].weight, c[0].bias))))
    err, bar = rel(out, ref), _bar(f32, ref)
    miss = (rel(wrong_pad, ref), rel(wrong_norm, ref))
    print(f"layer 0 at {hw}: {err:.2e} (bar {bar:.2e}); padded in raw units misses by {miss[0]:.2e}, without the normalisation by {miss[1]:.2e}")
    assert out.shape == ref.shape and err <= bar
    assert min(miss) > 1000 * bar


# ------------------------------------------------------------------ score decode
@pytest.mark.parametrize("cells", [(1, 1), (3, 5), (9, 18)])
def test_score_decode(cells):
    _, impl = _impl()
    g = torch.Generator().manual_seed(50 + cells[0])
    logits = torch.randn(2, 16, *cells, generator=g) * 4
    logits[0, 3, 0, 0], logits[1, 12, -1, -1], logits[0, 0, 0, 0] = 40.0, -40.0, 0.0
    out = impl.score_probe(nhwc(logits).to(DEV))
    torch.cuda.synchronize()
    ref, f32 = R.depth_to_space(torch.sigmoid(logits.double())), R.depth_to_space(R.sigmoid_explicit(logits))
    transposed = R.depth_to_space(torch.sigmoid(logits.double()).view(2, 4, 4, *cells).transpose(1, 2).reshape(2, 16, *cells))
    err, bar = rel(out, ref), _bar(f32, ref)
    print(f"score decode {cells} cells: {err:.2e} (bar {bar:.2e}); transposed depth-to-space off by {rel(transposed, ref):.2e}")
    assert tuple(out.shape) == (2, 4 * cells[0], 4 * cells[1]) and err <= bar and rel(transposed, ref) > 1000 * bar
    # the layout exactly: the +-40 logits and the zero sit where c = 4 dy + dx puts them
    assert out[0, 0, 3].item() == 1.0 and 0.0 < out[1, 4 * cells[0] - 1, 4 * cells[1] - 4].item() < 1e-17 and out[0, 0, 0].item() == 0.5


# ------------------------------------------------------------------ describe
@pytest.mark.parametrize("cells", [(4, 6), (12, 17)])
def test_describe(cells):
    _, impl = _impl()
    h, w = cells
    H, W = 4 * h, 4 * w
    g = torch.Generator().manual_seed(60 + h)
    dmap = torch.randn(2, 128, h, w, generator=g)
    fixed = [(0, 0), (W - 1, H - 1), (W - 1, 0), (0, H - 1)]
    # exact cell centres (4 c + 1.5: between pixels, the probe takes any position) and the pixels on either side of one
    fixed += [(4 * cx + o, 4 * cy + o) for cx, cy, o in ((1, 1, 1.5), (0, 0, 1.5), (w - 1, h - 1, 1.5), (2, 0, 1.5), (1, 1, 1), (1, 1, 2))]
    rnd = torch.stack([torch.randint(0, W, (40,), generator=g), torch.randint(0, H, (40,), generator=g)], dim=1).float()
    kp = torch.cat([torch.tensor(fixed, dtype=torch.float32), rnd])
    K = kp.shape[0] + 3
    kpb = torch.zeros(2, K, 2)
    kpb[0, : kp.shape[0]], kpb[1, : kp.shape[0]] = kp, kp.flip(0)
    counts = torch.tensor([kp.shape[0], 5], dtype=torch.int32)
    out, dn = impl.describe_probe(nhwc(dmap).to(DEV), kpb.to(DEV), counts.to(DEV))
    torch.cuda.synchronize()
    n64, n32 = F.normalize(dmap.double(), dim=1), F.normalize(dmap, dim=1)
    assert rel(dn, nhwc(n64)) <= _bar(nhwc(n32), nhwc(n64))
    for b in range(2):
        n = int(counts[b])
        ref = R.sample_descriptors(kpb[b, :n].double(), n64[b : b + 1])[0].t()
        f32 = R.sample_descriptors(kpb[b, :n], n32[b : b + 1])[0].t()
        err, bar = rel(out[b, :n], ref), _bar(f32, ref)
        norms = (out[b, :n].double().norm(dim=1) - 1).abs().max().item()
        print(f"describe {cells} cells, image {b}: {err:.2e} (bar {bar:.2e}); norms 1 within {norms:.2e}")
        assert err <= bar and norms <= bar
        assert not out[b, n:].any(), "rows past the count are zero"


# ------------------------------------------------------------------ crafted score maps
@pytest.mark.parametrize("name", sorted(crafted_cases()))
def test_crafted_selection(name):
    _, impl = _impl()
    score, size, conf, _ = crafted_cases()[name]
    got = impl.select_probe(score.to(DEV), size, conf)
    torch.cuda.synchronize()
    assert int(got["status"][0]) == 0
    assert torch.equal(got["nms"].cpu(), R.simple_nms(score))
    for b in range(score.shape[0]):
        pix, kp, sc, th = R.select(score[b], size, conf)
        n = int(got["num_keypoints"][b])
        assert n == len(pix), f"{name}: {n} key-points, the rule gives {len(pix)}"
        assert torch.equal(got["keypoints"][b, :n].cpu(), kp) and torch.equal(got["scores"][b, :n].cpu(), sc), name
        assert not got["keypoints"][b, n:].any() and not got["scores"][b, n:].any()
        assert got["threshold"][b].item() == torch.tensor(th, dtype=torch.float32).item()
