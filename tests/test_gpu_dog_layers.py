"""The launches csrc/dog.hip adds, each alone against float64 torch (tests/dog_reference.py): pyrdown (blur + bilinear halving) of a
70 x 101 image and of its 35 x 50 level, patch sampling on a 96 x 130 image (levels 0, 1, 2 and the clamped top level; 0, 90 degrees and
odd angles; centres on the corners, so border clamping is exercised) and on a 40 x 56 image where every scale clamps to level 0, both
input normalisations (with a constant patch), layer 1 fused with the normalisation, a stride-1 and a stride-2 implicit-GEMM layer with
patches as the batch dimension, the last layer as eight K groups (one batched launch and its fold) for n = 1, 33 and 257 in both arithmetic modes (rows bitwise independent
of n), and both output normalisations.  The probes read their row counts on the device like the forward, so the same kernel
instantiations run.

Every bar is 3 x the error of the SAME operation in float32 torch on the CPU against float64 on the same input, computed here (relative
to the largest magnitude of the float64 result; floored at half a float32 ulp of that magnitude, 6e-8), as
tests/test_gpu_netvlad_layers.py does.

Measured on one MI355X: pyrdown 4.0e-07 / 2.1e-07 (bars 1.2e-06 / 6.3e-07); sampling 5.2e-06 (bar 1.2e-05) and 1.7e-05 on 40 x 56 (bar
6.2e-05), a negated orientation misses by 0.65, a centre without its + 0.5 by 0.22; the normalisations 2.5e-07 / 2.2e-07 (bars 5.9e-07 /
4.9e-07); layer 1 2.2e-07 / 1.9e-07 (bars 6.1e-07 / 6.5e-07); layers 2 and 3 4.6e-07 / 4.0e-07 split, 4.7e-07 / 4.7e-07 exact (bars
7.5e-07 / 9.3e-07); layer 7 3.0e-07 .. 5.3e-07 split, 4.6e-07 exact (bars 7.9e-07, 1.4e-06, 1.6e-06; with the weight matrix split as it
is read WITHOUT the power-of-two scaling of the packed format the split mode measured 7.87e-07 against 7.90e-07 at n = 1); the output
normalisations 5.4e-08 (bars 2.1e-07 / 3.0e-07)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import dog_reference as R
from test_dog_cpu import NETS, pack, rel, state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ULP_HALF = 6e-8


def _bar(f32, ref):
    """3 x the float32 restatement's own error against float64."""
    return 3 * max(rel(f32, ref), ULP_HALF)


@functools.lru_cache(maxsize=None)
def _impl():
    from imcui_hip import backend

    return backend.PatchDescHIP()


@functools.lru_cache(maxsize=None)
def _packed(name):
    return pack(name).to(DEV)


def texture(h, w, seed):
    """Gray float32 [h,w] in [0,1]: 2x2-averaged noise plus a coarse component (structure at every pyramid level)."""
    g = torch.Generator().manual_seed(seed)
    fine = F.avg_pool2d(torch.rand(1, 1, 2 * h, 2 * w, generator=g), 2)
    coarse = F.interpolate(torch.rand(1, 1, h // 8 + 2, w // 8 + 2, generator=g), size=(h, w), mode="bilinear", align_corners=False)
    return (0.5 * fine + 0.5 * coarse)[0, 0].contiguous()


def test_pyrdown_levels_of_a_70x101_image():
    img = torch.stack([texture(70, 101, 1), texture(70, 101, 2)])
    src = img
    for lev in (1, 2):
        h, w = src.shape[-2:]
        got = _impl().layer_probe("pyrdown", src.to(DEV))
        torch.cuda.synchronize()
        ref, f32 = R.pyrdown(src[:, None].double())[:, 0], R.pyrdown(src[:, None])[:, 0]
        avg = F.avg_pool2d(src[:, None].double(), 2)[:, 0]  # the 2x2 average of the UNBLURRED level
        err, bar = rel(got, ref), _bar(f32, ref)
        print(f"[dog-layers] pyrdown level {lev} ({h}x{w} -> {h // 2}x{w // 2}): err {err:.2e}, bar {bar:.2e}; without the blur {rel(got, avg):.1e}")
        assert got.shape == (2, h // 2, w // 2) and err < bar, (err, bar)
        assert rel(got, avg) > 1e-3
        src = ref.float()  # the next level starts from the float64 level, rounded once


def _sampling_case(h, w, sigmas):
    img = texture(h, w, h)
    centres = [(0.52 * w, 0.47 * h), (0.0, 0.0), (w - 1.0, h - 1.0), (3.2, h - 5.9)]
    angles = [0.0, 90.0, 37.3, -161.2]
    kp, sc, od = [], [], []
    for s in sigmas:
        for a in angles:
            for c in centres:
                kp.append(c), sc.append(s), od.append(a)
    return img, torch.tensor(kp), torch.tensor(sc), torch.tensor(od)


@pytest.mark.parametrize("case", [(96, 130, (1.5, 7.0, 14.0, 60.0), (0, 1, 2, 2)), (40, 56, (1.5, 7.0, 14.0, 60.0), (0, 0, 0, 0))], ids=["96x130", "40x56-level0"])
def test_patch_sampling_against_float64(case):
    h, w, sigmas, want_levels = case
    img, kp, sc, od = _sampling_case(h, w, sigmas)
    got, status = _impl().patch_probe(img.to(DEV), kp.to(DEV), sc.to(DEV), od.to(DEV))
    torch.cuda.synchronize()
    levels, l2 = R.patch_levels(R.lafs_from_keypoints(kp, sc, od, dtype=torch.float64), h, w)
    assert levels.view(len(sigmas), -1).tolist() == [[lv] * 16 for lv in want_levels]
    assert (l2 - l2.round()).abs().min().item() > 1e-3  # no level is in doubt
    ref = R.extract_patches(img[None, None].double(), R.lafs_from_keypoints(kp, sc, od, dtype=torch.float64))[:, 0]
    f32 = R.extract_patches(img[None, None], R.lafs_from_keypoints(kp, sc, od))[:, 0]
    # wrong references: the orientation's sign, and the centre without its + 0.5
    flipped = R.extract_patches(img[None, None].double(), R.lafs_from_keypoints(kp, sc, -od, dtype=torch.float64))[:, 0]
    uncentred = R.extract_patches(img[None, None].double(), R.lafs_from_keypoints(kp - 0.5, sc, od, dtype=torch.float64))[:, 0]
    err, bar = rel(got, ref), _bar(f32, ref)
    print(f"[dog-layers] sampling {h}x{w}: err {err:.2e}, bar {bar:.2e}; negated orientation {rel(got, flipped):.1e}, centre without + 0.5 {rel(got, uncentred):.1e}")
    assert got.shape == (len(kp), 32, 32) and status.item() == 0 and err < bar, (err, bar)
    assert rel(got, flipped) > 1e-2 and rel(got, uncentred) > 1e-3
    # a patch centred on the corner reads clamped pixels: its outer quadrant is the corner pixel itself at level 0, angle 0
    assert torch.equal(got[1, :8, :8].cpu(), torch.full((8, 8), img[0, 0].item()))


def test_a_level_the_pyramid_never_reaches_is_zero_and_non_finite_rows_are_flagged():
    """160 x 200: the clamp allows level 4, kornia's loop stops at level 3 (20 x 25), so such a patch stays zero; a NaN scale sets bit 2."""
    img = texture(160, 200, 3)
    kp = torch.tensor([[100.0, 80.0], [100.0, 80.0], [50.0, 50.0]])
    sc, od = torch.tensor([50.0, 20.0, float("nan")]), torch.zeros(3)
    got, status = _impl().patch_probe(img.to(DEV), kp.to(DEV), sc.to(DEV), od.to(DEV))
    torch.cuda.synchronize()
    lafs = R.lafs_from_keypoints(kp[:2], sc[:2], od[:2], dtype=torch.float64)
    assert R.patch_levels(lafs, 160, 200)[0].tolist() == [4, 2]
    ref = R.extract_patches(img[None, None].double(), lafs)[:, 0]
    assert ref[0].abs().max().item() == 0 and got[0].abs().max().item() == 0 and got[2].abs().max().item() == 0
    assert rel(got[1], ref[1]) < 1e-4 and status.item() == 2


@functools.lru_cache(maxsize=None)
def _patches():
    """33 patches: textures of different contrast and one constant patch (index 7)."""
    g = torch.Generator().manual_seed(33)
    p = torch.rand(33, 32, 32, generator=g) * torch.linspace(0.05, 1.0, 33).view(-1, 1, 1) + 0.1 * torch.rand(33, 1, 1, generator=g)
    p[7] = 0.5
    return p


@pytest.mark.parametrize("name", NETS)
def test_input_normalisation(name):
    net, p = R.build(name, state(name)), _patches()
    got = _impl().layer_probe("norm", p.to(DEV), name)
    torch.cuda.synchronize()
    ref, f32 = net.normalize_input(p[:, None].double())[:, 0], net.normalize_input(p[:, None])[:, 0]
    other = (R.SOSNet if name == "hardnet" else R.HardNet).normalize_input(p[:, None].double())[:, 0]
    err, bar = rel(got, ref), _bar(f32, ref)
    print(f"[dog-layers] {name} input normalisation: err {err:.2e}, bar {bar:.2e}; the other network's rule {rel(got, other):.1e}")
    assert err < bar, (err, bar)
    assert got[7].abs().max().item() == 0 and rel(got, other) > 1e-4


@pytest.mark.parametrize("name", NETS)
def test_layer1_fused_with_the_normalisation(name):
    net, p = R.build(name, state(name)), _patches()
    conv, bn = R.layer_modules(net)[0]
    got = _impl().layer_probe("layer1", p.to(DEV), name, _packed(name))
    torch.cuda.synchronize()

    def layer(x, dt):
        with torch.no_grad():
            return torch.relu(bn.to(dt)(conv.to(dt)(net.normalize_input(x[:, None].to(dt))))).permute(0, 2, 3, 1)

    ref, f32 = layer(p, torch.float64), layer(p, torch.float32)
    err, bar = rel(got, ref), _bar(f32, ref)
    print(f"[dog-layers] {name} layer 1: err {err:.2e}, bar {bar:.2e}")
    assert got.shape == (33, 32, 32, 32) and err < bar, (err, bar)


@pytest.mark.parametrize("layer", [2, 3], ids=["layer2-s1", "layer3-s2"])
def test_gemm_layer_with_patches_as_the_batch(layer, precision):
    """32 -> 32 (stride 1) and 32 -> 64 (stride 2) on 5 patches: 5120 and 1280 GEMM rows, zero padding at every patch's own border."""
    net = R.build("hardnet", state("hardnet"))
    conv, bn = R.layer_modules(net)[layer - 1]
    x = torch.relu(torch.randn(5, 32, 32, 32, generator=torch.Generator().manual_seed(layer)))
    got = _impl().layer_probe(f"layer{layer}", x.permute(0, 2, 3, 1).contiguous().to(DEV), "hardnet", _packed("hardnet"))
    torch.cuda.synchronize()

    def run(dt):
        with torch.no_grad():
            return torch.relu(bn.to(dt)(conv.to(dt)(x.to(dt)))).permute(0, 2, 3, 1)

    ref, f32 = run(torch.float64), run(torch.float32)
    err, bar = rel(got, ref), _bar(f32, ref)
    print(f"[dog-layers] layer {layer} mode {precision}: err {err:.2e}, bar {bar:.2e}")
    assert got.shape == tuple(ref.shape) and err < bar, (err, bar)


@functools.lru_cache(maxsize=None)
def _final_case():
    """257 ReLU'd 8 x 8 x 128 maps and layer 7 + BatchNorm in float64 / float32 (computed once, read-only)."""
    net = R.build("hardnet", state("hardnet"))
    conv, bn = R.layer_modules(net)[6]
    x = torch.relu(torch.randn(257, 128, 8, 8, generator=torch.Generator().manual_seed(257)))
    with torch.no_grad():
        ref = bn.to(torch.float64)(conv.to(torch.float64)(x.double())).view(257, 128)
        f32 = bn.to(torch.float32)(conv.to(torch.float32)(x)).view(257, 128)
        unshifted = conv.to(torch.float64)(x.double()).view(257, 128) / torch.sqrt(bn.running_var.double() + 1e-5)
    return x.permute(0, 2, 3, 1).contiguous(), ref, f32, unshifted


def test_final_gemm_in_k_groups(precision):
    x, ref, f32, unshifted = _final_case()
    outs = {}
    for n in (1, 33, 257):
        outs[n] = _impl().layer_probe("final", x[:n].to(DEV), "hardnet", _packed("hardnet"))
        torch.cuda.synchronize()
        err, bar = rel(outs[n], ref[:n]), _bar(f32[:n], ref[:n])
        print(f"[dog-layers] layer 7 n={n} mode {precision}: err {err:.2e}, bar {bar:.2e}; without the BatchNorm shift {rel(outs[n], unshifted[:n]):.1e}")
        assert outs[n].shape == (n, 128) and err < bar, (n, err, bar)
        assert rel(outs[n], unshifted[:n]) > 1e-3
    assert torch.equal(outs[1][0], outs[257][0]) and torch.equal(outs[33], outs[257][:33]), "a row's bits depend on the rows it rides with"


@pytest.mark.parametrize("name", NETS)
def test_output_normalisation(name):
    x = torch.randn(6, 128, generator=torch.Generator().manual_seed(6)) * torch.tensor([1e-3, 1.0, 30.0, 1.0, 1.0, 1.0]).view(-1, 1)
    x[4] = 0.0
    got = _impl().layer_probe("outnorm", x.to(DEV), name)
    torch.cuda.synchronize()

    def run(dt):
        if name == "hardnet":
            return F.normalize(x.to(dt), dim=1)
        return torch.nn.LocalResponseNorm(256, alpha=256.0, beta=0.5, k=0.0)(x.to(dt).view(6, 128, 1, 1) + 1e-10).view(6, 128)

    ref, f32 = run(torch.float64), run(torch.float32)
    err, bar = rel(got, ref), _bar(f32, ref)
    print(f"[dog-layers] {name} output normalisation: err {err:.2e}, bar {bar:.2e}")
    assert err < bar and torch.isfinite(got).all().item()
    live = [0, 1, 2, 3, 5] if name == "hardnet" else list(range(6))
    assert torch.allclose(got[live].norm(dim=1).cpu(), torch.ones(len(live)), atol=1e-5)
