"""The stages LiftFeat adds (csrc/liftfeat.hip), each alone against the float64 restatement (tests/liftfeat_reference.py).

Every bar is 3 x the error of the SAME operation in float32 torch on the CPU against float64 on the same input, computed here (relative
to the largest magnitude of the float64 result, floored at half a float32 ulp of that magnitude: 3 x 6e-8 = 1.8e-07), the project's layer
rule.  None of these stages goes through the shared GEMM (the token network runs on v_mfma_f32_32x32x2_f32 in both arithmetic modes), so no
GEMM bar is added.

  input stage     32x48 (no pad), 50x70 (64x96) and 33x33 (64x64), B = 2: the pad is zero, mean and invstd against float64; statistics over
                  the real pixels only must miss by orders of magnitude
  up-conv stages  each of the three on 1x1, 3x5 and 9x13 maps, B = 2; a reference with align_corners=False must miss (not at 1x1, where
                  both rules copy the one pixel); the fused last stage at 4x4, 4x8 and 12x20: values, the layout c * 64 + dy * 8 + dx
                  (a transposed layout must miss), a pixel whose three values are zero gives zeros
  booster         N = 1, 31, 32, 33 and 200 tokens, with and without kenc: the encoders' sum and the boosted rows
  AFT layer       N = 1 (kv = v), 24, 33 (one chunk + 1), 70 (two chunks + a partial one), crafted inputs (k = +80 / -80, a channel with
                  all k equal, a constant row); B = 2 with different images; an image alone against inside the batch bitwise
  selection       tests/test_liftfeat_cpu.py `crafted_cases` through imcui_hip_liftfeat_select_probe: count, order, key-points and scores
                  equal the restated rule bit for bit; a constant map sets status bit 1 and the retry succeeds
  launch gate     the forward in each arithmetic mode under the route recorder: every (route, feature) pair of the shared GEMM it launches
                  is one tests/test_gpu_gemm_variants.py checks against float64; no launch of the 3x3 convolution kernels or the fused FFN

Measured on one MI355X: input stage (invstd, -mean invstd) 2.9e-08 .. 4.0e-08 (bars 1.8e-07 .. 1.9e-07), statistics over the real pixels off
by 0.55 .. 0.67; up-conv stages 2.9e-07 .. 1.3e-06 (bars 4.2e-07 .. 2.4e-06), align_corners=False off by 0.22 .. 0.41; fused last stage
7.7e-07 .. 7.2e-06 (bars 2.6e-06 .. 6.2e-05), transposed layout off by 1.8 .. 1.9; booster encoders 1.2e-07 .. 1.8e-07 (bars 2.4e-07 ..
5.4e-07), boosted rows 3.7e-07 .. 5.5e-07 (bars 8.9e-07 .. 1.8e-06); AFT layer 2.0e-07 .. 2.9e-07 (bars 4.6e-07 .. 8.3e-07), kv 1.4e-07 ..
5.5e-07 (bars 3.2e-07 .. 1.1e-06), crafted 1.3e-07 / kv 3.7e-07 (bars 3.2e-07 / 1.2e-06); crafted selection bit for bit; 19 shared-GEMM
launches per mode, every (route, feature) pair covered.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import liftfeat_reference as R
from test_liftfeat_cpu import crafted_boosted, crafted_cases, image, net, restated_selection, state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ULP_HALF = 6e-8


def rel(a, ref):
    return ((a.double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max().clamp_min(1e-30)).item()


def _bar(f32, ref):
    """3 x the float32 restatement's own error against float64, floored at 1.8e-07."""
    return 3 * max(rel(f32, ref), ULP_HALF)


@functools.lru_cache(maxsize=None)
def _impl(kenc=True):
    from imcui_hip import backend

    packed, cfg = backend.pack_liftfeat(dict(state(kenc=kenc) if not kenc else state()))
    return packed.to(DEV), backend.LiftFeatHIP(cfg)


def _net(double, kenc=True):
    return net(double) if kenc else net(double, kenc=False)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------ input stage
@pytest.mark.parametrize("hw", [(32, 48), (50, 70), (33, 33)])
def test_input_stage(hw):
    _, impl = _impl()
    img = image(*hw, seed=2, batch=2)
    gray, norm = impl.input_probe(img.to(DEV))
    torch.cuda.synchronize()
    H, W = hw
    Hp, Wp = gray.shape[-2:]
    assert (Hp, Wp) == ((H + 31) // 32 * 32, (W + 31) // 32 * 32)
    assert not gray[:, H:].any() and not gray[:, :, W:].any(), "the pad is zero"

    def stats(x):  # [B,3,H,W] in x's dtype -> gray, (invstd, -mean * invstd) over the PADDED image
        g = F.pad(((x * 255) / 255).mean(dim=1), (0, Wp - W, 0, Hp - H))
        mean, var = g.mean(dim=(1, 2)), g.var(dim=(1, 2), unbiased=False)
        inv = 1 / torch.sqrt(var + 1e-5)
        return g, torch.stack([inv, -mean * inv], dim=1)

    g64, n64 = stats(img.double())
    g32, n32 = stats(img)
    real = ((img.double() * 255) / 255).mean(dim=1)
    inv_r = 1 / torch.sqrt(real.var(dim=(1, 2), unbiased=False) + 1e-5)
    n_real = torch.stack([inv_r, -real.mean(dim=(1, 2)) * inv_r], dim=1)
    eg, en, bar = rel(gray, g64), rel(norm, n64), _bar(n32, n64)
    miss = rel(n_real, n64)
    print(f"input stage {hw} -> {Hp}x{Wp}: gray {eg:.2e}, (invstd, -mean invstd) {en:.2e} (bar {bar:.2e}); statistics over the real pixels miss by {miss:.2e}")
    assert eg <= _bar(g32, g64) and en <= bar
    if (Hp, Wp) != hw:
        assert miss > 1000 * bar


# ------------------------------------------------------------------ up-conv stages
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (9, 13)])
@pytest.mark.parametrize("stage", [0, 1, 2])
def test_upconv_stage(stage, hw):
    packed, impl = _impl()
    cin = (64, 32, 16)[stage]
    x = torch.randn(2, cin, *hw, generator=torch.Generator().manual_seed(10 * stage + hw[0]))
    out = impl.upconv_probe(packed, nhwc(x).to(DEV), stage)
    solo = impl.upconv_probe(packed, nhwc(x[1:]).to(DEV), stage)
    torch.cuda.synchronize()
    with torch.no_grad():
        ref, f32 = nhwc(net(True).normal_head[stage](x.double())), nhwc(net().normal_head[stage](x))
        wrong = nhwc(net(True).normal_head[stage](x.double(), align_corners=False))
    err, bar, miss = rel(out, ref), _bar(f32, ref), rel(wrong, ref)
    print(f"up-conv stage {stage} ({cin} -> {cin // 2}) on {hw}: {err:.2e} (bar {bar:.2e}); align_corners=False misses by {miss:.2e}")
    assert out.shape == ref.shape and err <= bar
    assert torch.equal(out[1], solo[0]), "bits are independent of the batch"
    if hw != (1, 1):
        assert miss > 1000 * bar


@pytest.mark.parametrize("hw", [(4, 4), (4, 8), (12, 20)])
def test_upconv_fused_last_stage(hw):
    packed, impl = _impl()
    x = torch.randn(2, 16, *hw, generator=torch.Generator().manual_seed(30 + hw[1]))
    out = impl.upconv_probe(packed, nhwc(x).to(DEV), 2, fused=True)
    torch.cuda.synchronize()

    def ref_of(m, x_):
        with torch.no_grad():
            return F.normalize(m.normal_head[3](m.normal_head[2](x_)), dim=1, eps=1e-12)  # D1 [B,3,2h,2w]

    d64, d32 = ref_of(net(True), x.double()), ref_of(net(), x)
    ref, f32 = nhwc(R.X.unfold8(d64)), nhwc(R.X.unfold8(d32))
    u = R.X.unfold8(d64)
    transposed = nhwc(u.view(2, 3, 8, 8, *u.shape[2:]).transpose(2, 3).reshape(u.shape))  # channel c * 64 + dx * 8 + dy
    err, bar = rel(out, ref), _bar(f32, ref)
    miss = rel(transposed, ref)
    print(f"fused last stage on {hw}: {err:.2e} (bar {bar:.2e}); transposed layout misses by {miss:.2e}")
    assert out.shape == ref.shape and err <= bar and miss > 1000 * bar
    # the layout exactly: folding the device's output back gives unit vectors at every pixel
    B, h8, w8, _ = out.shape
    d = out.cpu().reshape(B, h8, w8, 3, 8, 8).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 8 * h8, 8 * w8)
    assert rel(d, d64) <= bar and (d.double().norm(dim=1) - 1).abs().max().item() <= bar


def test_upconv_fused_zero_pixel_gives_zeros():
    """Weights that make every pre-normalisation value zero: x / max(|x|, 1e-12) is 0, not NaN."""
    from imcui_hip import backend

    sd = dict(state())
    sd["normal_head.3.weight"] = torch.zeros_like(sd["normal_head.3.weight"])
    sd["normal_head.3.bias"] = torch.zeros_like(sd["normal_head.3.bias"])
    packed, cfg = backend.pack_liftfeat(sd)
    x = torch.randn(1, 4, 4, 16, generator=torch.Generator().manual_seed(5))
    out = backend.LiftFeatHIP(cfg).upconv_probe(packed.to(DEV), x.to(DEV), 2, fused=True)
    torch.cuda.synchronize()
    assert out.shape == (1, 1, 1, 192) and not out.any() and torch.isfinite(out).all()


# ------------------------------------------------------------------ booster
def _tokens(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, 64, generator=g), torch.randn(B, N, 65, generator=g), F.normalize(torch.randn(B, N, 3, 64, generator=g), dim=2).reshape(B, N, 192)


@pytest.mark.parametrize("kenc", [True, False], ids=["kenc", "no-kenc"])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 200])
def test_booster(N, kenc):
    packed, impl = _impl(kenc)
    d, k, n = _tokens(2, N, 400 + N)
    out, xe = impl.booster_probe(packed, d.to(DEV), k.to(DEV), n.to(DEV))
    torch.cuda.synchronize()

    def ref_of(m, d_, k_, n_):
        fb = m.feature_boost
        with torch.no_grad():
            enc = torch.stack([fb.encode(d_[b], k_[b], n_[b]) for b in range(2)])
            return enc, torch.stack([F.normalize(fb(d_[b], k_[b], n_[b]), dim=1, eps=1e-12) for b in range(2)])

    e64, r64 = ref_of(_net(True, kenc), d.double(), k.double(), n.double())
    e32, r32 = ref_of(_net(False, kenc), d, k, n)
    err_e, bar_e, err, bar = rel(xe, e64), _bar(e32, e64), rel(out, r64), _bar(r32, r64)
    print(f"booster N={N} kenc={kenc}: encoders {err_e:.2e} (bar {bar_e:.2e}), boosted rows {err:.2e} (bar {bar:.2e})")
    assert err_e <= bar_e and err <= bar
    assert (out.double().norm(dim=2) - 1).abs().max().item() <= bar


# ------------------------------------------------------------------ one AFT layer
def _aft_ref(m, layer, x):
    L = m.feature_boost.layers[layer]
    with torch.no_grad():
        return torch.stack([L(x[b]) for b in range(x.shape[0])]), torch.stack([L.attn.kv(x[b]) for b in range(x.shape[0])])


@pytest.mark.parametrize("N", [1, 24, 33, 70])
@pytest.mark.parametrize("layer", [0, 2])
def test_aft_layer(layer, N):
    packed, impl = _impl()
    x = torch.randn(2, N, 64, generator=torch.Generator().manual_seed(500 + N + layer))
    out, kv = impl.aft_probe(packed, x.to(DEV), layer)
    solo, _ = impl.aft_probe(packed, x[1:].to(DEV), layer)
    torch.cuda.synchronize()
    r64, kv64 = _aft_ref(net(True), layer, x.double())
    r32, kv32 = _aft_ref(net(), layer, x)
    err, bar, ekv, bkv = rel(out, r64), _bar(r32, r64), rel(kv, kv64), _bar(kv32, kv64)
    print(f"AFT layer {layer} N={N}: {err:.2e} (bar {bar:.2e}), kv {ekv:.2e} (bar {bkv:.2e})")
    assert err <= bar and ekv <= bkv
    assert torch.equal(out[1], solo[0]), "an image alone and inside the batch: the same bits"
    assert not torch.equal(out[0], out[1])
    if N == 1:  # one token: the soft-max is 1 and kv = v
        with torch.no_grad():
            v64 = net(True).feature_boost.layers[layer].attn.v(x.double())[:, 0]
        assert rel(kv, v64) <= bkv


def test_aft_layer_crafted():
    """k = +80 on one token and -80 on another (exp stays finite after the max is taken out), a channel whose k is equal on every token
    (kv = the mean of v), and a constant input row with the output projection zeroed, so that the first LayerNorm sees variance 0."""
    from imcui_hip import backend

    sd = dict(state())
    p = "feature_boost.layers.0.attn.k"
    wk, bk = sd[f"{p}.weight"].clone(), sd[f"{p}.bias"].clone()
    wk[5] = 0.0  # channel 5: k = bias on every token
    wk[7] = 0.0
    wk[7, 0] = 1.0  # channel 7: k = x[:, 0]
    bk[7] = 0.0
    sd[f"{p}.weight"], sd[f"{p}.bias"] = wk, bk
    for t in ("weight", "bias"):  # no attention output: the constant row reaches the first LayerNorm as it is
        sd[f"feature_boost.layers.0.attn.proj.{t}"] = torch.zeros_like(sd[f"feature_boost.layers.0.attn.proj.{t}"])
    packed, cfg = backend.pack_liftfeat(sd)
    impl = backend.LiftFeatHIP(cfg)
    N = 40
    x = torch.randn(1, N, 64, generator=torch.Generator().manual_seed(9))
    x[0, 3, 0], x[0, 35, 0] = 80.0, -80.0
    x[0, 10] = 0.25
    out, kv = impl.aft_probe(packed.to(DEV), x.to(DEV), 0)
    torch.cuda.synchronize()
    m64, m32 = R.load_model(sd).double(), R.load_model(sd)
    r64, kv64 = _aft_ref(m64, 0, x.double())
    r32, kv32 = _aft_ref(m32, 0, x)
    err, bar, ekv, bkv = rel(out, r64), _bar(r32, r64), rel(kv, kv64), _bar(kv32, kv64)
    print(f"AFT layer crafted: {err:.2e} (bar {bar:.2e}), kv {ekv:.2e} (bar {bkv:.2e})")
    assert torch.isfinite(out).all() and torch.isfinite(kv).all()
    assert err <= bar and ekv <= bkv
    with torch.no_grad():
        v64 = m64.feature_boost.layers[0].attn.v(x[0].double())
    assert abs(kv[0, 5].item() - v64[:, 5].mean().item()) <= bkv * kv64.abs().max().item()  # equal k: the mean of v
    assert abs(kv[0, 7].item() - v64[3, 7].item()) <= bkv * kv64.abs().max().item()  # k = +80 takes all the weight


# ------------------------------------------------------------------ crafted heat maps
@pytest.mark.parametrize("name", sorted(crafted_cases()))
def test_crafted_selection(name):
    _, impl = _impl()
    heat, H, W, thr, k, _ = crafted_cases()[name]
    boosted = crafted_boosted()
    got = impl.select_probe(heat[None].to(DEV), nhwc(boosted).to(DEV), H, W, thr, k)
    torch.cuda.synchronize()
    want = restated_selection(heat, boosted, H, W, thr, k)
    n = int(got["num_keypoints"][0])
    assert int(got["status"][0]) == 0
    assert n == len(want["scores"]), f"{name}: {n} key-points, the rule gives {len(want['scores'])}"
    assert torch.equal(got["keypoints"][0, :n].cpu(), want["keypoints"]) and torch.equal(got["scores"][0, :n].cpu(), want["scores"]), name
    assert not got["keypoints"][0, n:].any() and not got["scores"][0, n:].any() and not got["descriptors"][0, n:].any()
    if n:
        ref = restated_selection(heat.double(), boosted.double(), H, W, thr, k)["descriptors"]
        assert rel(got["descriptors"][0, :n], ref) <= _bar(want["descriptors"], ref)


def test_constant_map_overflows_and_retry_succeeds():
    _, impl = _impl()
    heat, boosted = torch.full((1, 32, 32), 0.1), crafted_boosted()
    got = impl.select_probe(heat.to(DEV), nhwc(boosted).to(DEV), 28, 28, 0.05, 5000)
    torch.cuda.synchronize()
    assert int(got["status"][0]) & 2, "one plateau: more key-points than the NMS bound holds"
    got = impl.select_probe(heat.to(DEV), nhwc(boosted).to(DEV), 28, 28, 0.05, 5000, kcap=32 * 32)
    torch.cuda.synchronize()
    want = restated_selection(heat[0], boosted, 28, 28, 0.05, 5000)
    n = int(got["num_keypoints"][0])
    assert int(got["status"][0]) == 0 and n == 28 * 28
    assert torch.equal(got["keypoints"][0, :n].cpu(), want["keypoints"]) and torch.equal(got["scores"][0, :n].cpu(), want["scores"])
    assert not got["keypoints"][0, n:].any()


# ------------------------------------------------------------------ launch gate
def test_launches_are_covered():
    """The forward in each arithmetic mode under the route recorders: the shared-GEMM launches (the trunk's) must be pairs the GEMM case
    tables check against float64; LiftFeat launches none of the 3x3 convolution kernels, attention kernels or fused FFNs."""
    import test_gpu_gemm_variants as gv
    from imcui_hip import backend as be
    from imcui_hip.hloc.extractors.liftfeat import Liftfeat

    covered = gv.covered_pairs()
    m = Liftfeat({"state_dict": dict(state())}).eval().to(DEV)
    img = image(50, 70, seed=3, batch=2).to(DEV)
    resets = (be.gemm_route_reset, be.attn_route_reset, be.conv_route_reset, be.ffn_route_reset)
    try:
        for mode in (1, 0):
            be.set_precision(DEV, mode)
            for reset in resets:
                reset(DEV)
            m.forward_batched(img)
            torch.cuda.synchronize()
            feats = be.gemm_route_features(DEV)
            counts = be.gemm_route_counts(DEV)
            pairs = set()
            for r in counts:
                pairs |= gv.pairs_of(r, feats.get(r, 0))
            print(f"mode {mode}: {sum(counts.values())} shared-GEMM launches: {gv.pair_names(pairs)}")
            assert sum(counts.values()) == 19, "the trunk's 15 layers and the key-point head's 4"
            assert pairs <= covered, f"launched without a float64 case: {gv.pair_names(pairs - covered)}"
            assert be.conv_route_counts(DEV) == {} and be.attn_route_counts(DEV) == {} and be.ffn_route_counts(DEV) == {}
    finally:
        be.set_precision(DEV, 1)
        for reset in resets:
            reset(DEV)
