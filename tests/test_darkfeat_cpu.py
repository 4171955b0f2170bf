"""DarkFeat without a GPU: the restatement (tests/darkfeat_reference.py) against the golden file written by the reference's own wrapper
and against a second, independent float64 numpy evaluation of the score rule; the strict packer and its refusals; the plugin's conf
table; the seeded weights' operating point; and the near-tie caps the GPU tests rely on (seed 0)."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import darkfeat_reference as R
from imcui_hip import backend
from imcui_hip.synth_weights import DARKFEAT_LAYERS, darkfeat_synth_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "darkfeat_golden.npz")
SIZES = ((32, 48), (50, 70), (96, 128))  # the images of the GPU tests; 50x70 is odd behind both stride-2 layers
SEED = 0  # satisfies the near-tie caps below at every size; a seed that did not would be replaced and recorded here


def image(h, w, seed=0, batch=1):
    return torch.rand(batch, 3, h, w, generator=torch.Generator().manual_seed(3000 + 10 * h + seed))


@functools.lru_cache(maxsize=None)
def state(seed=SEED, bias=False):
    return darkfeat_synth_state(seed, bias=bias)


@functools.lru_cache(maxsize=None)
def net(seed=SEED, double=False, bias=False):
    m = R.DarkFeat(state_dict=state(seed, bias))
    return m.double() if double else m


@functools.lru_cache(maxsize=None)
def parts(h, w, seed=0, double=False):
    img = image(h, w, seed)
    with torch.no_grad():
        return net(double=double).parts(img.double() if double else img)


def relmax(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


def score_bar(hw):
    """max(1e-4, 3 x the restatement's float32-vs-float64 spread), relative to the map's largest magnitude; and that magnitude."""
    s32, s64 = parts(*hw)["score"], parts(*hw, double=True)["score"]
    return max(1e-4, 3 * relmax(s32, s64)), s64.abs().max().item()


def candidates(score, det=R.DET):
    """Pixels that pass everything but the threshold, row-major."""
    return torch.nonzero(R.detect_mask(score, dict(det, score_thld=-1.0)).flatten()).flatten()


def median_threshold(hw):
    """Midway between the two middle candidate scores of the float64 restatement."""
    s64 = parts(*hw, double=True)["score"][0]
    return R.between(s64.flatten()[candidates(s64)])


# ------------------------------------------------------------------ the packer
def test_layer_table_is_the_restatements():
    got = [(L["name"], L["cin"], L["cout"], L["stride"], L["norm"], L["tap"]) for L in backend.darkfeat_layers()]
    assert got == list(R.LAYERS) == list(DARKFEAT_LAYERS)
    names = backend.darkfeat_tensor_names()
    assert names[:2] == ["conv0.0.weight", "conv0.0.bias"] and names[-5:] == ["clf.weight", "clf.bias"] + [f"moving_avg_params.{i}" for i in range(3)]


@pytest.mark.parametrize("bias", [False, True])
def test_packer_round_trip(bias):
    sd = state(SEED, bias)
    assert any(k.endswith(R.DROPPED) for k in sd), "the synthetic checkpoint carries the keys upstream drops"
    assert ("conv3.0.bias" in sd) == bias
    p = backend.pack_darkfeat(sd).numpy()
    assert p[0] == 17478.0 and [p[1 + i] for i in range(3)] == [float(sd[f"moving_avg_params.{i}"]) for i in range(3)]
    w0 = sd["conv0.0.weight"].numpy()  # [32,3,3,3] -> [tap][cin][32] at 64
    assert np.array_equal(p[64 : 64 + 864].reshape(9, 3, 32), w0.reshape(32, 3, 9).transpose(2, 1, 0))
    off = 64 + 896
    assert np.array_equal(p[off : off + 32], sd["conv0.0.bias"].numpy() if bias else np.zeros(32, np.float32))
    off += 64  # conv1 as a GEMM layer: [cout][tap][cin], then its bias
    w1 = sd["conv1.0.weight"].numpy()
    assert np.array_equal(p[off : off + 32 * 288].reshape(32, 9, 32), w1.reshape(32, 32, 9).transpose(0, 2, 1))
    off += 32 * 288
    assert np.array_equal(p[off : off + 32], sd["conv1.0.bias"].numpy() if bias else np.zeros(32, np.float32))
    # clf at the end: [2][128] and the bias, each on its own 64-float slot
    assert np.array_equal(p[-320:-64], sd["clf.weight"].numpy().reshape(-1))
    assert np.array_equal(p[-64:-62], sd["clf.bias"].numpy())


def test_packer_refusals():
    sd = dict(state())
    missing = {k: v for k, v in sd.items() if k != "conv5.0.weight"}
    with pytest.raises(backend.ImcuiHipError, match="missing.*conv5.0.weight"):
        backend.pack_darkfeat(missing)
    with pytest.raises(backend.ImcuiHipError, match="unexpected.*conv7.0.weight"):
        backend.pack_darkfeat({**sd, "conv7.0.weight": torch.zeros(1)})
    with pytest.raises(backend.ImcuiHipError, match="unexpected.*conv0.1.weight"):  # an AFFINE norm is not one of the dropped keys
        backend.pack_darkfeat({**sd, "conv0.1.weight": torch.ones(32)})
    with pytest.raises(backend.ImcuiHipError, match="shape"):
        backend.pack_darkfeat({**sd, "conv2.0.weight": torch.zeros(64, 32, 1, 1)})
    with pytest.raises(backend.ImcuiHipError, match="missing.*moving_avg_params.2"):
        backend.pack_darkfeat({k: v for k, v in sd.items() if k != "moving_avg_params.2"})
    # the BatchNorm-statistics keys upstream drops are ignored wherever they sit
    extra = {**sd, "conv3.1.running_var": torch.ones(64), "bn1.0.num_batches_tracked": torch.tensor(3)}
    assert torch.equal(backend.pack_darkfeat(extra), backend.pack_darkfeat(sd))


# ------------------------------------------------------------------ the score rule, evaluated a second time
def _np_up(m, H, W):
    """bilinear, align_corners=True, float64 numpy: m [h,w] -> [H,W]."""
    h, w = m.shape
    ys = np.arange(H) * ((h - 1) / (H - 1)) if H > 1 else np.zeros(1)
    xs = np.arange(W) * ((w - 1) / (W - 1)) if W > 1 else np.zeros(1)
    y0, x0 = np.minimum(np.floor(ys).astype(int), h - 1), np.minimum(np.floor(xs).astype(int), w - 1)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    fy, fx = (ys - y0)[:, None], (xs - x0)[None]
    return (1 - fy) * ((1 - fx) * m[y0][:, x0] + fx * m[y0][:, x1]) + fy * ((1 - fx) * m[y1][:, x0] + fx * m[y1][:, x1])


def _np_softplus(v):
    return np.where(v > 20, v, np.log1p(np.exp(np.minimum(v, 20))))


def _np_score(raws, mavg, desc, cw, cb, H, W):
    total = np.zeros((H, W))
    for i, (x, d) in enumerate(zip(raws, R.DILATION)):
        x = x / mavg[i]
        C, h, w = x.shape
        xp = np.pad(x, ((0, 0), (d, d), (d, d)), mode="reflect")
        box = np.zeros_like(x)
        for dy in (0, d, 2 * d):
            for dx in (0, d, 2 * d):
                box += xp[:, dy : dy + h, dx : dx + w]
        s = (_np_softplus(x - box / 9) * _np_softplus(x - x.mean(axis=0, keepdims=True))).max(axis=0)
        total += (i + 1) / 6 * _np_up(s, H, W)
    logit = np.einsum("oc,chw->ohw", cw, desc * desc) + cb[:, None, None]
    e = np.exp(logit - logit.max(axis=0, keepdims=True))
    return total * _np_up(e[1] / e.sum(axis=0), H, W)


@pytest.mark.parametrize("hw", [(18, 22), (50, 70)])
def test_score_rule_against_an_independent_float64_evaluation(hw):
    H, W = hw
    with torch.no_grad():
        o = net(double=True).parts(image(H, W, seed=3).double())
    m = net(double=True)
    raws = [o["raw"][i][0].numpy() for i, L in enumerate(R.LAYERS) if L[5] >= 0]
    want = _np_score(raws, [float(p) for p in m.moving_avg_params], o["desc_map"][0].numpy(), m.clf.weight.detach()[:, :, 0, 0].numpy(), m.clf.bias.detach().numpy(), H, W)
    err = np.abs(o["score"][0].numpy() - want).max() / np.abs(want).max()
    print(f"{hw}: restated score against the numpy evaluation {err:.2e}")
    assert err < 1e-12
    # the map sizes behind the stride-2 layers
    assert backend.darkfeat_map_sizes(H, W) == (*o["peaks"][1].shape[-2:], *o["peaks"][2].shape[-2:])


def test_input_norm_and_instance_norm_definitions():
    x = image(17, 23, seed=5, batch=2).double()
    n = R.normalise_image(x)
    for b in range(2):
        v = x[b].flatten()
        assert torch.allclose(n[b].flatten(), (v - v.mean()) / torch.sqrt(((v - v.mean()) ** 2).sum() / (len(v) - 1)), atol=1e-12)
    y = torch.randn(2, 4, 5, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    want = F.relu((y - y.mean(dim=(2, 3), keepdim=True)) / torch.sqrt(y.var(dim=(2, 3), unbiased=False, keepdim=True) + 1e-5))
    assert torch.allclose(R.inorm_relu(y), want, atol=1e-12)


# ------------------------------------------------------------------ the plugin's conf table
def test_plugin_conf_table_and_refusals():
    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc.extractors.darkfeat import DarkFeat

    assert DarkFeat.default_conf == {"model_name": "DarkFeat.pth", "max_keypoints": 1000, "detection_threshold": 0.5, "sub_pixel": False}
    assert DarkFeat.required_inputs == ["image"]
    conf = ef.confs["darkfeat"]
    assert conf["output"] == "feats-darkfeat-n5000-r1600" and conf["model"]["name"] == "darkfeat" and conf["model"]["max_keypoints"] == 5000
    assert conf["preprocessing"] == {"grayscale": False, "force_resize": True, "resize_max": 1600, "width": 640, "height": 480, "dfactor": 8}
    assert backend.darkfeat_det_conf({}) == {"score_thld": 0.5, "edge_thld": 10, "nms_size": 3, "eof_mask": 5, "kpt_n": 5000} == R.DET
    assert backend.darkfeat_det_conf({"nms_size": 0, "kpt_n": 9})["kpt_n"] == 9
    m = DarkFeat({"state_dict": state(), **conf["model"]})
    assert m.conf["max_keypoints"] == 5000 and "state_dict" not in m.conf and m.packed.dtype == torch.float32
    for bad, word in (({"multi_scale": True}, "multi_scale"), ({"multi_level": False}, "multi_level"), ({"use_peakiness": False}, "use_peakiness"),
                      ({"nms_size": 5}, "nms_size"), ({"max_keypoints": -3}, "negative"), ({"kpt_n": 0}, "kpt_n")):  # fmt: skip
        with pytest.raises(ValueError, match=word):
            DarkFeat({"state_dict": state(), **bad})
    with pytest.raises(ValueError, match="RGB"):
        backend.darkfeat_check_args((1, 1, 64, 64))
    with pytest.raises(ValueError, match="at least 16"):
        backend.darkfeat_check_args((1, 3, 15, 64))
    with pytest.raises(backend.ImcuiHipError, match="ROCm device"):  # no CPU fallback
        m({"image": image(32, 48)})


# ------------------------------------------------------------------ the golden file of the reference's wrapper
@pytest.mark.parametrize("tag", ["40x56", "50x70"])
def test_restatement_through_the_cut_reproduces_the_wrapper_golden(tag):
    """tests/golden/darkfeat_golden.npz was written by imcui/hloc/extractors/darkfeat.py itself around the restated network
    (make_darkfeat_golden.py).  The restatement + `wrapper_cut` reproduce count, order and key-points exactly, and scores and
    descriptors to float32 round-off (the convolutions may be summed in another order on another host)."""
    g = np.load(GOLDEN)
    img = torch.from_numpy(g[f"image_u8_{tag}"]).float() / 255.0
    with torch.no_grad():
        pred = net(int(g["seed"]))({"image": img})
    full = torch.from_numpy(g[f"descriptors_all_{tag}"])
    for name, k in (("all", 0), ("top7", 7), ("above", 1000)):
        r = R.wrapper_cut(pred, k)
        want_kp, want_sc = torch.from_numpy(g[f"keypoints_{name}_{tag}"]), torch.from_numpy(g[f"scores_{name}_{tag}"])
        want_de = full if name == "all" else full[torch.from_numpy(g[f"desc_rows_{name}_{tag}"])]
        n = len(want_sc)
        assert r["keypoints"].shape == (1, n, 2) and r["scores"].shape == (1, n) and r["descriptors"].shape == (1, 128, n)
        assert n == (7 if k == 7 else len(full)) and n > 0 and bool((want_sc[1:] >= want_sc[:-1]).all()), "ascending score"
        errs = ((r["scores"][0] - want_sc).abs().max().item(), (r["descriptors"][0].t() - want_de).abs().max().item())
        print(f"{tag} {name}: {n} key-points; max |difference| scores {errs[0]:.2e}, descriptors {errs[1]:.2e}")
        assert torch.equal(r["keypoints"][0], want_kp) and errs[0] <= 1e-5 and errs[1] <= 1e-5


def test_select_stable_order_cut_and_refusal():
    s = torch.zeros(24, 24)
    for y, x, v in ((8, 8, 2.0), (8, 14, 1.0), (14, 8, 2.0), (14, 14, 2.0), (5, 5, 3.0), (4, 12, 9.0)):  # (4, 12) lies in the border band
        s[y, x] = v
    pix, kp, sc = R.select(s)
    assert pix.tolist() == [8 * 24 + 14, 8 * 24 + 8, 14 * 24 + 8, 14 * 24 + 14, 5 * 24 + 5]  # ascending score, equal scores in pixel order
    assert kp[0].tolist() == [14.0, 8.0] and sc.tolist() == [1.0, 2.0, 2.0, 2.0, 3.0]
    assert R.select(s, R.DET, 3)[0].tolist() == [14 * 24 + 8, 14 * 24 + 14, 5 * 24 + 5]  # the cut keeps the later pixels among equals
    assert R.select(s, dict(R.DET, kpt_n=2), 3)[0].tolist() == [14 * 24 + 14, 5 * 24 + 5]
    assert R.select(s, dict(R.DET, score_thld=2.0))[0].tolist() == [5 * 24 + 5]  # strict threshold
    with pytest.raises(ValueError, match="negative"):
        R.select(s, R.DET, -1)


# ------------------------------------------------------------------ crafted score maps (run on the device by tests/test_gpu_darkfeat.py)
CRAFT_H, CRAFT_W = 32, 40


def _blob(s, y, x, a, b=None, c=0.0):
    """A peak of height 2 at (y, x) with its eight dilation-3 taps: 2 - a above / below, 2 - b left / right, 2 - a - b +- c on the
    diagonals, so that dii = -2 a, djj = -2 b, dij = c there (exact for dyadic a, b, c)."""
    b = a if b is None else b
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            s[y + 3 * dy, x + 3 * dx] = 2.0 - a * dy * dy - b * dx * dx + c * dy * dx
    return s


def crafted_cases():
    """(name, score map [H,W], conf, expectation): `exact` = the kept pixels in output order, `has` / `lacks` = pixels that must / must
    not be kept, `count` = how many are kept.  Blobs are probed at score_thld 1.99, so that only their centres (2.0) are candidates."""
    H, W = CRAFT_H, CRAFT_W
    px = lambda y, x: y * W + x  # noqa: E731
    base = torch.full((H, W), 0.25)
    hi = {"score_thld": 1.99}
    cases = []
    # the border band: eof_mask 5 keeps [5, H - 5) x [5, W - 5)
    s = _blob(_blob(base.clone(), 5, 5, 0.5), H - 6, W - 6, 0.5)
    cases.append(("band: inside on its edge", s, hi, {"exact": [px(5, 5), px(H - 6, W - 6)]}))
    s = _blob(_blob(_blob(base.clone(), 4, 12, 0.5), 12, W - 5, 0.5), H - 5, 20, 0.5)
    cases.append(("band: outside on its edge", s, hi, {"count": 0}))
    cases.append(("band: eof_mask 4", s, {**hi, "eof_mask": 4}, {"exact": [px(4, 12), px(12, W - 5), px(H - 5, 20)]}))
    # the edge ratio (a + b)^2 / (a b) against (10 + 1)^2 / 10 = 12.1 at a = 1
    for b, keep in ((0.09, False), (0.11, True), (1.0, True), (0.02, False)):
        cases.append((f"edge ratio b={b}", _blob(base.clone(), 16, 20, 1.0, b), hi, {"count": int(keep)}))
    # ... and just either side of 121 / 10: the horizontal taps walk over the 17 float32 values around 1.9 (ratio 12.1 -+ 1e-4)
    t = np.float32(1.9)
    for _ in range(8):
        t = np.nextafter(t, np.float32(0))
    for i in range(17):
        cases.append((f"edge ratio walk {i - 8:+d} ulp", _blob(base.clone(), 16, 20, 1.0, 2.0 - float(t)), hi, {"walk": True}))
        t = np.nextafter(t, np.float32(4))
    # det <= 0: a saddle (dii = -2, djj = +3), and det == 0 exactly (dii = djj = -1, dij = 1)
    sad = base.clone()
    sad[16, 20], sad[13, 20], sad[19, 20], sad[16, 17], sad[16, 23] = 2.0, 1.0, 1.0, 3.5, 3.5
    cases.append(("det < 0", sad, hi, {"lacks": [px(16, 20)], "has": [px(16, 17), px(16, 23)]}))
    cases.append(("det == 0", _blob(base.clone(), 16, 20, 0.5, 0.5, c=1.0), hi, {"lacks": [px(16, 20)]}))
    # a plateau-like dome, concave everywhere, without NMS, band and edge ratio: EVERY pixel is a candidate (the list holds H W entries)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    dome = 1000.0 - ((yy - 15.5) ** 2 + (xx - 19.5) ** 2)
    every = {"eof_mask": 0, "nms_size": 0, "edge_thld": 1e6, "kpt_n": H * W}
    cases.append(("every pixel a candidate", dome, every, {"count": H * W}))
    cases.append(("every pixel a candidate, cut to 5", dome, {**every, "max_keypoints": 5}, {"count": 5}))
    cases.append(("a constant map", torch.full((H, W), 4.0), {"eof_mask": 0}, {}))
    # the threshold: all below it; a score equal to it is dropped (strict >); the next float32 below it keeps the pixel
    s = _blob(base.clone(), 16, 20, 0.5)
    cases.append(("all below the threshold", s, {"score_thld": 2.5}, {"count": 0}))
    cases.append(("equal to the threshold", s, {"score_thld": 2.0}, {"count": 0}))
    cases.append(("just above the threshold", s, {"score_thld": float(np.nextafter(np.float32(2.0), np.float32(0)))}, {"exact": [px(16, 20)]}))
    # nms_size 0: the neighbour of a peak counts too
    s2 = _blob(base.clone(), 16, 20, 0.5)
    s2[16, 21] = 1.995
    cases.append(("nms_size 3", s2, hi, {"exact": [px(16, 20)]}))
    cases.append(("nms_size 0", s2, {**hi, "nms_size": 0}, {"has": [px(16, 20), px(16, 21)]}))
    # a cut through equal scores keeps the stable order: the LATER pixels, in pixel order; k = 1; kpt_n cuts the same way
    s = base.clone()
    for y, x in ((8, 8), (8, 24), (20, 8), (20, 24)):
        _blob(s, y, x, 0.5)
    cases.append(("equal scores, all", s, hi, {"exact": [px(8, 8), px(8, 24), px(20, 8), px(20, 24)]}))
    cases.append(("equal scores, k = 2", s, {**hi, "max_keypoints": 2}, {"exact": [px(20, 8), px(20, 24)]}))
    cases.append(("equal scores, k = 1", s, {**hi, "max_keypoints": 1}, {"exact": [px(20, 24)]}))
    cases.append(("equal scores, kpt_n = 3", s, {**hi, "kpt_n": 3}, {"exact": [px(8, 24), px(20, 8), px(20, 24)]}))
    s = s.clone()
    s[8, 24] = 2.5
    cases.append(("k = 1 takes the highest", s, {**hi, "max_keypoints": 1}, {"exact": [px(8, 24)]}))
    return cases


def check_crafted(name, pix, expect):
    pix = pix.tolist()
    if "exact" in expect:
        assert pix == expect["exact"], name
    if "count" in expect:
        assert len(pix) == expect["count"], (name, len(pix))
    assert all(p in pix for p in expect.get("has", ())) and not any(p in pix for p in expect.get("lacks", ())), name


def test_crafted_cases_on_the_restated_detector():
    walk = []
    for name, s, conf, expect in crafted_cases():
        conf = dict(conf)
        pix, kp, sc = R.select(s, dict(R.DET, **{k: v for k, v in conf.items() if k != "max_keypoints"}), conf.get("max_keypoints", 0))
        check_crafted(name, pix, expect)
        assert bool((sc[1:] >= sc[:-1]).all())
        if expect.get("walk"):
            walk.append(len(pix))
    assert walk[0] == 1 and walk[-1] == 0 and sorted(walk, reverse=True) == walk, f"the walk crosses the ratio once: {walk}"


# ------------------------------------------------------------------ the operating point and the near-tie caps
@pytest.mark.parametrize("hw", SIZES + ((40, 56),))
def test_synthetic_weights_put_a_useful_share_of_the_maxima_above_the_threshold(hw):
    s = parts(*hw)["score"][0]
    mx = (s == F.max_pool2d(s[None, None], 3, 1, 1)[0, 0])[5:-5, 5:-5]
    share = (s[5:-5, 5:-5][mx] > 0.5).float().mean().item()
    print(f"{hw}: {int(mx.sum())} maxima inside the band, {share:.2f} of them above 0.5; scores {s.min():.3f} .. {s.max():.3f}")
    assert 0.40 <= share <= 0.75


@pytest.mark.parametrize("hw", SIZES)
def test_near_tie_caps_of_seed_0(hw):
    """What tests/test_gpu_darkfeat.py relies on: float32 against float64 changes at most 2 % of the key-points at every setting it
    uses, and no candidate lies within the score bar of a threshold it uses."""
    bar, top = score_bar(hw)
    s32, s64 = parts(*hw)["score"][0], parts(*hw, double=True)["score"][0]
    med = median_threshold(hw)
    cand = s64.flatten()[candidates(s64)]
    for thr in (0.5, med):
        gap = (cand - thr).abs().min().item()
        print(f"{hw}: threshold {thr:.6f}: nearest candidate {gap:.2e} away (score bar {bar * top:.2e}), {int((cand > thr).sum())} of {len(cand)} candidates above")
        assert gap > bar * top
        for k in (0, 7, 100000):
            a = set(R.select(s32, dict(R.DET, score_thld=thr), k)[0].tolist())
            b = set(R.select(s64, dict(R.DET, score_thld=thr), k)[0].tolist())
            assert len(a) > 0 and len(a ^ b) <= 0.02 * len(b), (thr, k, sorted(a ^ b))
