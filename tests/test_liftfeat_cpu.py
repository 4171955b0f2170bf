"""LiftFeat without a GPU: the restatement (tests/liftfeat_reference.py), the calibration of the synthetic checkpoint, the wrapper's two
output orders, the crafted selection cases the GPU test replays, the strict packer and the plugin's registration.

Calibration of `liftfeat_synth_state(0)` (asserted below): 274 key-points above 0.05 on the 96x128 image and 32 on the 32x48 image (the
bars are 30 and 8); the largest weight any AFT soft-max column puts on one token at 96x128 is 0.115 (layer 0), far below 0.9.
"""
import functools

import numpy as np
import pytest
import torch

import liftfeat_reference as R
from imcui_hip.synth_weights import liftfeat_synth_state

SEED = 0
THRESHOLD = 0.05


@functools.lru_cache(maxsize=None)
def state(seed=SEED, **kw):
    return liftfeat_synth_state(seed, **dict(kw))


@functools.lru_cache(maxsize=None)
def net(double=False, seed=SEED, **kw):
    m = R.load_model(state(seed, **kw))
    return m.double() if double else m


@functools.lru_cache(maxsize=None)
def image(h, w, seed=0, batch=1):
    """[batch,3,h,w] float32 = uint8 values / 255 (what the file driver feeds), seeded."""
    u8 = torch.randint(0, 256, (batch, 3, h, w), generator=torch.Generator().manual_seed(100 + h + 1000 * seed), dtype=torch.uint8)
    return u8.float() / 255.0


def hwc255(img: torch.Tensor) -> np.ndarray:
    """liftfeat.py:35-36: `data["image"].cpu().numpy().squeeze() * 255`, then `.transpose(1, 2, 0)`."""
    return (img.cpu().numpy().squeeze() * 255).transpose(1, 2, 0)


def extract(img: torch.Tensor, double=False, threshold=THRESHOLD, seed=SEED):
    m = net(double, seed)
    maps = R.dense_maps(m, hwc255(img), torch.float64 if double else torch.float32)
    return maps, R.select(maps["heat"], maps["boosted"], img.shape[-2], img.shape[-1], threshold)


# ------------------------------------------------------------------ crafted selection cases (replayed on the GPU by test_gpu_liftfeat_layers.py)
def _peaks(Hp, Wp, peaks, base=0.01):
    m = torch.full((Hp, Wp), base, dtype=torch.float32)
    for x, y, v in peaks:
        m[y, x] = v
    return m


@functools.lru_cache(maxsize=None)
def crafted_cases():
    """name -> (heat [Hp,Wp], H, W, threshold, max_keypoints, expected (x, y) list in output order).  Hp = Wp = 32, the image 28 x 28."""
    six = [(3, 3, 0.3), (12, 3, 0.2), (21, 3, 0.2), (3, 12, 0.2), (12, 12, 0.2), (21, 12, 0.5)]
    rm = [(x, y) for x, y, _ in six]
    c = {
        # a pad-region peak suppresses the real neighbour two pixels to its left and is not itself kept
        "pad_suppresses": (_peaks(32, 32, [(29, 10, 0.5), (27, 10, 0.4), (5, 5, 0.3)]), 28, 28, 0.05, 5000, [(5, 5)]),
        "edge_columns": (_peaks(32, 32, [(27, 4, 0.3), (28, 20, 0.3), (4, 27, 0.3), (20, 28, 0.3)]), 28, 28, 0.05, 5000, [(27, 4), (4, 27)]),
        "score_equals_threshold": (_peaks(32, 32, [(5, 5, 0.25), (15, 15, 0.2500001)]), 28, 28, 0.25, 5000, [(15, 15)]),
        "count_below_k": (_peaks(32, 32, six), 28, 28, 0.05, 7, rm),  # row-major
        "count_equals_k": (_peaks(32, 32, six), 28, 28, 0.05, 6, rm),  # `max_keypoints < len` is false: still row-major
        "ties_cut_stably": (_peaks(32, 32, six), 28, 28, 0.05, 3, [rm[4], rm[0], rm[5]]),  # four 0.2s: the last of them survives
        "k_zero": (_peaks(32, 32, six), 28, 28, 0.05, 0, [rm[1], rm[2], rm[3], rm[4], rm[0], rm[5]]),
        "k_minus_one": (_peaks(32, 32, six), 28, 28, 0.05, -1, [rm[2], rm[3], rm[4], rm[0], rm[5]]),
        "k_minus_seven": (_peaks(32, 32, six), 28, 28, 0.05, -7, []),  # argsort()[7:] of six
    }
    return c


def crafted_boosted(Hp=32, Wp=32):
    return torch.randn(1, 64, Hp // 8, Wp // 8, generator=torch.Generator().manual_seed(77))


def restated_selection(heat, boosted, H, W, threshold, k):
    return R.wrapper_cut(R.select(heat[None, None], boosted.to(heat.dtype), H, W, threshold), k)


@pytest.mark.parametrize("name", sorted(crafted_cases()))
def test_crafted_expectations(name):
    heat, H, W, thr, k, want = crafted_cases()[name]
    got = restated_selection(heat, crafted_boosted(), H, W, thr, k)
    assert [tuple(int(v) for v in p) for p in got["keypoints"]] == want
    assert got["descriptors"].shape == (len(want), 64) and got["scores"].shape == (len(want),)
    for (x, y), s in zip(want, got["scores"]):
        assert s.item() == heat[y, x].item()  # the nearest sample is the pixel itself


def test_constant_map_is_one_plateau():
    heat = torch.full((32, 32), 0.1)
    got = restated_selection(heat, crafted_boosted(), 28, 28, 0.05, 5000)
    assert len(got["keypoints"]) == 28 * 28  # every pixel of the image equals its window's maximum; the pad pixels are dropped
    assert torch.equal(got["keypoints"][:29, 0], torch.cat([torch.arange(28.0), torch.zeros(1)]))  # row-major


# ------------------------------------------------------------------ the restatement
def test_restatement_shapes_and_units():
    img = image(50, 70)
    maps, pred = extract(img)
    assert maps["M1"].shape == (1, 64, 8, 12) and maps["K1"].shape == (1, 65, 8, 12) and maps["D1"].shape == (1, 3, 64, 96)
    assert maps["boosted"].shape == (1, 64, 8, 12) and maps["heat"].shape == (1, 1, 64, 96)
    assert torch.allclose(maps["D1"].norm(dim=1), torch.ones(1, 64, 96), atol=1e-5)
    assert torch.allclose(maps["boosted"].norm(dim=1), torch.ones(1, 8, 12), atol=1e-5)
    n = len(pred["scores"])
    assert pred["keypoints"].shape == (n, 2) and pred["descriptors"].shape == (n, 64) and n > 0
    assert (pred["scores"] > THRESHOLD).all()
    assert torch.allclose(pred["descriptors"].norm(dim=1), torch.ones(n), atol=1e-5)


def test_unfold_layout_is_channel_major():
    d = torch.arange(3 * 8 * 16, dtype=torch.float32).view(1, 3, 8, 16)
    n = R.X.unfold8(d)
    assert n.shape == (1, 192, 1, 2)
    for c, dy, dx, cx in ((0, 0, 0, 0), (2, 7, 3, 1), (1, 4, 5, 0)):
        assert n[0, c * 64 + dy * 8 + dx, 0, cx] == d[0, c, dy, 8 * cx + dx]


def test_pad_mask_and_statistics():
    img = image(50, 70)
    x = R.pad_image(hwc255(img))
    assert x.shape == (1, 3, 64, 96)
    assert not x[..., 50:, :].any() and not x[..., :, 70:].any()
    assert torch.equal(x[..., :50, :70], (img * 255) / 255)
    # the pad zeros count in the statistics: a padded pixel becomes -mean * invstd, not 0
    g = x.mean(dim=1, keepdim=True)
    n = net().norm(g)
    mean, var = g.mean(), g.var(unbiased=False)
    assert torch.allclose(n[0, 0, 60, 90], -mean / torch.sqrt(var + 1e-5), rtol=1e-5)
    real_only = g[..., :50, :70]
    assert abs(real_only.mean() - mean) > 0.1  # the statistics over the real pixels alone are another number
    # no key-point in the pad
    _, pred = extract(img)
    assert (pred["keypoints"][:, 0] < 70).all() and (pred["keypoints"][:, 1] < 50).all()


def test_both_output_orders_and_negative_k():
    _, pred = extract(image(50, 70))
    n = len(pred["scores"])
    assert n > 8
    flat = pred["keypoints"][:, 1] * 96 + pred["keypoints"][:, 0]
    assert (flat[1:] > flat[:-1]).all(), "extract leaves in nonzero (row-major) order"
    same = R.wrapper_cut(pred, n)
    assert torch.equal(same["keypoints"], pred["keypoints"])  # count <= k: untouched
    top = R.wrapper_cut(pred, 7)
    assert len(top["scores"]) == 7 and (top["scores"][1:] >= top["scores"][:-1]).all()  # ascending
    assert top["scores"][-1] == pred["scores"].max()
    allk = R.wrapper_cut(pred, 0)
    assert len(allk["scores"]) == n and (allk["scores"][1:] >= allk["scores"][:-1]).all()
    m1 = R.wrapper_cut(pred, -1)
    assert len(m1["scores"]) == n - 1 and torch.equal(m1["scores"], allk["scores"][1:])  # the lowest score is dropped


def test_top_k_is_stored_not_applied():
    m = R.LiftFeat(state(), top_k=3, detect_threshold=THRESHOLD)
    assert m.top_k == 3 and len(m.extract(hwc255(image(50, 70)))["scores"]) > 3


def test_synthetic_state_is_calibrated():
    _, p96 = extract(image(96, 128))
    _, p32 = extract(image(32, 48))
    print(f"key-points above {THRESHOLD}: {len(p96['scores'])} at 96x128, {len(p32['scores'])} at 32x48")
    assert len(p96["scores"]) >= 30 and len(p32["scores"]) >= 8
    maps, _ = extract(image(96, 128))
    m = net()
    tok = lambda t: t[0].reshape(t.shape[1], -1).t()
    with torch.no_grad():
        x = m.feature_boost.encode(tok(maps["M1"]), tok(maps["K1"]), tok(R.X.unfold8(maps["D1"])))
        for i, layer in enumerate(m.feature_boost.layers):
            peak = torch.softmax(layer.attn.k(x), dim=0).max().item()
            print(f"AFT layer {i}: the largest soft-max weight on one token is {peak:.3f}")
            assert peak <= 0.9
            x = layer(x)


def test_restatement_reads_widths_from_shapes():
    sd = liftfeat_synth_state(1, kenc=False, ffn=96, n_layers=2)
    cfg = R.booster_config(sd)
    assert cfg == {"n_layers": 2, "ffn": 96, "denc": [64, 64, 64], "nenc": [192, 128, 64, 64], "kenc": None}
    assert not hasattr(R.load_model(sd).feature_boost, "kenc")
    with pytest.raises(ValueError, match="heatmap_head.2.weight"):
        R.load_model({**sd, "heatmap_head.2.weight": torch.zeros(1, 64, 1, 1)})
    with pytest.raises(ValueError, match="block3.0.layer.0.weight"):
        R.load_model({**sd, "block3.0.layer.0.weight": torch.zeros(48, 24, 3, 3)})


# ------------------------------------------------------------------ packing, plugin, conf
def test_packing_is_strict(lib):
    from imcui_hip import backend

    sd = dict(state())
    packed, cfg = backend.pack_liftfeat(sd)
    assert cfg == {"kenc": 1, "ffn": 128, "denc": 64, "nenc1": 128, "nenc2": 64, "kenc1": 128, "kenc2": 64, "n_layers": 3}
    assert packed.dtype == torch.float32 and packed.numel() == lib.imcui_hip_liftfeat_packed_floats(backend.liftfeat_cfg_array(cfg))
    names = backend.liftfeat_tensor_names(cfg)
    assert set(names) == {k for k in sd if not k.endswith("num_batches_tracked")} and len(names) == len(set(names))
    assert set(names) == set(backend.liftfeat_tensor_shapes(cfg))
    assert not any(n.startswith("heatmap_head.") for n in names)
    _, cfg2 = backend.pack_liftfeat(liftfeat_synth_state(1, kenc=False, ffn=96, n_layers=2))
    assert cfg2["kenc"] == 0 and cfg2["ffn"] == 96 and cfg2["n_layers"] == 2
    with pytest.raises(backend.ImcuiHipError, match="descriptor_head.0.weight"):  # an unknown key group, by name
        backend.pack_liftfeat({**sd, "descriptor_head.0.weight": torch.zeros(1)})
    with pytest.raises(backend.ImcuiHipError, match="block3.0.layer.0.weight"):  # a foreign trunk width, by name
        backend.pack_liftfeat({**sd, "block3.0.layer.0.weight": torch.zeros(48, 24, 3, 3)})
    with pytest.raises(backend.ImcuiHipError, match="feature_boost.nenc.2.bias"):
        backend.pack_liftfeat({k: v for k, v in sd.items() if k != "feature_boost.nenc.2.bias"})
    with pytest.raises(backend.ImcuiHipError, match="normal_head.1.conv.weight"):
        backend.pack_liftfeat({**sd, "normal_head.1.conv.weight": torch.zeros(16, 32, 1, 1)})
    with pytest.raises(backend.ImcuiHipError, match="not supported"):
        backend.pack_liftfeat(liftfeat_synth_state(1, ffn=256))
    with pytest.raises(ValueError, match="three channels"):
        backend.liftfeat_check_args((1, 1, 32, 32))


def test_packed_linear_is_transposed(lib):
    """final_proj is the last Linear of the layout: Wt [64][64] then the bias, ahead of the normal head."""
    from imcui_hip import backend

    sd = state()
    packed, _ = backend.pack_liftfeat(dict(sd))
    w, b = sd["feature_boost.final_proj.weight"], sd["feature_boost.final_proj.bias"]
    flat = packed.numpy()
    pos = [i for i in range(0, flat.size - 64, 64) if np.array_equal(flat[i : i + 64], b.numpy())]
    assert len(pos) == 1
    assert np.array_equal(flat[pos[0] - 4096 : pos[0]].reshape(64, 64), w.t().numpy())


def test_plugin_and_conf_match_the_reference():
    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.utils.base_model import dynamic_load

    cls = dynamic_load(extractors, "liftfeat")
    assert cls.__name__ == "Liftfeat" and cls.__module__ == "imcui_hip.hloc.extractors.liftfeat"
    assert cls.default_conf == {"keypoint_threshold": 0.05, "max_keypoints": 5000, "model_name": "LiftFeat.pth"}
    assert cls.required_inputs == ["image"]
    conf = ef.confs["liftfeat"]
    assert conf["output"] == "feats-liftfeat-n5000-r1600" and conf["model"] == {"name": "liftfeat", "max_keypoints": 5000}
    assert conf["preprocessing"] == {"grayscale": False, "resize_max": 1600}
