"""SFD2 without a GPU: the restatement (tests/sfd2_reference.py) against the golden file written by the reference's own wrapper; its
explicit-order forms against its torch forms; the key table, the configuration read from shapes and the strict packer with their
refusals; the crafted selection cases the GPU test replays (their hand-written expectations are checked here against the restated rule);
the seeded weights' operating point; and the near-tie cap the GPU tests rely on (seed 0).

Agreement of the explicit forms with the torch forms, measured here (float32, CPU): the depth-to-space equals F.pixel_shuffle bit for
bit; 1 / (1 + exp(-v)) is within 2 ulp of torch.sigmoid on [-40, 40] (asserted: 4 ulp); the explicit sampler is within 9e-8 absolute of
grid_sample + F.normalize on unit descriptors (asserted: 1e-6)."""
from __future__ import annotations

import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sfd2_reference as R
from imcui_hip import backend
from imcui_hip.synth_weights import sfd2_synth_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sfd2_golden.npz")
SIZES = ((32, 48), (50, 70), (96, 128))  # the images of the GPU tests; 50x70 is odd behind both stride-2 layers (score map 52x72)
SEED = 0  # satisfies the near-tie cap below at every size; a seed that did not would be replaced and recorded here
CAP = 0.02


def image(h, w, seed=0, batch=1):
    return torch.rand(batch, 3, h, w, generator=torch.Generator().manual_seed(4000 + 10 * h + seed))


@functools.lru_cache(maxsize=None)
def state(seed=SEED, **kw):
    return sfd2_synth_state(seed, **dict(kw))


@functools.lru_cache(maxsize=None)
def net(seed=SEED, double=False):
    m = R.load_sfd2(state_dict=state(seed))
    return m.double() if double else m


@functools.lru_cache(maxsize=None)
def parts(h, w, seed=0, double=False):
    img = image(h, w, seed)
    with torch.no_grad():
        return net(double=double).parts(R.normalise_image(img.double() if double else img))


def relmax(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


def nms_maxima(score, image_size, border=4):
    """Scores of the NMS survivors inside the border band of one map [Hs,Ws]."""
    H, W = image_size
    nms = R.simple_nms(score[None])[0][border : H - border, border : W - border]
    return nms[nms > 0]


def median_threshold(hw):
    """Midway between the two middle candidate scores of the float64 restatement."""
    return R.between(nms_maxima(parts(*hw, double=True)["score"][0], hw))


def compare_keypoints(pix_a, sc_a, pix_b, sc_b, map_b, Ws, threshold, tol):
    """The key-points of run a (pixel indices, scores) against run b's on run b's score map [Hs,Ws]: a key-point in only one of the
    two sets may be left out only if its score (on b's map) is within `tol` of the threshold, or a rival inside its NMS window is
    within `tol` of it.  -> (common pixel list, number excused, number unexplained)."""
    a, b = set(pix_a.tolist()), set(pix_b.tolist())
    common = sorted(a & b)
    excused = unexplained = 0
    flat = map_b.flatten()
    for p in sorted(a ^ b):
        y, x = divmod(p, Ws)
        s = float(flat[p])
        win = map_b[max(0, y - R.NMS_RADIUS) : y + R.NMS_RADIUS + 1, max(0, x - R.NMS_RADIUS) : x + R.NMS_RADIUS + 1].flatten()
        rival = (win - s).abs() <= tol
        if abs(s - threshold) <= tol or int(rival.sum()) > 1:
            excused += 1
        else:
            unexplained += 1
    return common, excused, unexplained


# ------------------------------------------------------------------ the crafted selection cases (replayed on the GPU)
TH = float(np.float32(0.001))


def _peaks(shape, items, fill=0.0):
    m = torch.full(shape, fill, dtype=torch.float32)
    for x, y, v in items:
        m[y, x] = v
    return m


def crafted_cases() -> dict:
    """name -> (score [B,52,56], image size (H, W), conf, expected): expected = per image the (x, y) list in output order, or an int
    (the count only).  Written by hand from the rule; `test_crafted_expectations` checks them against `R.select`."""
    S = (52, 56)
    base = {"conf_th": 0.001, "remove_borders": 4, "min_keypoints": 0, "max_keypoints": 0}
    sub = [(10, 40, 0.0005), (30, 40, 0.0004)]  # sub-threshold maxima
    three = [(10, 10, 0.9), (30, 10, 0.8), (45, 25, 0.7)]
    c = {}
    c["band_edge"] = (_peaks(S, [(4, 10, 0.9), (3, 20, 0.8), (51, 30, 0.7), (52, 40, 0.6), (20, 4, 0.5), (30, 3, 0.4), (40, 47, 0.3), (25, 48, 0.2)])[None], S, base,
                      [[(4, 10), (51, 30), (20, 4), (40, 47)]])  # fmt: skip
    c["image_smaller_than_map"] = (_peaks(S, [(10, 45, 0.9), (20, 46, 0.8), (30, 47, 0.7), (51, 20, 0.6)])[None], (50, 56), base, [[(10, 45), (51, 20)]])
    c["equal_peaks_4_and_5_apart"] = (_peaks(S, [(10, 10, 0.5), (14, 10, 0.5), (10, 30, 0.5), (15, 30, 0.5), (30, 10, 0.6), (34, 10, 0.5), (30, 30, 0.6), (35, 30, 0.5)])[None],
                                      S, base, [[(30, 10), (30, 30), (10, 10), (14, 10), (10, 30), (15, 30), (35, 30)]])  # fmt: skip
    above = float(np.nextafter(np.float32(TH), np.float32(1.0)))
    c["score_equal_to_conf_th"] = (_peaks(S, [(10, 10, TH), (30, 10, above), (10, 30, 0.5)])[None], S, base, [[(10, 30), (30, 10)]])
    c["min_keypoints_met"] = (_peaks(S, three + sub)[None], S, dict(base, min_keypoints=3), [[(10, 10), (30, 10), (45, 25)]])
    c["min_keypoints_missed_by_one"] = (_peaks(S, three + sub)[None], S, dict(base, min_keypoints=4), [[(10, 10), (30, 10), (45, 25), (10, 40), (30, 40)]])
    c["fallback_in_one_image_of_two"] = (torch.stack([_peaks(S, three + sub), _peaks(S, three + [(20, 25, 0.6)] + sub[:1])]), S, dict(base, min_keypoints=4),
                                         [[(10, 10), (30, 10), (45, 25), (10, 40), (30, 40)], [(10, 10), (30, 10), (45, 25), (20, 25)]])  # fmt: skip
    c["constant_map"] = (torch.full((1, *S), 0.5), S, base, [44 * 48])
    four = [(10, 10, 0.9), (40, 30, 0.5), (20, 20, 0.5), (30, 40, 0.5), (45, 10, 0.5)]
    c["cut_through_four_equal"] = (_peaks(S, four)[None], S, dict(base, max_keypoints=3), [[(10, 10), (45, 10), (20, 20)]])
    c["k_1"] = (_peaks(S, four)[None], S, dict(base, max_keypoints=1), [[(10, 10)]])
    c["max_keypoints_above_count"] = (_peaks(S, four)[None], S, dict(base, max_keypoints=4096), [[(10, 10), (45, 10), (20, 20), (40, 30), (30, 40)]])
    return c


@pytest.mark.parametrize("name", sorted(crafted_cases()))
def test_crafted_expectations(name):
    score, size, conf, expected = crafted_cases()[name]
    for b, exp in enumerate(expected):
        pix, kp, sc, th = R.select(score[b], size, conf)
        if isinstance(exp, int):
            assert len(pix) == exp and torch.equal(pix, torch.sort(pix).values), "a constant map: every pixel of the band, in pixel order"
            continue
        assert [tuple(int(v) for v in row) for row in kp] == exp, name
        assert torch.equal(sc, score[b][kp[:, 1].long(), kp[:, 0].long()])
    if name == "fallback_in_one_image_of_two":
        assert R.select(score[0], size, conf)[3] == 0.0 and R.select(score[1], size, conf)[3] == TH
    if name == "min_keypoints_met":
        assert R.select(score[0], size, conf)[3] == TH


# ------------------------------------------------------------------ explicit-order forms
def _ulps(a, b):
    return (a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max().item()


def test_explicit_forms_equal_the_torch_forms():
    g = torch.Generator().manual_seed(5)
    v = torch.cat([torch.linspace(-40, 40, 20001), torch.randn(20000, generator=g) * 3, torch.tensor([-40.0, 40.0, 0.0])])
    u = _ulps(R.sigmoid_explicit(v), torch.sigmoid(v))
    x = torch.randn(2, 16, 5, 7, generator=g)
    assert torch.equal(R.depth_to_space(x), F.pixel_shuffle(x, 4)[:, 0])
    dmap = F.normalize(torch.randn(1, 128, 12, 17, generator=g), dim=1)
    kp = torch.stack([torch.randint(0, 68, (300,), generator=g), torch.randint(0, 48, (300,), generator=g)], dim=1).float()
    a, b = R.sample_explicit(kp, dmap[0]), R.sample_descriptors(kp, dmap)[0].t()
    d = (a - b).abs().max().item()
    print(f"sigmoid: {u} ulp; sampler: {d:.2e} absolute on unit descriptors")
    assert u <= 4 and d <= 1e-6
    assert bool(((a * a).sum(dim=1) - 1).abs().max() < 1e-6)


# ------------------------------------------------------------------ the key table, the configuration, the packer
def test_layer_table_and_config():
    from imcui_hip.hloc.extractors.sfd2 import map_sfd2_keys

    sd = map_sfd2_keys(state())
    cfg = backend.sfd2_config(sd)
    assert cfg == {"widths": (64, 128, 256), "blocks": 3, "group_channels": 8, "hidden": 256, "k": (3, 1), "bn": 1, "bias": 1, "block_bias": 0}
    layers = backend.sfd2_layers(cfg)
    assert [L["name"] for L in layers[:6]] == [f"{n}.0" for n, _ in R.TRUNK] and [L["stride"] for L in layers[:6]] == [s for _, s in R.TRUNK]
    assert [(L["kind"], L["block"]) for L in layers[6:9]] == [("conv1x1", 1), ("grouped3x3", 2), ("conv1x1", 3)]
    assert len(layers) == 6 + 9 + 1 and layers[-1]["kind"] == "heads" and layers[-1]["cout"] == 512 and layers[0]["kind"] == "stem"
    names = backend.sfd2_tensor_names(cfg)
    assert set(names) == {k for k in state() if not k.endswith("num_batches_tracked")}
    packed, cfg2 = backend.pack_sfd2(sd)
    p = packed.numpy()
    assert cfg2 == cfg and p[0] == 21318.0 and list(p[1:13]) == [64, 128, 256, 3, 8, 256, 3, 1, 1, 1, 0, 0]
    assert np.array_equal(p[16:22], np.array(R.MEAN + R.STD, dtype=np.float32))
    # layer 0: [tap][cin][64] with the BatchNorm scale folded in float32
    s = state()
    scale = (s["conv1a.1.weight"] / torch.sqrt(s["conv1a.1.running_var"] + 1e-5)).numpy()
    w0 = (s["conv1a.0.weight"].numpy() * scale[:, None, None, None]).reshape(64, 3, 9).transpose(2, 1, 0)
    assert np.allclose(p[64 : 64 + 27 * 64].reshape(9, 3, 64), w0, rtol=1e-6, atol=0)


@pytest.mark.parametrize("kw", [dict(k_pb=1), dict(k_db=3), dict(bn=False), dict(bias=False), dict(groups=16, blocks=2), dict(groups=64, blocks=1), dict(widths=(64, 64, 128), hidden=128)])
def test_config_is_read_from_shapes(kw):
    sd = state(SEED, **kw)
    packed, cfg = backend.pack_sfd2({k: v for k, v in sd.items()})
    full = {**dict(widths=(64, 128, 256), blocks=3, groups=32, hidden=256, k_pb=3, k_db=1, bn=True, bias=True), **kw}
    assert cfg["widths"] == tuple(full["widths"]) and cfg["blocks"] == full["blocks"] and cfg["group_channels"] == full["widths"][2] // full["groups"]
    assert cfg["k"] == (full["k_pb"], full["k_db"]) and cfg["bn"] == int(full["bn"]) and cfg["bias"] == int(full["bias"]) and cfg["hidden"] == full["hidden"]
    assert packed.numel() > 0 and bool(torch.isfinite(packed).all())
    R.load_sfd2(state_dict=sd)  # the restatement builds itself from the same shapes


def test_refusals():
    from imcui_hip.hloc.extractors.sfd2 import map_sfd2_keys

    sd = dict(state())
    with pytest.raises(backend.ImcuiHipError, match="SFD2_KEYS.*segmentation.0.weight"):
        map_sfd2_keys({**sd, "segmentation.0.weight": torch.zeros(1)})
    assert not any(k.endswith("num_batches_tracked") for k in map_sfd2_keys(sd))
    with pytest.raises(backend.ImcuiHipError, match="missing.*conv2a.0.weight"):
        backend.pack_sfd2({k: v for k, v in sd.items() if k != "conv2a.0.weight"})
    with pytest.raises(backend.ImcuiHipError, match="conv3b.0.weight.*is missing"):
        backend.pack_sfd2({k: v for k, v in sd.items() if k != "conv3b.0.weight"})
    with pytest.raises(backend.ImcuiHipError, match="unexpected.*conv4.7.bn1.weight"):
        backend.pack_sfd2({**sd, "conv4.7.bn1.weight": torch.ones(256)})
    with pytest.raises(backend.ImcuiHipError, match="shape"):
        backend.pack_sfd2({**sd, "conv2a.0.weight": torch.zeros(128, 64, 1, 1)})
    with pytest.raises(backend.ImcuiHipError, match="1x1 or 3x3"):
        backend.pack_sfd2({**sd, "convPb.weight": torch.zeros(16, 256, 5, 5)})
    with pytest.raises(backend.ImcuiHipError, match="16"):
        backend.pack_sfd2({**sd, "convPb.weight": torch.zeros(65, 256, 1, 1)})
    with pytest.raises(backend.ImcuiHipError, match="refuses the configuration"):  # 32 channels per group
        backend.pack_sfd2(dict(state(SEED, groups=8)))
    with pytest.raises(ValueError, match="negative"):
        backend.sfd2_select_conf({"max_keypoints": -1})
    with pytest.raises(ValueError, match="multiscale"):
        backend.sfd2_select_conf({"multiscale": True})
    with pytest.raises(ValueError, match="RGB"):
        backend.sfd2_check_args((1, 1, 32, 32))
    with pytest.raises(ValueError, match="at least 16"):
        backend.sfd2_check_args((1, 3, 15, 32))


def test_plugin_conf_and_preprocessing_rule():
    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc.extractors.sfd2 import SFD2

    assert SFD2.default_conf == {"max_keypoints": 4096, "model_name": "sfd2_20230511_210205_resnet4x.79.pth", "conf_th": 0.001}
    assert SFD2.required_inputs == ["image"]
    conf = ef.confs["sfd2"]
    assert conf["output"] == "feats-sfd2-n4096-r1600" and conf["model"] == {"name": "sfd2", "max_keypoints": 4096}
    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, **conf["preprocessing"]})
    # ImageDataset.__getitem__ (:83-88): force_resize scales the longer side to resize_max, whatever the size; width / height are not read
    assert ef.target_size((1280, 960), pconf) == (1600, 1200) and ef.target_size((2000, 1000), pconf) == (1600, 800)
    assert ef.target_size((1280, 960), SimpleNamespace(**{**vars(pconf), "resize_max": 640})) == (640, 480)


# ------------------------------------------------------------------ the seeded weights' operating point and the near-tie cap
def test_synthetic_weights_operating_point():
    for hw in SIZES + ((40, 56),):
        m = nms_maxima(parts(*hw)["score"][0], hw)
        share = (m > 0.5).float().mean().item()
        print(f"{hw}: {len(m)} NMS maxima inside the band, {100 * share:.0f} % above 0.5, lowest {m.min().item():.3f}")
        assert 0.3 <= share <= 0.7 and m.min().item() > 0.001


@pytest.mark.parametrize("hw", SIZES)
def test_float32_against_float64_stays_within_the_cap(hw):
    """The restatement in float32 against itself in float64, at the default conf and at the median threshold: the key-points that differ
    are all excused by the two closeness tests, and are at most 2 % of the key-points."""
    p32, p64 = parts(*hw), parts(*hw, double=True)
    s32, s64 = p32["score"][0], p64["score"][0]
    spread = (s32.double() - s64).abs().max().item()
    Ws = s64.shape[1]
    for conf in ({}, {"conf_th": median_threshold(hw), "min_keypoints": 0}):
        a, b = R.select(s32, hw, conf), R.select(s64, hw, conf)
        common, excused, unexplained = compare_keypoints(a[0], a[2], b[0], b[2], R.simple_nms(s64[None])[0], Ws, b[3], spread)
        print(f"{hw} {conf or 'default'}: {len(b[0])} key-points, spread {spread:.2e}, {excused} excused, {unexplained} unexplained")
        assert unexplained == 0 and excused <= CAP * max(len(b[0]), 1)
    print(f"{hw}: score map float32 vs float64 {relmax(s32, s64):.2e}, descriptor map {relmax(p32['desc_map'], p64['desc_map']):.2e}")


# ------------------------------------------------------------------ the golden file
@pytest.mark.parametrize("tag", ["40x56", "50x70"])
def test_restatement_reproduces_the_golden_file(tag):
    z = np.load(GOLDEN)
    assert int(z["seed"]) == SEED
    img = torch.from_numpy(z[f"image_u8_{tag}"]).float() / 255.0
    m = net()
    full = z[f"descriptors_default_{tag}"]
    for name, k in (("default", 4096), ("top7", 7), ("above", 1000)):
        with torch.no_grad():
            r = m.extract_local_global({"image": R.normalise_image(img)}, {"max_keypoints": k, "conf_th": 0.001})
        kp, sc, de = r["keypoints"][0].numpy(), r["scores"][0].numpy(), r["descriptors"][0].numpy().T
        want = full if name == "default" else full[z[f"desc_rows_{name}_{tag}"]]
        # the CPU library sums a convolution in an order that depends on its thread count: the same key-points in the same order,
        # scores and (unit) descriptors within 1e-5 absolute, the bar of the other golden files written through a restated network
        errs = (np.abs(sc - z[f"scores_{name}_{tag}"]).max(), np.abs(de - want).max())
        print(f"{tag} {name}: {len(sc)} key-points; max |difference| scores {errs[0]:.2e}, descriptors {errs[1]:.2e}")
        assert np.array_equal(kp, z[f"keypoints_{name}_{tag}"]) and errs[0] <= 1e-5 and errs[1] <= 1e-5
        assert len(sc) == (7 if k == 7 else len(full)) and (np.diff(sc) <= 0).all(), "descending scores"
