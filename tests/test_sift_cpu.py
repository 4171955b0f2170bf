"""SIFT without a GPU: the restatement (tests/sift_reference.py) against the reference's own wrapper functions (golden files written by
tests/golden/make_sift_golden.py), against itself in float32, and against a shift of the image; the plugin's contract; the batch drivers'
`scales` / `oris` datasets."""
from __future__ import annotations

import functools
import json
import os

import numpy as np
import pytest
import torch

import sift_reference as R

SIZES = {"97x131": (97, 131, 0), "240x320": (240, 320, 1)}
FLOOR = 64 * 2.0**-24


# ------------------------------------------------------------------ the wrapper half that is in the reference
@pytest.mark.parametrize("tag", ["r0", "r3", "r0_all"])
def test_wrapper_stages_and_rootsift_equal_the_reference_functions(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, f"sift_wrapper_{tag}.npz"))
    shape, radius, maxk = tuple(int(v) for v in g["image_shape"]), int(g["nms_radius"]), int(g["max_keypoints"])
    keep = R.filter_points(g["points"], g["scales"], g["angles"], shape, radius, scores=g["scores"])
    assert np.array_equal(keep, g["keep"])
    if len(keep) > maxk:
        k, tie = R.top_k_keep(g["scores"][keep], maxk)
        assert not tie
        keep = keep[k]
    assert np.array_equal(keep, g["topk"])  # (the reference orders the cut by score; ours keeps detection order: same set)
    assert np.abs(R.rootsift(g["descriptors"].astype(np.float64)) - g["rootsift"]).max() <= 1e-6
    assert np.abs(R.rootsift(g["descriptors"]) - g["rootsift"]).max() <= 1e-6
    # the composition: the same detections as a key-point table (doubled units, degrees) through `wrapper_stages` with the golden radius
    # and cut (retainBest off: it is OpenCV's stage, not the wrapper's).  Degrees -> radians is monotone and maps equal angles to equal
    # angles, so the lowest-|angle| rule decides as on the stored radians: the kept SET must be the reference's.
    n = len(g["points"])
    table = np.zeros((n, 12), np.float32)
    table[:, 10:12], table[:, 8], table[:, 7] = g["points"] * 2, g["scales"] * 2, g["scores"]
    table[:, 9] = (g["angles"].astype(np.float64) * R.DEG).astype(np.float32)
    sel = R.wrapper_stages(table, shape, 0, radius, maxk)
    assert np.array_equal(sel["keep"], g["topk"]) and not sel["tie_at_cut"]
    assert np.array_equal(sel["keypoints"], g["points"][g["topk"]]) and np.array_equal(sel["scales"], g["scales"][g["topk"]])
    assert np.array_equal(sel["scores"], g["scores"][g["topk"]]) and np.abs(sel["oris"] - g["angles"][g["topk"]]).max() < 1e-6


def test_opencv_post_processing_rules():
    t = np.zeros((6, 12), np.float32)
    t[:, 10], t[:, 11], t[:, 8], t[:, 9] = [10, 10, 30, 50, 50, 70], [20, 20, 20, 20, 20, 20], 4, 90
    t[:, 7] = [0.2, 0.3, 0.1, 0.5, 0.5, 0.05]
    sel = R.wrapper_stages(t, (64, 64), 0, None, 0)
    assert sel["keep"].tolist() == [1, 2, 3, 5]  # duplicates: the higher response, then the earlier row
    assert np.array_equal(sel["keypoints"][0], [5, 10]) and sel["scales"][0] == 2 and sel["oris"][0] == np.float32(90) * R.RAD32
    t[4, 9] = 45  # no longer a duplicate: retainBest(2) keeps both tied rows at the cut
    assert R.wrapper_stages(t, (64, 64), 2, None, 0)["keep"].tolist() == [3, 4]
    assert R.wrapper_stages(t, (64, 64), 3, None, 0)["keep"].tolist() == [1, 3, 4]
    assert R.wrapper_stages(t, (64, 64), 0, 0, 0)["keep"].tolist() == [1, 2, 4, 5]  # one per pixel: the lowest |angle| of the tied scores
    sel = R.wrapper_stages(t, (64, 64), 0, 0, 1)
    assert sel["keep"].tolist() == [4] and not sel["tie_at_cut"]
    assert R.wrapper_stages(t, (64, 64), 0, 12, 0)["keep"].tolist() == [1, 4]  # NMS radius 12: pixels 10 apart; row 1 only neighbours the weaker row 2


# ------------------------------------------------------------------ the restatement against itself
@functools.lru_cache(maxsize=None)
def _both(size):
    h, w, seed = SIZES[size]
    img = R.seeded_image(h, w, seed)[None]
    return R.extract(img, dtype=np.float64), R.extract(img, dtype=np.float32)


@pytest.mark.parametrize("size", list(SIZES))
def test_float32_restatement_stays_with_the_float64_one(size):
    a, b = _both(size)
    assert len(a["pyramid"]) == R.num_octaves(*SIZES[size][:2])
    spread = max(np.abs(p.astype(np.float64) - q).max() for p, q in zip(b["pyramid"], a["pyramid"])) / 255.0
    ka, kb = {tuple(r[:4].astype(int)) + (round(float(r[9]) / 10),) for r in a["orient"]["table"]}, {tuple(r[:4].astype(int)) + (round(float(r[9]) / 10),) for r in b["orient"]["table"]}
    differ = len(ka ^ kb)
    print(f"{size}: {len(a['pyramid'])} octaves, {len(a['detect']['extrema'])} extrema, {len(a['orient']['table'])} oriented key-points, {len(a['keep'])} after the wrapper; "
          f"float32 vs float64: pyramid spread / 255 = {spread:.2e} (floor {FLOOR:.2e}), {differ} table rows differ end to end")  # fmt: skip
    assert len(a["keep"]) > 100 and spread < FLOOR  # the floor of the GPU test's bar is above the format's own spread
    assert differ <= 0.01 * len(ka)
    # same pyramid: the float32 refinement takes the float64 decisions
    p32 = [p.astype(np.float32) for p in a["pyramid"]]
    d64, d32 = R.detect(p32, dtype=np.float64), R.detect(p32, dtype=np.float32)
    assert np.array_equal(d64["extrema"], d32["extrema"])
    v64, v32 = (np.array([q["valid"] for q in d["refined"]]) for d in (d64, d32))
    print(f"{size}: same pyramid, {int((v64 != v32).sum())} of {int(v64.sum())} refined key-points differ between float32 and float64")
    assert (v64 != v32).sum() <= 0.01 * v64.sum()


def test_tiny_octaves_reflect_repeatedly():
    x = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert R.reflect101(np.arange(-7, 10), 3).tolist() == [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1]
    out = R.blur(x, 3.09, np.float64)  # radius 13 on a 3 x 4 image
    assert out.shape == (3, 4) and np.isfinite(out).all() and abs(out.mean() - x.mean()) < 1.0
    assert np.allclose(R.blur(np.full((3, 5), 7.0), 2.0, np.float32), 7.0, atol=1e-5)


def test_shift_consistency_of_the_restatement():
    a, b = R.shift_pair(240, 320)
    ra, rb = R.extract(a), R.extract(b)
    res = R.shift_consistency(ra, rb, (240, 320), R.mutual_nn(ra["descriptors"], rb["descriptors"]))
    print(f"restatement, crops offset by {R.SHIFT}: {res}")
    assert res["interior"] > 100 and res["share"] > 0.9 and res["matched_share"] > 0.9


# ------------------------------------------------------------------ plugin contract
def test_plugin_conf_and_refusals(lib, golden_dir):
    import imcui_hip.hloc.extractors as extractors
    from imcui_hip import ImcuiHipError
    from imcui_hip.hloc.utils.base_model import BaseModel, dynamic_load

    SIFT = dynamic_load(extractors, "sift")
    ref = json.load(open(os.path.join(golden_dir, "sift_conf.json")))
    assert issubclass(SIFT, BaseModel) and SIFT.__name__ == "SIFT"
    assert SIFT.default_conf == ref["default_conf"] and list(SIFT.default_conf) == list(ref["default_conf"]) and SIFT.required_data_keys == ref["required_data_keys"]
    m = SIFT({"max_keypoints": 300})
    assert m.conf["max_keypoints"] == 300 and m.conf["num_octaves"] == 4 and len(list(m.buffers())) == 1
    with pytest.raises(ImcuiHipError):
        m({"image": torch.zeros(1, 1, 64, 64)})  # no CPU fallback
    for bad in ({"backend": "pycolmap"}, {"backend": "pycolmap_cpu"}, {"first_octave": 0}, {"num_octaves": 2}, {"num_octaves": 6}):
        with pytest.raises(ImcuiHipError):
            SIFT(bad)
    with pytest.raises(ValueError):
        SIFT({"backend": "vlfeat"})
    assert lib.imcui_hip_sift_num_octaves(97, 131) == R.num_octaves(97, 131) == 7 and lib.imcui_hip_sift_num_octaves(480, 640) == R.num_octaves(480, 640)
    for layers in (3, 4, 5):
        want = sum((layers + 3) * 2 * h * w for h, w in zip(*[[s >> o for o in range(R.num_octaves(97, 131))] for s in (2 * 97, 2 * 131)]))
        assert lib.imcui_hip_sift_pyramid_floats(2, 97, 131, layers) == want
        assert lib.imcui_hip_sift_workspace_bytes(2, 97, 131, layers, 1024, 512) > 4 * want
    assert lib.imcui_hip_sift_workspace_bytes(1, 97, 131, 6, 1024, 512) == 0 and lib.imcui_hip_sift_workspace_bytes(1, 97, 131, 4, 512, 1024) == 0


# ------------------------------------------------------------------ drivers
class _StubExtractor(torch.nn.Module):
    """What the batch driver needs of a plugin, with fixed outputs."""

    def __init__(self):
        super().__init__()
        self.register_buffer("anchor", torch.zeros(1))

    def forward_checked(self, batch):
        B, K = batch.shape[0], 5
        g = torch.Generator().manual_seed(int(batch.shape[-1]))
        out = {"keypoints": torch.rand(B, K, 2, generator=g) * 50, "scores": torch.rand(B, K, generator=g), "descriptors": torch.rand(B, K, 128, generator=g),
               "scales": torch.rand(B, K, generator=g) * 8 + 2, "oris": torch.rand(B, K, generator=g) * 6}  # fmt: skip
        self.last = out
        return out, [4] * B


def test_drivers_carry_scales_and_oris(tmp_path, monkeypatch):
    from PIL import Image

    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import match_features as mf

    root = tmp_path / "images"
    root.mkdir()
    rng = np.random.default_rng(0)
    for name in ("a.png", "b.png"):
        Image.fromarray(rng.integers(0, 255, (60, 80), dtype=np.uint8)).save(root / name)
    # half-size "preprocessing" on the host, so that the resize factor (2) shows in the stored scales
    monkeypatch.setattr(ef, "preprocess_on_device", lambda img, conf, device, rgb=False: torch.as_tensor(img)[None, None, ::2, ::2].float() / 255)
    model = _StubExtractor()
    conf = {"output": "feats-stub", "model": {"name": "sift"}, "preprocessing": {"grayscale": True}}
    for as_half, dt in ((True, np.float16), (False, np.float32)):
        path = ef.main(conf, root, tmp_path / f"out{as_half}", model=model, batch_size=2, decode="host", as_half=as_half)
        store = mf.H5FeatureStore(path)
        for b, name in enumerate(("a.png", "b.png")):
            f = store.get(name)
            assert f["scales"].dtype == dt and f["oris"].dtype == dt and f["scales"].shape == (4,) and f["oris"].shape == (4,)
            assert np.array_equal(f["scales"], (model.last["scales"][b, :4].numpy() * np.float32(2.0)).astype(dt))  # x scales.mean() of the resize
            assert np.array_equal(f["oris"], model.last["oris"][b, :4].numpy().astype(dt))
    # collation: present on both sides -> [B, ncap] tensors; absent -> exactly the old batch
    batch, c0, c1 = mf.collate([("a.png", "b.png")], [0], store, store, torch.device("cpu"))
    assert c0 == [4] and batch["scales0"].shape == (1, 4) and torch.equal(batch["oris1"][0], torch.from_numpy(store.get("b.png")["oris"]))
    plain = mf.DictFeatureStore({n: {k: v for k, v in store.get(n).items() if k not in ("scales", "oris")} for n in ("a.png", "b.png")})
    batch2, _, _ = mf.collate([("a.png", "b.png")], [0], plain, plain, torch.device("cpu"))
    assert set(batch2) == set(batch) - {"scales0", "oris0", "scales1", "oris1"}

    class _StubMatcher:
        add_scale_ori = True

        def forward_batched(self, kpts0, kpts1, desc0, desc1, n0, n1, size0, size1, layer_dump=False, scales_oris=None):
            self.got = scales_oris
            return {"matches0": torch.full(kpts0.shape[:2], -1, dtype=torch.int32), "matching_scores0": torch.zeros(kpts0.shape[:2])}

    sink, matcher = mf.DictMatchSink(), _StubMatcher()
    assert mf.match_from_pairs(matcher, [("a.png", "b.png")], store, store, sink, device=torch.device("cpu")) == 1
    assert len(matcher.got) == 4 and torch.equal(matcher.got[0], batch["scales0"]) and torch.equal(matcher.got[3], batch["oris1"])
    with pytest.raises(ValueError, match="add_scale_ori"):
        mf.match_from_pairs(matcher, [("a.png", "b.png")], plain, plain, mf.DictMatchSink(), device=torch.device("cpu"))
    matcher.add_scale_ori = False  # a matcher without the encoding is called exactly as before
    matcher.got = "unset"
    mf.match_from_pairs(matcher, [("a.png", "b.png")], store, store, mf.DictMatchSink(), device=torch.device("cpu"))
    assert matcher.got is None
