"""DISK without a GPU: the restated network's layout, the library's packing table against it, strict weight loading, kornia's
selection rule on hand-made heatmaps, and the argument refusals (imcui/hloc/extractors/disk.py:18-36 -> kornia DISK)."""
from __future__ import annotations

import pytest
import torch

from disk_reference import DISKReference, Unet, heatmap_to_keypoints, nms


def _sd(seed=0):
    from imcui_hip.synth_weights import disk_state_dict

    return disk_state_dict(seed)


def test_restatement_layout():
    m = DISKReference()
    sd = m.state_dict()
    assert len(sd) == 26
    assert sum(v.numel() for v in sd.values()) == 1_092_369
    assert tuple(sd["unet.path_down.0.1.3.weight"].shape) == (16, 3, 5, 5)
    assert "unet.path_down.0.1.1.weight" not in sd  # the first block has no norm / gate
    assert tuple(sd["unet.path_up.3.conv.3.weight"].shape) == (129, 80, 5, 5)
    assert tuple(sd["unet.path_up.0.conv.1.weight"].shape) == (128,)
    syn = _sd()
    assert {k: tuple(v.shape) for k, v in syn.items()} == {k: tuple(v.shape) for k, v in sd.items()}


def test_library_tensor_names_match_restatement(lib):
    from imcui_hip import backend

    names = backend.disk_tensor_names()
    assert names == list(DISKReference().state_dict().keys())
    assert backend.disk_tensor_shapes() == {k: tuple(v.shape) for k, v in DISKReference().state_dict().items()}


def test_pack_is_strict(lib):
    from imcui_hip import backend

    sd = _sd()
    p = backend.pack_disk(sd)
    assert p.dtype == torch.float32 and p.numel() == lib.imcui_hip_disk_packed_floats()
    missing = dict(sd)
    missing.pop("unet.path_up.2.conv.1.weight")
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_disk(missing)
    with pytest.raises(backend.ImcuiHipError, match="unexpected"):
        backend.pack_disk({**sd, "unet.path_down.0.1.1.weight": torch.ones(3)})
    bad = dict(sd)
    bad["unet.path_up.3.conv.3.weight"] = torch.zeros(128, 80, 5, 5)
    with pytest.raises(backend.ImcuiHipError, match="shape"):
        backend.pack_disk(bad)


def test_weight_containers(tmp_path, lib):
    from imcui_hip.hloc.extractors.disk import resolve_disk_state_dict

    sd = _sd(1)
    for conf in ({"state_dict": sd}, {"state_dict": {"extractor": sd}}):
        got = resolve_disk_state_dict(conf)
        assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    for obj, name in ((sd, "bare.pth"), ({"extractor": sd}, "depth-save.pth")):
        path = tmp_path / name
        torch.save(obj, path)
        got = resolve_disk_state_dict({"weights_path": str(path)})
        assert all(torch.equal(got[k], sd[k]) for k in sd)


def test_plugin_contract_without_gpu():
    from imcui_hip.hloc.extractors.disk import DISK

    assert DISK.default_conf == {"weights": "depth", "max_keypoints": None, "nms_window_size": 5, "detection_threshold": 0.0,
                                 "pad_if_not_divisible": True}  # fmt: skip
    assert DISK.required_inputs == ["image"]


# ---- selection rule (kornia heatmap_to_keypoints) on the restatement
def _kp(heat, **kw):
    (xy, logp), = heatmap_to_keypoints(torch.tensor(heat, dtype=torch.float32)[None, None], **kw)
    return xy.tolist(), logp.tolist()


def test_nms_first_maximum_wins_ties():
    xy, _ = _kp([[1.0, 2.0, 2.0, 0.5]], n=None, window_size=5, score_threshold=0.0)
    assert xy == [[1, 0]]
    # a later tie inside the window loses, an equal pixel outside the window survives
    xy, _ = _kp([[2.0, 1.0, 2.0, 1.0, 0.1]], n=None, window_size=5, score_threshold=0.0)
    assert xy == [[0, 0]]
    xy, _ = _kp([[2.0, 1.0, 2.0, 1.0, 0.1]], n=None, window_size=3, score_threshold=0.0)
    assert xy == [[0, 0], [2, 0]]


def test_strict_threshold_and_row_major_order():
    heat = torch.zeros(9, 9)
    heat[0, 6], heat[4, 0], heat[8, 8], heat[4, 4] = 3.0, 5.0, 1.0, 0.25
    xy, lp = _kp(heat.tolist(), n=None, window_size=3, score_threshold=0.25)
    assert xy == [[6, 0], [0, 4], [8, 8]] and lp == [3.0, 5.0, 1.0]  # row-major, not by score; 0.25 is not > 0.25


def test_n_plus_one_cutoff_quirks():
    heat = torch.zeros(1, 13)
    heat[0, ::3] = torch.tensor([4.0, 1.0, 3.0, 2.0, 5.0])
    # n = 2: the third largest (3.0) is the cut-off, kept strictly above it, row-major
    xy, lp = _kp(heat.tolist(), n=2, window_size=3, score_threshold=0.0)
    assert lp == [4.0, 5.0]
    # fewer than n + 1 candidates: every candidate equal to the minimum is dropped
    xy, lp = _kp(heat.tolist(), n=10, window_size=3, score_threshold=0.0)
    assert lp == [4.0, 3.0, 2.0, 5.0]
    # ties at the (n + 1)-th value are all dropped
    heat[0, ::3] = torch.tensor([4.0, 2.0, 2.0, 2.0, 5.0])
    xy, lp = _kp(heat.tolist(), n=2, window_size=3, score_threshold=0.0)
    assert lp == [4.0, 5.0]
    xy, lp = _kp(heat.tolist(), n=3, window_size=3, score_threshold=0.0)
    assert lp == [4.0, 5.0]


def test_zero_candidates_raise_in_the_reference():
    with pytest.raises((RuntimeError, IndexError)):
        _kp([[-1.0, -2.0]], n=5, window_size=3, score_threshold=0.0)
    assert _kp([[-1.0, -2.0]], n=None, window_size=3, score_threshold=0.0) == ([], [])


def test_refusals():
    from imcui_hip import backend

    m = Unet()
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 40, 48))  # not a multiple of 16
    with pytest.raises(ValueError):
        m(torch.zeros(1, 1, 32, 32))
    with pytest.raises(ValueError):
        nms(torch.zeros(1, 8, 8), window_size=4)
    with pytest.raises(ValueError):
        backend.disk_check_args((1, 3, 40, 48), 5, pad_if_not_divisible=False)
    with pytest.raises(ValueError):
        backend.disk_check_args((1, 3, 48, 48), 4, pad_if_not_divisible=True)
    with pytest.raises(ValueError):
        backend.disk_check_args((1, 1, 48, 48), 5, pad_if_not_divisible=True)
    backend.disk_check_args((1, 3, 40, 48), 5, pad_if_not_divisible=True)


def test_bound_is_exact_for_nms_survivors(lib):
    # a checkerboard of maxima every s pixels reaches the bound ceil(H / s) ceil(W / s), s = window // 2 + 1
    for window in (1, 3, 5):
        s = window // 2 + 1
        H, W = 13, 17
        heat = torch.zeros(H, W)
        heat[::s, ::s] = 1.0 + torch.arange(len(range(0, H, s)) * len(range(0, W, s)), dtype=torch.float32).reshape(len(range(0, H, s)), -1) * 1e-3
        xy, _ = _kp(heat.tolist(), n=None, window_size=window, score_threshold=0.0)
        assert len(xy) == lib.imcui_hip_disk_max_keypoints_bound(H, W, window) == -(-H // s) * -(-W // s)


def test_batch_driver_still_refuses_rgb_for_superpoint():
    from types import SimpleNamespace

    import numpy as np

    from imcui_hip.hloc import extract_features as ef

    conf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, "grayscale": False})
    with pytest.raises(NotImplementedError, match="gray"):
        ef.preprocess_on_device(np.zeros((8, 8, 3), np.uint8), conf, "cpu")
