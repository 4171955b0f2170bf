"""XFeat without a GPU (imcui/hloc/extractors/xfeat.py:8-34 -> verlab/accelerated_features): the restatement's index conventions, its
NMS against a brute-force scan, the three quirks of detectAndCompute on constructed maps, the library's packing table and BatchNorm
fold, the plugin's reference seam, and the synthetic weights' key-point count on the seeded image."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import xfeat_reference as xr


def _image(h, w, seed):
    """Seeded RGB in [0, 1]: smooth structure at several scales + a little pixel noise (as tests/test_gpu_disk.py::_image)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.zeros(1, 3, h, w)
    for s, a in ((8, 0.5), (32, 0.3), (128, 0.2)):
        low = torch.rand(1, 3, max(2, h // s), max(2, w // s), generator=g)
        img += a * F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)
    return (img + 0.02 * torch.rand(1, 3, h, w, generator=g)).clamp(0, 1)


@functools.lru_cache(maxsize=None)
def _sd():
    from imcui_hip.synth_weights import xfeat_state_dict

    return xfeat_state_dict(0)


def test_unfold8_is_pixel_unshuffle_and_the_heatmap_unshuffle_is_its_inverse():
    x = torch.arange(2 * 1 * 16 * 24, dtype=torch.float32).reshape(2, 1, 16, 24)
    u = xr.unfold8(x)
    assert u.shape == (2, 64, 2, 3)
    assert torch.equal(u, F.pixel_unshuffle(x, 8))
    assert u[1, 3 * 8 + 5, 1, 2] == x[1, 0, 8 + 3, 16 + 5]  # channel = dy * 8 + dx
    assert torch.equal(xr.unshuffle_heatmap(u), x)
    assert torch.equal(xr.unshuffle_heatmap(u), F.pixel_shuffle(u, 8))


def _brute_nms(m, thr):
    H, W = m.shape
    out = []
    for y in range(H):
        for x in range(W):
            win = m[max(0, y - 2) : y + 3, max(0, x - 2) : x + 3]
            if m[y, x] == win.max() and m[y, x] > thr:
                out.append((x, y))
    return out


def test_nms_equals_a_brute_force_scan_and_keeps_every_member_of_a_plateau():
    g = torch.Generator().manual_seed(3)
    m = torch.rand(24, 40, generator=g)
    m[5:7, 10:13] = 2.0  # an exact plateau of six pixels: every member equals its window's maximum
    m[20, 39] = 3.0
    got = [tuple(p) for p in xr.nms(m[None, None], threshold=0.6)[0].tolist()]
    assert got == _brute_nms(m, 0.6)  # row-major (x, y)
    assert {(x, y) for x in (10, 11, 12) for y in (5, 6)} <= set(got)
    assert (39, 20) in got and all(m[y, x] > 0.6 for x, y in got)


def _maps(H, W, peaks, rel=0.5):
    """K1h with the given {(x, y): value} peaks on a 0.01 floor, a constant reliability map and a random unit-norm M1."""
    K1h = torch.full((1, 1, H, W), 0.01)
    for (x, y), v in peaks.items():
        K1h[0, 0, y, x] = v
    H1 = torch.full((1, 1, H // 8, W // 8), rel)
    M1 = F.normalize(torch.randn(1, 64, H // 8, W // 8, generator=torch.Generator().manual_seed(0)), dim=1)
    return M1, K1h, H1


def test_the_three_quirks_of_detect_and_compute():
    H, W = 64, 96
    peaks = {(10, 10): 0.9, (30, 20): 0.8, (50, 40): 0.7, (70, 50): 0.6}
    base = xr.select(*_maps(H, W, peaks), 1.0, 1.0, top_k=100)
    assert [tuple(p) for p in base["xy"].tolist()] == [(10, 10), (30, 20), (50, 40), (70, 50)]
    assert torch.allclose(base["scores"], torch.tensor([0.45, 0.4, 0.35, 0.3]), atol=1e-6)
    assert torch.allclose(base["descriptors"].norm(dim=1), torch.ones(4), atol=1e-6)
    # (1) the nearest sample of the last column / row rounds half-to-even OUT of the map and reads zero: score 0, dropped by score > 0
    for edge in ((W - 1, 30), (40, H - 1), (W - 1, H - 1)):
        out = xr.select(*_maps(H, W, {**peaks, edge: 0.95}), 1.0, 1.0, top_k=100)
        assert [tuple(p) for p in out["xy"].tolist()] == [tuple(p) for p in base["xy"].tolist()], edge
    # ... while the column / row before it stays (with a lower score: the bilinear sample of the reliability map meets the zero padding)
    out = xr.select(*_maps(H, W, {**peaks, (W - 2, H - 2): 0.95}), 1.0, 1.0, top_k=100)
    assert (W - 2, H - 2) in [tuple(p) for p in out["xy"].tolist()] and len(out["xy"]) == 5
    # (2) a key-point at exactly (0, 0) is taken for padding
    out = xr.select(*_maps(H, W, {**peaks, (0, 0): 0.95}), 1.0, 1.0, top_k=100)
    assert [tuple(p) for p in out["xy"].tolist()] == [tuple(p) for p in base["xy"].tolist()]
    out = xr.select(*_maps(H, W, {**peaks, (1, 0): 0.95}), 1.0, 1.0, top_k=100)
    assert (1, 0) in [tuple(p) for p in out["xy"].tolist()] and len(out["xy"]) == 5
    # (3) top_k = -1 is Python's [:-1]: exactly the lowest score goes
    out = xr.select(*_maps(H, W, peaks), 1.0, 1.0, top_k=-1)
    assert [tuple(p) for p in out["xy"].tolist()] == [(10, 10), (30, 20), (50, 40)]
    # key-points are scaled by (rw, rh)
    out = xr.select(*_maps(H, W, peaks), 1.5, 1.25, top_k=100)
    assert torch.equal(out["keypoints"], base["xy"].float() * torch.tensor([1.25, 1.5]))


def test_pack_weights_names_and_the_folded_first_layer(lib):
    from imcui_hip import backend

    sd = _sd()
    names = backend.xfeat_tensor_names()
    assert names == [k for k in sd if not k.endswith("num_batches_tracked") and not k.startswith("fine_matcher.")]
    assert any(k.startswith("fine_matcher.") for k in sd) and any(k.endswith("num_batches_tracked") for k in sd)
    assert backend.xfeat_tensor_shapes() == {k: tuple(sd[k].shape) for k in names}
    assert set(names) == {k for k in xr.XFeatModel().state_dict() if not k.endswith("num_batches_tracked")}
    p = backend.pack_xfeat(sd).numpy()
    assert p.dtype == np.float32 and p.size == lib.imcui_hip_xfeat_packed_floats()
    # block1.0 at float 0 as [9 taps][4], its folded bias from float 64: w / sqrt(var + eps), -mean / sqrt(var + eps)
    w = sd["block1.0.layer.0.weight"].numpy().astype(np.float64)
    var = sd["block1.0.layer.1.running_var"].numpy().astype(np.float64)
    mean = sd["block1.0.layer.1.running_mean"].numpy().astype(np.float64)
    want_w = (w / np.sqrt(var + 1e-5)[:, None, None, None])[:, 0].reshape(4, 9).T.reshape(-1)
    want_b = -mean / np.sqrt(var + 1e-5)
    for got, want in ((p[:36], want_w), (p[64:68], want_b)):
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got.astype(np.float64) - want) <= ulp), np.abs(got - want).max()
    # strict on the network's own keys
    with pytest.raises(backend.ImcuiHipError):
        backend.pack_xfeat({k: v for k, v in sd.items() if k != "block3.1.layer.0.weight"})
    with pytest.raises(backend.ImcuiHipError):
        backend.pack_xfeat({**sd, "block9.0.layer.0.weight": torch.zeros(1)})
    with pytest.raises(backend.ImcuiHipError):
        backend.pack_xfeat({**sd, "skip1.1.bias": torch.zeros(23)})


def test_plugin_keeps_the_reference_seam_and_refuses_the_cpu(lib):
    from imcui_hip import backend
    from imcui_hip.hloc.extractors.xfeat import XFeat

    assert XFeat.default_conf == {"keypoint_threshold": 0.005, "max_keypoints": -1}
    assert XFeat.required_inputs == ["image"]
    assert XFeat.takes_rgb is True
    assert XFeat.__module__.rsplit(".", 1)[-1] == "xfeat"
    m = XFeat({"state_dict": _sd()}).eval()
    assert "state_dict" not in m.conf and m.packed.numel() == lib.imcui_hip_xfeat_packed_floats()
    with pytest.raises(backend.ImcuiHipError):
        m({"image": torch.rand(1, 3, 64, 64)})  # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        backend.xfeat_check_args((1, 2, 64, 64))
    with pytest.raises(ValueError):
        backend.xfeat_check_args((1, 3, 31, 64))
    assert lib.imcui_hip_xfeat_workspace_bytes(2, 480, 640) > 0 and lib.imcui_hip_xfeat_workspace_bytes(1, 16, 640) == 0
    assert lib.imcui_hip_xfeat_max_keypoints_bound(100, 150) == 32 * 43  # 96 x 128 after the resize


@functools.lru_cache(maxsize=None)
def _seeded_run(threads: int):
    old = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        net = xr.load_model(_sd())
        img = _image(480, 640, 0)
        m = xr.dense_maps(net, img)
        return m, xr.select(m["M1"], m["K1h"], m["reliability"], m["rh"], m["rw"], top_k=-1)
    finally:
        torch.set_num_threads(old)


def test_synthetic_weights_give_a_useful_keypoint_set_on_the_seeded_image():
    m, out = _seeded_run(1)
    n = len(out["scores"])
    assert 300 <= n <= 480 * 640 // 100, n
    rel = m["reliability"]
    assert rel.min() < 0.2 and rel.max() > 0.8 and 0.3 < rel.mean() < 0.7, (rel.min().item(), rel.mean().item(), rel.max().item())
    # the threshold cuts inside the distribution of the NMS maxima
    all_max = len(xr.nms(m["K1h"], threshold=0.0)[0])
    assert n < 0.5 * all_max, (n, all_max)
    assert torch.all(out["scores"][1:] <= out["scores"][:-1]) and out["scores"][-1] > 0


def test_restatement_keypoints_are_stable_across_thread_counts():
    """The cap the GPU test puts on end-to-end differences, max(2, 1 %), holds for the reference against itself."""
    a = {tuple(p) for p in _seeded_run(1)[1]["xy"].tolist()}
    b = {tuple(p) for p in _seeded_run(8)[1]["xy"].tolist()}
    assert len(a ^ b) <= max(2, 0.01 * len(a)), (len(a ^ b), len(a))
