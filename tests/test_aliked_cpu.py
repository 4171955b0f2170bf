"""ALIKED without a GPU: the restatement's layout against the seeded weights and the library's tensor table, the pieces of the
restatement the GPU tests lean on (deformable convolution, the branch-wise first score-head layer, the DKD rules), strict packing
with BatchNorm folding, the workspace condition, the seeded score head's operating point and the plugin's contract / refusals."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from aliked_reference import ALIKEDReference, deform_conv2d_ref, dkd_refine, dkd_select, simple_nms
from imcui_hip import backend
from imcui_hip.synth_weights import aliked_state_dict


def image(h, w, seed):
    """Seeded RGB in [0, 1]: smooth structure at several scales + a little pixel noise (the image family of the GPU tests)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.zeros(1, 3, h, w)
    for s, a in ((8, 0.5), (32, 0.3), (128, 0.2)):
        low = torch.rand(1, 3, max(2, h // s), max(2, w // s), generator=g)
        img += a * F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)
    return (img + 0.02 * torch.rand(1, 3, h, w, generator=g)).clamp(0, 1)


@functools.lru_cache(maxsize=None)
def _sd():
    return aliked_state_dict(0)


@functools.lru_cache(maxsize=None)
def _ref():
    return ALIKEDReference(_sd())


# ------------------------------------------------------------------ layout
def test_seeded_weights_load_strictly_and_match_the_library_table(lib):
    ref = ALIKEDReference()
    missing, unexpected = ref.load_state_dict(_sd(), strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    keys = [k for k in ref.state_dict() if not k.endswith("num_batches_tracked")]
    assert backend.aliked_tensor_names() == keys
    assert len(keys) == 65
    shapes = backend.aliked_tensor_shapes()
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items() if k in shapes} == shapes
    for name in ("block1.bn1", "block3.bn2"):  # running statistics that are not the identity
        assert (_sd()[f"{name}.running_mean"].abs() > 0.01).any() and ((_sd()[f"{name}.running_var"] - 1).abs() > 0.05).any()


# ------------------------------------------------------------------ the restatement's deformable convolution
def test_deform_conv_with_zero_offsets_is_conv2d():
    """In float64, so that the comparison is to 1 ulp and not a statement about two fp32 summation orders (the restatement
    multiplies a gathered [C k k, H W] matrix, F.conv2d does not): at fp32 the two differ by 3.5 ulp of the largest output."""
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(2, 8, 9, 11, generator=g).double(), torch.randn(6, 8, 3, 3, generator=g).double()
    out = deform_conv2d_ref(x, torch.zeros(2, 18, 9, 11, dtype=torch.float64), w)
    ref = F.conv2d(x, w, padding=1)
    assert (out - ref).abs().max().item() <= torch.finfo(torch.float64).eps * ref.abs().max().item()


def test_deform_conv_with_integer_offsets_is_a_shifted_tap_convolution():
    """Tap k reads x[y - 1 + ky + dy_k, x - 1 + kx + dx_k] with dy_k in offset channel 2k and dx_k in 2k + 1 (torchvision's order),
    zero outside the map: compared with shifting zero-padded copies of the input tap by tap."""
    g = torch.Generator().manual_seed(2)
    H, W = 10, 12
    x, w = torch.randn(1, 4, H, W, generator=g), torch.randn(5, 4, 3, 3, generator=g)
    shifts = [(2, -1), (0, 3), (-3, 0), (1, 1), (0, 0), (-2, 2), (4, -4), (-1, -1), (0, -5)]  # (dy, dx) per tap
    off = torch.zeros(1, 18, H, W)
    for k, (dy, dx) in enumerate(shifts):
        off[0, 2 * k], off[0, 2 * k + 1] = dy, dx
    out = deform_conv2d_ref(x, off, w)
    P = 8
    xp = F.pad(x, (P, P, P, P))
    ref = torch.zeros(1, 5, H, W)
    for k, (dy, dx) in enumerate(shifts):
        ky, kx = k // 3, k % 3
        win = xp[:, :, P - 1 + ky + dy : P - 1 + ky + dy + H, P - 1 + kx + dx : P - 1 + kx + dx + W]
        ref += torch.einsum("oc,bchw->bohw", w[:, :, ky, kx], win)
    assert (out - ref).abs().max().item() < 1e-5


def test_score_head_first_layer_branchwise_equals_the_concatenated_form():
    """The re-association the HIP path makes (W_a f1 + up2(W_b f2) + up8(W_c f3) + up32(W_d f4)); its error is recorded here."""
    ref = _ref()
    img, _ = ref.pad(image(96, 128, 3))
    _, f = ref.branches(img)
    up = [f[0]] + [F.interpolate(t, scale_factor=s, mode="bilinear", align_corners=True) for t, s in zip(f[1:], (2, 8, 32))]
    cat = ref.score_head[0](torch.cat(up, 1))
    bw = ref.score_head0_branchwise(f)
    err = (cat - bw).abs().max().item()
    print(f"branch-wise vs concatenated score_head.0: {err:.2e} at scale {cat.abs().max().item():.2f}")
    assert err < 1e-5 * max(1.0, cat.abs().max().item())


# ------------------------------------------------------------------ packing
def test_pack_is_strict(lib):
    sd = dict(_sd())
    packed = backend.pack_aliked(sd)
    assert packed.numel() == lib.imcui_hip_aliked_packed_floats()
    sd_counters = {**sd, "block1.bn1.num_batches_tracked": torch.tensor(7)}
    assert torch.equal(backend.pack_aliked(sd_counters), packed)  # ignored
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_aliked({k: v for k, v in sd.items() if k != "block3.conv1.offset_conv.bias"})
    with pytest.raises(backend.ImcuiHipError, match="unexpected"):
        backend.pack_aliked({**sd, "desc_head.mask_conv.weight": torch.zeros(1)})
    with pytest.raises(backend.ImcuiHipError, match="shape"):
        backend.pack_aliked({**sd, "conv4.weight": torch.zeros(32, 64, 1, 1)})
    for name in ("aliked-t16", "aliked-n32", "aliked-x"):
        with pytest.raises(backend.ImcuiHipError, match="not served"):
            backend.pack_aliked(sd, name)


def test_batchnorm_is_folded_into_the_first_convolution(lib):
    """The packed buffer begins with block1.conv1 folded with block1.bn1 as [9][3][16] + 16 biases (include/imcui_hip.h): a
    convolution with those equals the restatement's bn1(conv1(x))."""
    packed = backend.pack_aliked(_sd())
    w = packed[: 9 * 3 * 16].reshape(3, 3, 3, 16).permute(3, 2, 0, 1).contiguous()  # [ky][kx][ci][co] -> OIHW
    b = packed[448 : 448 + 16]
    x = torch.randn(1, 3, 20, 24, generator=torch.Generator().manual_seed(4))
    ref = _ref()
    want = ref.block1.bn1(ref.block1.conv1(x))
    got = F.conv2d(x, w, b, padding=1)
    assert (want - got).abs().max().item() < 1e-5


# ------------------------------------------------------------------ workspace and bounds
@pytest.mark.parametrize("hw", [(480, 640), (768, 1024), (472, 632)])
def test_workspace_is_smaller_than_one_dense_128_channel_map(lib, hw):
    H, W = hw
    Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    for B in (1, 8):
        ws = lib.imcui_hip_aliked_workspace_bytes(B, H, W)
        assert 0 < ws < B * Hp * Wp * 128 * 4, (ws, B * Hp * Wp * 128 * 4)
        print(f"{H}x{W} B={B}: {ws / (B * Hp * Wp * 4):.1f} floats per padded pixel")


def test_max_keypoints_bound_covers_the_restatements_nms_survivors(lib):
    sm = _ref().dense(image(480, 640, 0))["score_map"]
    for r in (1, 2, 3):
        surv = int((simple_nms(sm, r) > 0).sum())
        assert surv <= lib.imcui_hip_aliked_max_keypoints_bound(480, 640, r), r


# ------------------------------------------------------------------ DKD rules on hand-made maps
def _flat_map(h=24, w=32, base=0.1):
    return torch.full((h, w), base)


def test_threshold_is_strict_and_order_is_row_major():
    sm = _flat_map()
    for (y, x), v in {(5, 20): 0.5, (5, 6): 0.2, (12, 12): 0.9, (18, 3): 0.3}.items():
        sm[y, x] = v
    idx, branch = dkd_select(sm, 2, 0.2, -1)
    assert branch == "threshold" and idx.tolist() == [5 * 32 + 20, 12 * 32 + 12, 18 * 32 + 3]  # 0.2 itself is not > 0.2


def test_border_of_radius_pixels_is_removed():
    sm = _flat_map()
    sm[1, 10] = sm[10, 1] = sm[22, 10] = sm[10, 30] = 0.9  # inside the 2-pixel border
    sm[2, 10] = 0.8  # suppressed by (1, 10), which then leaves with the border
    sm[12, 16] = 0.7
    idx, _ = dkd_select(sm, 2, 0.2, -1)
    assert idx.tolist() == [12 * 32 + 16]


def test_mean_fallback_when_nothing_passes_the_threshold():
    sm = _flat_map(base=0.05)
    sm[8, 8], sm[16, 20] = 0.15, 0.12
    idx, branch = dkd_select(sm, 2, 0.2, -1)
    assert branch == "mean" and idx.tolist() == [8 * 32 + 8, 16 * 32 + 20]


def test_n_limit_cut_keeps_the_highest_and_breaks_a_tie_by_index():
    sm = _flat_map()
    pts = {(4, 4): 0.9, (4, 14): 0.5, (10, 8): 0.5, (16, 20): 0.5, (20, 28): 0.7}
    for (y, x), v in pts.items():
        sm[y, x] = v
    idx, _ = dkd_select(sm, 2, 0.2, 3)
    assert idx.tolist() == [4 * 32 + 4, 4 * 32 + 14, 20 * 32 + 28]  # of the three 0.5s the lowest index stays
    idx, branch = dkd_select(sm, 2, -1.0, 2)
    assert branch == "topk" and idx.tolist() == [4 * 32 + 4, 20 * 32 + 28]


def test_refinement_moves_towards_the_heavier_neighbour():
    sm = _flat_map(base=0.0)
    sm[10, 10], sm[10, 11] = 0.6, 0.5
    kn, ks = dkd_refine(sm, torch.tensor([10 * 32 + 10]), 2)
    xy = (kn[0] + 1) / 2 * torch.tensor([31.0, 23.0])
    assert 10.0 < xy[0].item() < 10.5 and abs(xy[1].item() - 10.0) < 1e-5 and 0.5 < ks[0].item() < 0.6


# ------------------------------------------------------------------ the seeded score head's operating point
def test_default_threshold_decides_on_the_seeded_network():
    """At 480x640 the 0.2 threshold keeps between 5 % and 90 % of the NMS survivors, max_num_keypoints 300 takes the n_limit cut,
    and a score map that stays below the threshold takes the mean fallback."""
    ref = _ref()
    sm = ref.dense(image(480, 640, 0))["score_map"][0, 0]
    nms = simple_nms(sm[None, None], 2)[0, 0]
    nms[:2], nms[-2:], nms[:, :2], nms[:, -2:] = 0, 0, 0, 0
    surv, above = int((nms > 0).sum()), int((nms > 0.2).sum())
    print(f"{surv} NMS survivors, {above} above 0.2, score mean {sm.mean().item():.3f}")
    assert 0.05 * surv < above < 0.9 * surv
    assert above > 300 and dkd_select(sm, 2, 0.2, 300)[0].numel() == 300
    # the mean fallback: zero-padded convolutions raise the scores along the border of ANY image, a flat one included, so the
    # "nothing above the threshold" map is made with the seeded weights' logit shift instead (the same trunk, logits 3 lower)
    low = ALIKEDReference(aliked_state_dict(0, score_shift=-6.6)).dense(image(96, 128, 3))["score_map"][0, 0]
    idx, branch = dkd_select(low, 2, 0.2, -1)
    assert branch == "mean" and low.max().item() < 0.2 and 0 < idx.numel() < int((simple_nms(low[None, None], 2) > 0).sum())


@pytest.mark.parametrize("h,w,seed", [(480, 640, 0), (472, 632, 1), (768, 1024, 2)])
def test_restatement_is_stable_across_thread_counts(h, w, seed):
    """The end-to-end GPU test audits differing key-points as ties and caps them at 1 %: the restatement itself, evaluated at 1 and
    8 intra-op threads, has to sit far below that (a tenth of the cap) on every image the GPU cases use."""
    ref, img = _ref(), image(h, w, seed)
    old = torch.get_num_threads()
    sets, maps = [], []
    try:
        for t in (1, 8):
            torch.set_num_threads(t)
            sm = ref.dense(img)["score_map"][0, 0]
            maps.append(sm)
            sets.append(set(dkd_select(sm, 2, 0.2, -1)[0].tolist()))
    finally:
        torch.set_num_threads(old)
    diff = len(sets[0] ^ sets[1])
    print(f"{h}x{w}: score map spread {(maps[0] - maps[1]).abs().max().item():.2e}, {diff} of {len(sets[0])} key-points differ")
    assert diff <= 0.001 * len(sets[0])


# ------------------------------------------------------------------ plugin contract
def test_plugin_contract_and_refusals():
    from imcui_hip.hloc.extractors.aliked import ALIKED
    from imcui_hip.hloc.utils.base_model import dynamic_load
    from imcui_hip.hloc import extractors

    assert dynamic_load(extractors, "aliked") is ALIKED
    assert ALIKED.default_conf == {"model_name": "aliked-n16", "max_num_keypoints": -1, "detection_threshold": 0.2, "nms_radius": 2}
    assert ALIKED.required_inputs == ["image"] and ALIKED.takes_rgb
    m = ALIKED({"name": "aliked", "state_dict": _sd()})
    assert "state_dict" not in m.conf and m.packed.dtype == torch.float32 and not m.packed.is_cuda
    assert ALIKED({"model_name": "aliked-n16rot", "state_dict": _sd()}).packed.numel() == m.packed.numel()
    for name in ("aliked-t16", "aliked-n32", "superpoint"):
        with pytest.raises(backend.ImcuiHipError, match="not served"):
            ALIKED({"model_name": name, "state_dict": _sd()})
    for variant in ("mask", "conv2D"):
        with pytest.raises(backend.ImcuiHipError, match=variant):
            ALIKED({variant: True, "state_dict": _sd()})
    for r in (0, 5):
        with pytest.raises(ValueError, match="nms_radius"):
            ALIKED({"nms_radius": r, "state_dict": _sd()})
    with pytest.raises(backend.ImcuiHipError, match="ROCm device"):  # no CPU fallback
        m({"image": torch.zeros(1, 3, 64, 64)})
    with pytest.raises(ValueError, match="RGB"):
        backend.aliked_check_args((1, 2, 64, 64), 2)
    with pytest.raises(AssertionError):
        m({})


def test_aliked_conf_runs_on_the_device_resize():
    """`aliked-n16` (grayscale False, resize_max 1024, no force_resize): the batch extractor's device preprocessing takes it."""
    from types import SimpleNamespace

    from imcui_hip.hloc import extract_features as ef

    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, "grayscale": False, "resize_max": 1024})
    assert ef.target_size((1600, 1200), pconf) == (1024, 768)
    assert ef.target_size((640, 480), pconf) is None
