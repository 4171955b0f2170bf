"""R2D2 without a GPU: the scale schedule against a literal restatement of extract_multiscale's loop, the strict packer (key names,
shapes, `module.` prefix, the 'net' string), the BatchNorm fold, the packed digest, the restatement against its own float64 run, the
seeded weights' thresholds and the plugin's contract."""
import hashlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

import r2d2_reference as R
from imcui_hip import backend
from imcui_hip.synth import make_pair_batch
from imcui_hip.synth_weights import r2d2_state_dict


def image(h, w, seed=0):
    """A seeded RGB image [1,3,h,w]: blobs on band-limited noise plus a little colour noise."""
    img = make_pair_batch(seed, 1, h, w, n_blobs=max(10, h * w // 250))[0].repeat(1, 3, 1, 1)
    g = torch.Generator().manual_seed(5 + seed)
    return (img + 0.15 * torch.rand(1, 3, h, w, generator=g)).clamp(0, 1)


# expected lists computed with the literal loop (float64, banker's round) for the default scale_factor 2 ** 0.25
SCHEDULES = {
    (768, 1024, 256): [(768, 1024), (646, 861), (543, 724), (457, 609), (384, 512), (323, 431), (272, 362), (228, 304), (192, 256)],
    (480, 640, 256): [(480, 640), (404, 538), (339, 453), (285, 381), (240, 320), (202, 269)],
    (48, 64, 16): [(48, 64), (40, 54), (34, 45), (29, 38), (24, 32), (20, 27), (17, 23), (14, 19), (12, 16)],
}


@pytest.mark.parametrize("key", list(SCHEDULES), ids=[f"{h}x{w}_min{m}" for h, w, m in SCHEDULES])
def test_level_schedule_is_upstreams_loop(key):
    H, W, min_size = key
    got = backend.r2d2_levels(H, W, 2**0.25, min_size, 1024, 0, 1)
    assert [(a, b) for a, b, _ in got] == SCHEDULES[key] and all(r for *_, r in got)
    assert got == R.schedule(H, W, 2**0.25, min_size, 1024, 0, 1)


def test_level_schedule_skips_levels_above_max_size_and_refuses_max_scale_above_one():
    got = backend.r2d2_levels(1200, 1600)
    assert got == R.schedule(1200, 1600, 2**0.25, 256, 1024, 0, 1)
    assert [r for *_, r in got] == [False] * 3 + [True] * 8 and got[3][:2] == (714, 951)  # levels are interpolated even when they do not run
    assert backend.r2d2_levels(100, 150, min_size=24, max_scale=0.5) == R.schedule(100, 150, 2**0.25, 24, 1024, 0, 0.5)
    with pytest.raises(ValueError, match="max_scale"):
        backend.r2d2_levels(480, 640, max_scale=1.5)
    with pytest.raises(ValueError, match="RGB"):
        backend.r2d2_check_args((1, 1, 64, 64), R.DEFAULT_CONF)
    with pytest.raises(ValueError, match="levels"):
        backend.r2d2_check_args((1, 3, 480, 640), {**R.DEFAULT_CONF, "scale_factor": 1.01, "min_size": 16})


def test_pack_is_strict(lib):
    sd = r2d2_state_dict(0)
    names = backend.r2d2_tensor_names()
    shapes = backend.r2d2_tensor_shapes()
    assert names == [k for k in sd if not k.endswith("num_batches_tracked")] and len(names) == 38
    assert {k: tuple(t.shape) for k, t in sd.items() if k in shapes} == shapes
    packed = backend.pack_r2d2(sd)
    assert packed.numel() == lib.imcui_hip_r2d2_packed_floats() > 0 and packed.dtype == torch.float32
    assert torch.equal(backend.pack_r2d2({k: t for k, t in sd.items() if not k.endswith("num_batches_tracked")}), packed)  # counters ignored
    assert torch.equal(backend.pack_r2d2(r2d2_state_dict(0, checkpoint=True)), packed)  # upstream's container, `module.` prefix
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_r2d2({k: t for k, t in sd.items() if k != "ops.21.running_var"})
    with pytest.raises(backend.ImcuiHipError, match="unexpected"):
        backend.pack_r2d2({**sd, "ops.1.weight": torch.ones(32)})  # an affine BatchNorm is another network
    with pytest.raises(backend.ImcuiHipError, match="shape"):
        backend.pack_r2d2({**sd, "ops.18.weight": torch.zeros(128, 128, 3, 3)})
    with pytest.raises(backend.ImcuiHipError, match="Fast_Quad_L2Net_ConfCFS"):
        backend.pack_r2d2({"net": "Fast_Quad_L2Net_ConfCFS()", "state_dict": sd})


def test_batchnorm_is_folded_into_the_first_convolution(lib):
    """The packed buffer begins with ops.0 folded with the affine-free BatchNorm ops.1 as [9][3][32] + 32 biases: a convolution with
    those equals eval-mode BatchNorm2d(conv(x)) evaluated in float64 to float32 round-off."""
    sd = r2d2_state_dict(0)
    packed = backend.pack_r2d2(sd)
    w = packed[: 27 * 32].reshape(3, 3, 3, 32).permute(3, 2, 0, 1).contiguous().double()  # [ky][kx][ci][co] -> OIHW
    off_b = (27 * 32 + 63) // 64 * 64
    b = packed[off_b : off_b + 32].double()
    x = torch.randn(1, 3, 20, 24, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    bn = torch.nn.BatchNorm2d(32, affine=False).double().eval()
    bn.running_mean.copy_(sd["ops.1.running_mean"])
    bn.running_var.copy_(sd["ops.1.running_var"])
    want = bn(F.conv2d(x, sd["ops.0.weight"].double(), sd["ops.0.bias"].double(), padding=1))
    got = F.conv2d(x, w, b, padding=1)
    err = (want - got).abs().max().item() / want.abs().max().item()
    print(f"folded ops.0 against BatchNorm2d in float64: {err:.2e}")
    assert err < 1e-6


def test_packed_buffer_is_byte_identical(lib, golden_dir):
    with open(os.path.join(golden_dir, "r2d2_packed_digest.json")) as f:
        golden = json.load(f)
    buf = backend.pack_r2d2(r2d2_state_dict(0)).numpy()
    assert buf.size == golden["floats"]
    assert hashlib.sha256(buf.tobytes()).hexdigest() == golden["sha256"]


def test_every_map_keeps_the_input_size():
    sd = R.strip(r2d2_state_dict(0))
    for h, w in ((13, 17), (24, 40)):
        r = R.network(sd, torch.rand(1, 3, h, w))
        assert r["map"].shape == (1, 128, h, w) and r["reliability"].shape == r["repeatability"].shape == (1, h, w)


def test_restatement_fp32_against_its_own_fp64_and_thresholds_cut():
    """100 x 150 with min_size 24: at least 200 key-points over at least four levels; both default thresholds fall inside the maps'
    distributions; float32 and float64 runs of the restatement select the same key-points up to the 1 % cap the GPU test allows."""
    sd, img = r2d2_state_dict(0), image(100, 150)
    conf = {"min_size": 24, "max_keypoints": 0}
    a, b = R.extract(sd, img, conf), R.extract(sd, img, conf, torch.float64)
    rel, rep = torch.cat([m.flatten() for m in a["reliability"]]), torch.cat([m.flatten() for m in a["repeatability"]])
    for name, m in (("reliability", rel), ("repeatability", rep)):
        frac = (m >= 0.7).float().mean().item()
        print(f"{name}: {frac:.2f} of the pixels at or above 0.7")
        assert 0.05 < frac < 0.95, (name, frac)
    n, per_level = a["scores"].numel(), torch.bincount(a["level"])
    sa, sb = set(zip(a["level"].tolist(), a["index"].tolist())), set(zip(b["level"].tolist(), b["index"].tolist()))
    print(f"{n} key-points over {int((per_level > 0).sum())} levels; float32 and float64 differ in {len(sa ^ sb)}")
    assert n >= 200 and int((per_level > 0).sum()) >= 4
    assert len(sa ^ sb) <= 0.01 * n
    assert torch.all(a["scores"][1:] >= a["scores"][:-1])  # ascending
    for x, y in zip(a["final_map"], b["final_map"]):
        assert (x.double() - y).abs().max().item() < 1e-4 * y.abs().max().item()
    common = sorted(sa & sb)
    ia = {k: i for i, k in enumerate(zip(a["level"].tolist(), a["index"].tolist()))}
    ib = {k: i for i, k in enumerate(zip(b["level"].tolist(), b["index"].tolist()))}
    da, db = a["descriptors"][[ia[k] for k in common]], b["descriptors"][[ib[k] for k in common]]
    assert (da.double() - db).abs().max().item() < 1e-4


def test_cut_keeps_the_later_of_tied_scores():
    s = torch.tensor([0.5, 0.9, 0.5, 0.5, 0.1])
    assert R.cut(s, 3).tolist() == [2, 3, 1] and R.cut(s, 0).tolist() == [4, 0, 2, 3, 1]


def test_plugin_contract_and_refusals():
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.extractors.r2d2 import R2D2
    from imcui_hip.hloc.utils.base_model import dynamic_load

    assert dynamic_load(extractors, "r2d2") is R2D2
    assert R2D2.default_conf == {"model_name": "r2d2_WASF_N16.pt", "max_keypoints": 5000, "scale_factor": 2**0.25, "min_size": 256, "max_size": 1024,
                                 "min_scale": 0, "max_scale": 1, "reliability_threshold": 0.7, "repetability_threshold": 0.7}  # fmt: skip
    assert R2D2.required_inputs == ["image"] and R2D2.takes_rgb
    m = R2D2({"name": "r2d2", "state_dict": r2d2_state_dict(0, checkpoint=True)})
    assert "state_dict" not in m.conf and m.packed.dtype == torch.float32 and not m.packed.is_cuda
    with pytest.raises(backend.ImcuiHipError, match="faster2d2"):
        R2D2({"state_dict": {"net": "Fast_Quad_L2Net_ConfCFS()", "state_dict": r2d2_state_dict(0)}})
    with pytest.raises(ValueError, match="max_scale"):
        R2D2({"state_dict": r2d2_state_dict(0), "max_scale": 2})
    with pytest.raises(backend.ImcuiHipError, match="ROCm device"):  # no CPU fallback
        m({"image": torch.zeros(1, 3, 64, 64)})
    with pytest.raises(ValueError, match="RGB"):
        m({"image": torch.zeros(1, 1, 64, 64)})
