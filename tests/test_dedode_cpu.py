"""DeDoDe without a GPU: the restatement's float32 run against its float64 run at the GPU test sizes (where the 2 % cap of
tests/test_gpu_dedode.py is checked for the restatement alone), its explicit-order detection arithmetic against upstream's library form,
the strict packer (widths read from the tensors), the packed digest, the plugin's contract against values recorded in
tests/golden/dedode_confs.json, the refusals, the grid convention and the tie rule at the cut."""
import functools
import hashlib
import json
import os

import pytest
import torch

import dedode_reference as R
from imcui_hip import backend
from imcui_hip.synth_weights import DEDODE_REFINERS, dedode_state_dicts

SIZES = ((32, 48), (40, 56), (96, 128))
K = 64  # the cut of the end-to-end GPU test
CAP = 0.02  # key-points present in one of two runs only, as a share of k


def image(h, w, seed=0):
    """A seeded uniform-random RGB image [1,3,h,w]."""
    return torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(100 + seed))


@functools.lru_cache(maxsize=None)
def sds():
    return dedode_state_dicts(0)


@functools.lru_cache(maxsize=None)
def reference(hw, dtype=torch.float32, k=K, form=R.scores_explicit):
    return R.extract(*sds(), image(*hw), {"max_keypoints": k}, dtype, form)


def only_one(a, b):
    return set(a["idx"].tolist()) ^ set(b["idx"].tolist())


@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_float32_and_float64_restatements_agree(hw):
    a, b = reference(hw), reference(hw, torch.float64)
    e_map = max((x.double() - y).abs().max().item() / y.abs().max().item() for x, y in zip(a["logits"], b["logits"]))
    e_logp = (a["logp"].double() - b["logp"]).abs().max().item()
    e_desc = (a["dense"].double() - b["dense"]).abs().max().item() / b["dense"].abs().max().item()
    diff = only_one(a, b)
    spread = b["logits"][-1].max().item() - b["logits"][-1].min().item()
    print(f"{hw}: logits {e_map:.1e} (full-resolution range {spread:.1f}), log p {e_logp:.1e}, description grid {e_desc:.1e}; "
          f"{len(diff) // 2} of {K} key-points differ between float32 and float64")  # fmt: skip
    assert e_map < 1e-5 and e_logp < 1e-3 and e_desc < 1e-5
    assert 3 < spread < 60, "the seeded logits spread over a few units and the soft-max is not one saturated peak"
    assert len(diff) // 2 <= CAP * K, "the restatement alone stays within the cap of the GPU test at this size, seed and k"
    assert torch.all(a["scores"][:-1] >= a["scores"][1:])
    assert a["keypoints"].shape == (K, 2) and a["descriptors"].shape == (K, 256)


@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_explicit_order_and_library_forms_select_the_same(hw):
    a, b = reference(hw), reference(hw, form=R.scores_library)
    rel = ((a["score"] - b["score"]).abs() / b["score"]).max().item()
    print(f"{hw}: explicit and library scores differ by {rel:.1e} (relative), {len(only_one(a, b)) // 2} key-points differ")
    assert rel < 1e-4
    assert not only_one(a, b)
    assert (a["logp"] - b["logp"]).abs().max().item() < 1e-4


def test_written_out_exp_is_float32_grade():
    x = torch.linspace(-90, 2, 200001)
    got, want = R.exp_explicit(x).double(), torch.exp(x.double().clamp(min=-80))
    assert ((got - want).abs() / want).max().item() < 3e-7


def test_grid_convention_and_pixel_coordinates():
    H, W = 40, 56
    idx = torch.tensor([0, 1, W, H * W - 1])
    g = R.grid_coords(idx, H, W)
    lin_x, lin_y = torch.linspace(-1 + 1 / W, 1 - 1 / W, W), torch.linspace(-1 + 1 / H, 1 - 1 / H, H)  # get_grid
    assert torch.allclose(g[:, 0], lin_x[[0, 1, 0, W - 1]], atol=1e-6) and torch.allclose(g[:, 1], lin_y[[0, 0, 1, H - 1]], atol=1e-6)
    px = R.to_pixel_coords(g, H, W)
    assert torch.allclose(px, torch.tensor([[0.5, 0.5], [1.5, 0.5], [0.5, 1.5], [W - 0.5, H - 0.5]]), atol=1e-4)
    # grid_sample (align_corners=False) at a pixel centre returns that pixel
    grid = torch.randn(256, H, W, generator=torch.Generator().manual_seed(1))
    d = R.describe(grid, g)
    want = grid.reshape(256, -1)[:, idx].t()
    assert (d - want).abs().max().item() < 1e-4


def test_cut_gives_equal_scores_to_the_lower_index_and_refuses_k_above_the_pixels():
    s = torch.tensor([[0.5, 0.9, 0.5], [0.5, 0.1, 0.9]])
    assert R.cut(s, 4).tolist() == [1, 5, 0, 2] and R.cut(s, 6).tolist() == [1, 5, 0, 2, 3, 4]
    assert R.cut(torch.full((4, 6), 0.25), 5).tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(RuntimeError, match="out of range"):
        R.cut(s, 7)


def test_pack_is_strict(lib):
    det, desc = sds()
    packed, dims = backend.pack_dedode(det, desc)
    assert dims == (512, 512, 257, 8, 512, 256, 129, 8, 256, 128, 65, 8, 128, 64, 2, 8,
                    512, 512, 512, 5, 512, 256, 384, 5, 256, 64, 288, 5, 96, 32, 257, 5)  # fmt: skip
    names, shapes = backend.dedode_tensor_names(dims), backend.dedode_tensor_shapes(dims)
    want = [f"{m}.{k}" for m, sd in zip(backend.DEDODE_MODELS, (det, desc)) for k in sd if not k.endswith("num_batches_tracked")] + ["density_taps"]
    assert names == want and set(shapes) == set(names)
    for m, sd in zip(backend.DEDODE_MODELS, (det, desc)):
        assert all(tuple(t.shape) == shapes[f"{m}.{k}"] for k, t in sd.items() if not k.endswith("num_batches_tracked"))
    cd = backend._dedode_cdims(dims)
    assert packed.numel() == lib.imcui_hip_dedode_packed_floats(cd) > 0 and packed.dtype == torch.float32
    assert torch.equal(packed[-64:-13], backend.dedode_density_taps())  # the 51 taps close the buffer (slots of 64 floats)
    k = "decoder.layers.4.hidden_blocks.3.3.weight"
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_dedode({n: t for n, t in det.items() if n != k}, desc)
    with pytest.raises(backend.ImcuiHipError, match="unexpected"):
        backend.pack_dedode(det, {**desc, "decoder.layers.1.block1.4.weight": torch.ones(32, 32, 1, 1)})
    with pytest.raises(backend.ImcuiHipError, match="shape"):
        backend.pack_dedode({**det, k: torch.zeros(256, 128, 1, 1)}, desc)
    with pytest.raises(backend.ImcuiHipError, match="shape"):
        backend.pack_dedode({**det, "encoder.layers.14.weight": torch.zeros(256, 64, 3, 3)}, desc)
    with pytest.raises(backend.ImcuiHipError):  # the two state dicts swapped: 256 logits where the detector has one
        backend.pack_dedode(desc, det)


def test_other_widths_pack_and_a_truncated_refiner_is_refused(lib):
    """The refiner shapes are read from the tensors: other hidden widths, context widths and block counts than the synthetic table load;
    a refiner that lost a layer, a whole scale, or whose context does not match what the coarser scale hands down is refused."""
    table = {"detector": (3, ((512, 256, 64 + 1), (256 + 64, 128, 32 + 1), (128 + 32, 64, 32 + 1), (64 + 32, 32, 1 + 1))),
             "descriptor": (2, ((512, 128, 64 + 256), (256 + 64, 64, 32 + 256), (128 + 32, 64, 64 + 256), (64 + 64, 64, 1 + 256)))}  # fmt: skip
    det, desc = dedode_state_dicts(1, refiners=table)
    packed, dims = backend.pack_dedode(det, desc)
    assert dims[:8] == (512, 256, 65, 3, 320, 128, 33, 3) and dims[-4:] == (128, 64, 257, 2)
    assert packed.numel() == lib.imcui_hip_dedode_packed_floats(backend._dedode_cdims(dims)) != backend.pack_dedode(*sds())[0].numel()
    assert table != DEDODE_REFINERS
    # truncated: the last hidden block of one scale without its 1x1, a block in the middle gone, a scale gone
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_dedode({k: v for k, v in det.items() if k != "decoder.layers.2.hidden_blocks.2.3.bias"}, desc)
    with pytest.raises(backend.ImcuiHipError, match="unexpected"):
        backend.pack_dedode({k: v for k, v in det.items() if not k.startswith("decoder.layers.2.hidden_blocks.1.")}, desc)
    with pytest.raises(backend.ImcuiHipError, match="scale 1 cannot be read"):
        backend.pack_dedode(det, {k: v for k, v in desc.items() if not k.startswith("decoder.layers.1.")})
    with pytest.raises(backend.ImcuiHipError, match="hands down"):  # context 48 where the coarser scale hands down 64
        bad = dict(det)
        bad["decoder.layers.4.block1.0.weight"] = torch.zeros(128, 256 + 48, 1, 1)
        backend.pack_dedode(bad, desc)
    with pytest.raises(backend.ImcuiHipError, match="hidden"):
        d2, _ = dedode_state_dicts(1, refiners={**table, "detector": (3, ((512, 40, 65), (320, 128, 33), (160, 64, 33), (96, 32, 2)))})
        backend.pack_dedode(d2, desc)


def test_packed_buffer_is_byte_identical(lib, golden_dir):
    with open(os.path.join(golden_dir, "dedode_packed_digest.json")) as f:
        golden = json.load(f)
    buf = backend.pack_dedode(*sds())[0].numpy()
    assert buf.size == golden["floats"]
    assert hashlib.sha256(buf.tobytes()).hexdigest() == golden["sha256"]


def test_batchnorm_is_folded_into_the_first_layer():
    """The packed buffer begins with the detector's encoder.layers.0 as [9 taps][3 input channels][64], BatchNorm folded."""
    det, _ = sds()
    packed = backend.pack_dedode(*sds())[0]
    w = packed[: 27 * 64].reshape(3, 3, 3, 64).permute(3, 2, 0, 1)
    scale = det["encoder.layers.1.weight"] / torch.sqrt(det["encoder.layers.1.running_var"] + 1e-5)
    assert torch.allclose(w, det["encoder.layers.0.weight"] * scale.view(64, 1, 1, 1), rtol=1e-6, atol=0)
    bias = det["encoder.layers.0.bias"] * scale + det["encoder.layers.1.bias"] - det["encoder.layers.1.running_mean"] * scale
    assert torch.allclose(packed[27 * 64 : 28 * 64], bias, rtol=1e-5, atol=1e-7)


def test_plugin_contract_and_refusals(golden_dir):
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.utils.base_model import dynamic_load

    with open(os.path.join(golden_dir, "dedode_confs.json")) as f:
        golden = json.load(f)
    cls = dynamic_load(extractors, golden["module"])
    assert cls.__name__ == golden["class_name"]
    assert cls.default_conf == golden["default_conf"] == R.DEFAULT_CONF
    assert cls.required_inputs == golden["required_inputs"] and cls.takes_rgb
    assert cls.hub_folder == golden["hub_folder"]
    assert golden["outputs"] == {"keypoints": [1, "N", 2], "scores": [1, "N"], "descriptors": [1, 256, "N"]}
    det, desc = sds()
    given = {"state_dict_detector": det, "state_dict_descriptor": desc}
    conf = golden["extractor_confs"]["dedode"]
    assert conf["preprocessing"]["dfactor"] == 8 and conf["preprocessing"]["grayscale"] is False
    m = cls({**conf["model"], **given})
    assert not any(k.startswith("state_dict") for k in m.conf) and m.packed.dtype == torch.float32 and not m.packed.is_cuda
    assert m.conf["max_keypoints"] == 5000 and m.conf["dense"] is False and len(m.dims) == 32
    with pytest.raises(backend.ImcuiHipError, match="ROCm device"):  # no CPU fallback
        m({"image": torch.zeros(1, 3, 96, 128)})
    with pytest.raises(ValueError, match="RGB"):
        m({"image": torch.zeros(1, 1, 96, 128)})
    with pytest.raises(ValueError, match="multiples of 8"):
        m({"image": torch.zeros(1, 3, 96, 100)})
    with pytest.raises(ValueError, match="topk"):  # 5000 > 64 * 64
        m({"image": torch.zeros(1, 3, 64, 64)})
    with pytest.raises(ValueError, match="dense"):
        cls({"dense": True, **given})
    with pytest.raises(ValueError, match="not served"):
        cls({"model_detector_name": "dedode_detector_B.pth", **given})
    with pytest.raises(ValueError, match="not served"):
        cls({"model_descriptor_name": "dedode_descriptor_G.pth", **given})
    with pytest.raises(FileNotFoundError):
        cls({"weights_path_detector": "/nonexistent/dedode_detector_L.pth", "state_dict_descriptor": desc})
