"""DoG + HardNet / SOSNet without a GPU: the restated networks take the seeded state dicts strictly (the key-name test), the packer's
layout, strictness and digest (tests/golden/dog_packed_digest.json, written by make_dog_golden.py), SOSNet's LocalResponseNorm being an L2
normalisation over 128 channels, the refusals raised before any launch, and the plugin's contract against values recorded from the
reference (tests/golden/dog_conf.json: dog.py:23-33 and configs/extractors.py:144-175)."""
import functools
import hashlib
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

import dog_reference as R
from imcui_hip import backend
from imcui_hip.synth_weights import hardnet_synth_state, sosnet_synth_state

NETS = ("hardnet", "sosnet")


@functools.lru_cache(maxsize=None)
def state(name: str) -> dict:
    """The seeded weights shared by every DoG test; read-only."""
    return {"hardnet": hardnet_synth_state, "sosnet": sosnet_synth_state}[name](0)


def pack(name: str, sd=None) -> torch.Tensor:
    return (backend.pack_hardnet if name == "hardnet" else backend.pack_sosnet)(state(name) if sd is None else sd)


def rel(out, ref) -> float:
    return (out.double().cpu() - ref.double()).abs().max().item() / ref.double().abs().max().item()


@pytest.mark.parametrize("name", NETS)
def test_state_dict_loads_strictly(name):
    net = R.build(name, state(name))
    assert len(R.layer_modules(net)) == 7
    var = torch.cat([v for k, v in state(name).items() if k.endswith("running_var")])
    assert var.min().item() > 0 and not torch.all(var == 1)
    root = "features" if name == "hardnet" else "layers"
    assert all(k.startswith(root + ".") for k in state(name))
    out = net(torch.rand(3, 1, 32, 32, generator=torch.Generator().manual_seed(1)))
    assert out.shape == (3, 128) and torch.allclose(out.norm(dim=1), torch.ones(3), atol=1e-5)


def test_lrn_over_128_channels_is_l2_normalisation():
    """LocalResponseNorm(256, alpha=256, beta=0.5, k=0): the window of every channel (128 back, 127 forward) covers all 128 channels, the
    average over 256 slots times alpha is the plain sum of squares, so y = x / sqrt(sum x^2)."""
    x = torch.randn(5, 128, 1, 1, generator=torch.Generator().manual_seed(2), dtype=torch.float64) + 1e-10
    lrn = torch.nn.LocalResponseNorm(256, alpha=256.0, beta=0.5, k=0.0)(x)
    l2 = x / x.pow(2).sum(dim=1, keepdim=True).sqrt()
    assert (lrn - l2).abs().max().item() < 1e-14
    x32 = x.float()
    assert (torch.nn.LocalResponseNorm(256, alpha=256.0, beta=0.5, k=0.0)(x32) - x32 / x32.pow(2).sum(dim=1, keepdim=True).sqrt()).abs().max().item() < 3e-7


@pytest.mark.parametrize("name", NETS)
def test_packed_buffer_is_byte_identical(lib, golden_dir, name):
    with open(os.path.join(golden_dir, "dog_packed_digest.json")) as f:
        gold = json.load(f)[name]
    buf = pack(name).numpy()
    assert buf.size == gold["floats"] == lib.imcui_hip_patchdesc_packed_floats()
    assert hashlib.sha256(buf.tobytes()).hexdigest() == gold["sha256"]


@pytest.mark.parametrize("name", NETS)
def test_packer_round_trip(lib, name):
    """Layer 1 is [9 taps][32] with the BatchNorm scale folded and the shift behind it; layer 7 follows the five GEMM layers as float32
    [128][8 x 8 taps][128 channels] times a power of two, its shift and the inverse of that power."""
    sd, buf = state(name), pack(name)
    (c0, b0), (c6, b6) = R.layer_modules(R.build(name, sd))[0], R.layer_modules(R.build(name, sd))[6]

    def fold(conv, bn):
        s = 1.0 / torch.sqrt(bn.running_var + 1e-5)
        return conv.weight.detach() * s.view(-1, 1, 1, 1), -bn.running_mean * s

    w, sh = fold(c0, b0)
    assert torch.equal(buf[: 9 * 32].view(9, 32), w.view(32, 9).t()) and torch.equal(buf[320 : 320 + 32], sh)
    pad = lambda n: (n + 63) // 64 * 64  # noqa: E731
    off = 320 + 64
    for cin, cout, _ in backend.PATCHDESC_LAYERS[1:6]:
        K, rows = 9 * cin, (cout + 31) // 32 * 32
        off += pad(cout * K) + pad(cout) + 2 * pad(rows * K // 2) + 64
    w, sh = fold(c6, b6)
    inv = buf[off + 128 * 8192 + 128].item()  # layer 7 is packed times a power of two (exact), 2^-e follows the shift
    assert math.frexp(inv)[0] == 0.5 and 4096 <= buf[off : off + 128 * 8192].abs().max().item() <= 8192
    assert torch.equal(buf[off : off + 128 * 8192].view(128, 8, 8, 128) * inv, w.permute(0, 2, 3, 1))
    assert torch.equal(buf[off + 128 * 8192 : off + 128 * 8192 + 128], sh)
    assert buf.numel() == off + 128 * 8192 + 128 + 64


def test_packer_is_strict_and_unwraps_checkpoints(lib):
    names = backend.patchdesc_tensor_names("hardnet")
    assert names[0] == "features.0.weight" and names[-1] == "features.20.running_var" and len(names) == 21
    assert backend.patchdesc_tensor_names("sosnet")[0] == "layers.1.weight" and backend.patchdesc_tensor_names("sosnet")[-1] == "layers.21.running_var"
    sd = dict(state("hardnet"))
    assert torch.equal(backend.pack_hardnet({"state_dict": sd}), pack("hardnet"))
    assert torch.equal(backend.pack_sosnet({"state_dict": state("sosnet")}), pack("sosnet"))
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_hardnet({k: v for k, v in sd.items() if k != "features.19.weight"})
    with pytest.raises(backend.ImcuiHipError, match="unexpected"):
        backend.pack_hardnet({**sd, "features.0.bias": torch.zeros(32)})
    with pytest.raises(backend.ImcuiHipError, match="shape"):
        backend.pack_hardnet({**sd, "features.19.weight": sd["features.19.weight"][:, :, :3, :3].contiguous()})
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_sosnet(sd)  # HardNet's key names are not SOSNet's


def test_pyramid_levels_follow_the_loop(lib):
    """The library builds the levels a key-point can choose: min(kornia's loop, its clamp + 1)."""
    for H, W in ((40, 56), (70, 101), (96, 130), (160, 200), (480, 640)):
        loop = len(R.pyramid(torch.zeros(1, 1, H, W)))
        assert lib.imcui_hip_patchdesc_num_levels(H, W) == min(loop, max(0, min(H, W) // 32 - 1) + 1), (H, W)
    assert lib.imcui_hip_patchdesc_num_levels(160, 200) == 4  # the clamp allows level 4, the loop stops at 3: such patches are zero


def test_refusals_before_any_launch(lib):
    from imcui_hip.hloc.extractors.dog import DoG

    sd = state("hardnet")
    for name in ("sift", "rootsift"):
        with pytest.raises(backend.ImcuiHipError, match="`sift` plugin"):
            DoG({"descriptor": name})
    with pytest.raises(backend.ImcuiHipError, match="`sift` plugin"):
        DoG({})  # the class default is rootsift
    with pytest.raises(ValueError, match="Unknown descriptor"):
        DoG({"descriptor": "tfeat", "state_dict": sd})
    with pytest.raises(backend.ImcuiHipError, match="first_octave"):
        DoG({"descriptor": "hardnet", "state_dict": sd, "options": {"first_octave": -1}})
    with pytest.raises(backend.ImcuiHipError, match="num_octaves"):
        DoG({"descriptor": "hardnet", "state_dict": sd, "options": {"num_octaves": 4}})
    with pytest.raises(backend.ImcuiHipError, match="patch_size"):
        DoG({"descriptor": "hardnet", "state_dict": sd, "patch_size": 64})
    with pytest.raises(FileNotFoundError):
        DoG({"descriptor": "sosnet", "checkpoint": "/nonexistent/sosnet.pth"})
    with pytest.raises(ValueError, match="gray"):
        backend.patchdesc_check_args((1, 3, 64, 64), 16, 1024, 12.0)
    with pytest.raises(ValueError, match="8 x 8"):
        backend.patchdesc_check_args((1, 1, 7, 64), 16, 1024, 12.0)
    with pytest.raises(ValueError, match="chunk"):
        backend.patchdesc_check_args((1, 1, 64, 64), 16, 0, 12.0)
    with pytest.raises(ValueError, match="mr_size"):
        backend.patchdesc_check_args((1, 1, 64, 64), 16, 1024, float("nan"))
    m = DoG({"descriptor": "hardnet", "state_dict": sd, "max_keypoints": 100})
    with pytest.raises(AssertionError):
        m({"image": torch.zeros(1, 3, 32, 32)})  # the reference's `assert image.shape[1] == 1`
    with pytest.raises(AssertionError):
        m({"image": torch.full((1, 1, 32, 32), 1.5)})  # ... and its range assertion


def test_plugin_contract(lib, golden_dir):
    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.utils.base_model import BaseModel, dynamic_load

    with open(os.path.join(golden_dir, "dog_conf.json")) as f:
        ref = json.load(f)
    cls = dynamic_load(extractors, "dog")  # asserts that the module defines exactly one BaseModel subclass
    assert cls.__name__ == "DoG" and issubclass(cls, BaseModel)
    assert cls.default_conf == ref["default_conf"] and list(cls.required_inputs) == ref["required_inputs"]
    assert cls.max_batch_size == 1024 and cls.detection_noise == 1.0
    for name in NETS:
        assert ef.confs[name] == ref["extractor_confs"][name]
        m = cls({**ef.confs[name]["model"], "state_dict": state(name)})
        assert torch.equal(m.packed, pack(name)) and "state_dict" not in m.conf
        assert m.sift_conf["detection_threshold"] == pytest.approx(0.03) and m.sift_conf["num_octaves"] == 3 and m.sift_conf["nms_radius"] is None
        assert m.sift_conf["max_keypoints"] == 5000


def test_restatement_float32_against_float64():
    """The float32 restatement against its own float64 run, end to end on a seeded texture: the CPU's own error is far inside the 1e-4
    descriptor bar of the GPU tests."""
    g = torch.Generator().manual_seed(5)
    img = F.avg_pool2d(torch.rand(1, 1, 96 * 2, 130 * 2, generator=g), 2)
    kp = torch.rand(24, 2, generator=g) * torch.tensor([129.0, 95.0])
    scales = torch.tensor([1.7, 3.1, 6.3] * 8)
    oris = torch.rand(24, generator=g) * 360 - 180
    for name in NETS:
        d32 = R.forward(name, state(name), img, kp, scales, oris, dtype=torch.float32)
        d64 = R.forward(name, state(name), img, kp, scales, oris, dtype=torch.float64)
        err = (d32.double() - d64).abs().max().item()
        print(f"[dog-cpu] {name}: float32 restatement against float64 {err:.2e}")
        assert err < 2e-5 and torch.allclose(d64.norm(dim=1), torch.ones(24, dtype=torch.float64), atol=1e-9)
