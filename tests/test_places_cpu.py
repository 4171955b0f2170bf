"""CosPlace / EigenPlaces without a GPU: the restatement (tests/places_reference.py) against the one outside fact that pins its layout
(torchvision's published parameter counts), the library's tensor-name table against the restatement's state dict for all four backbones,
the strict packer, the plugins' contract with the reference's values written out, the map-size formulas, and the float32 restatement's
own error against its float64 self on the inputs of the end-to-end GPU test (tests/test_gpu_places.py).

SPREAD records that error (largest absolute difference over the largest float64 magnitude; layer4 map, descriptor), measured here with
torch on the CPU.  The end-to-end bar of the project is max(1e-4, 3 x spread): every spread is below 1e-6, so the bar is 1e-4."""
import functools

import pytest
import torch

import places_reference as R
from imcui_hip import backend
from imcui_hip.synth_weights import places_synth_state

# (backbone, fc_output_dim, (H, W)) of the end-to-end test, all at B = 2 -> (layer4 map, descriptor) float32-vs-float64 spread
SPREAD = {
    (18, 512, (32, 48)): (5.11e-07, 2.94e-07),
    (18, 512, (50, 70)): (2.96e-07, 2.73e-07),
    (18, 512, (272, 336)): (4.67e-07, 2.23e-07),
    (50, 2048, (32, 48)): (4.90e-07, 4.17e-07),
    (50, 2048, (50, 70)): (4.27e-07, 3.49e-07),
    (50, 2048, (272, 336)): (6.54e-07, 2.45e-07),
    (101, 2048, (32, 48)): (5.46e-07, 4.38e-07),
    (152, 512, (32, 48)): (5.86e-07, 5.66e-07),
}
BAR = max(1e-4, 3 * max(max(v) for v in SPREAD.values()))

# torchvision.models.resnetNN: total parameters and those of `fc` (published with the weights' metadata)
PARAMS = {18: (11_689_512, 513_000), 50: (25_557_032, 2_049_000), 101: (44_549_160, 2_049_000), 152: (60_192_808, 2_049_000)}


@functools.lru_cache(maxsize=None)
def state(backbone: int, dim: int) -> dict:
    """The seeded weights shared by every CosPlace / EigenPlaces test (seed 0); read-only."""
    return places_synth_state(backbone, dim, 0)


@functools.lru_cache(maxsize=None)
def net(backbone: int, dim: int, dtype=torch.float32):
    return R.build(state(backbone, dim), backbone, dim, dtype)


@functools.lru_cache(maxsize=None)
def image(hw: tuple, B: int = 2) -> torch.Tensor:
    return torch.rand(B, 3, *hw, generator=torch.Generator().manual_seed(1000 * hw[0] + hw[1]))


@functools.lru_cache(maxsize=None)
def reference32(backbone: int, dim: int, hw: tuple) -> dict:
    """The float32 restatement's outputs on image(hw) (computed once, read-only)."""
    return R.forward(net(backbone, dim), image(hw))


def rel(out, ref) -> float:
    return (out.double().cpu() - ref.double()).abs().max().item() / ref.double().abs().max().item()


@pytest.mark.parametrize("backbone", [18, 50, 101, 152])
def test_parameter_counts_are_torchvisions(backbone):
    total, fc = PARAMS[backbone]
    m = R.make_backbone(backbone)
    assert sum(p.numel() for p in m.parameters() if p.requires_grad) == total - fc
    assert {18: 11_176_512, 50: 23_508_032, 101: 42_500_160, 152: 58_143_808}[backbone] == total - fc


@pytest.mark.parametrize("backbone,dim", [(18, 32), (50, 2048), (101, 128), (152, 512)])
def test_tensor_table_is_the_restatements_state_dict(lib, backbone, dim):
    keys = [k for k in R.GeoLocalizationNet(backbone, dim).state_dict() if not k.endswith("num_batches_tracked")]
    names = backend.places_tensor_names(backbone, dim)
    assert names == keys
    shapes = backend.places_tensor_shapes(backbone, dim)
    sd = R.GeoLocalizationNet(backbone, dim).state_dict()
    assert list(shapes) == keys and all(tuple(sd[k].shape) == shapes[k] for k in keys)
    synth = state(backbone, dim) if (backbone, dim) in ((18, 32),) else None
    if synth is not None:  # the synthetic state carries the module's keys in the module's order, num_batches_tracked included
        assert list(synth) == list(sd) and all(synth[k].shape == sd[k].shape for k in sd)
    assert lib.imcui_hip_places_num_tensors(backbone, dim) == len(keys)
    assert lib.imcui_hip_places_tensor_name(backbone, dim, len(keys)) is None
    assert lib.imcui_hip_places_num_tensors(34, dim) == 0 and lib.imcui_hip_places_packed_floats(34, dim) == 0


def test_packer_is_strict_and_folds_the_batchnorm(lib):
    sd = state(18, 32)
    packed = backend.pack_places(sd, "ResNet18", 32)
    assert packed.numel() == lib.imcui_hip_places_packed_floats(18, 32)
    assert torch.equal(packed, backend.pack_places({"state_dict": sd}, 18, 32)) and torch.equal(packed, backend.pack_places({"model_state_dict": sd}, 18, 32))
    # the stem: [tap][cin (RGB)][64] times bn1's scale, then its shift, both folded in float32
    scale = sd["backbone.1.weight"] / torch.sqrt(sd["backbone.1.running_var"] + torch.tensor(1e-5))
    w = packed[: 147 * 64].view(7, 7, 3, 64).permute(3, 2, 0, 1)
    assert torch.equal(w, sd["backbone.0.weight"] * scale.view(64, 1, 1, 1))
    assert torch.equal(packed[147 * 64 : 148 * 64], sd["backbone.1.bias"] - sd["backbone.1.running_mean"] * scale)
    # the head rides at the end: p, W [D][F], bias (every entry on a 64-float slot)
    assert packed[-(64 + 32 * 512 + 64)].item() == sd["aggregation.1.p"].item()
    assert torch.equal(packed[-(32 * 512 + 64) : -64].view(32, 512), sd["aggregation.3.weight"]) and torch.equal(packed[-64:-32], sd["aggregation.3.bias"])
    plain = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    assert torch.equal(packed, backend.pack_places(plain, 18, 32))
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_places({k: v for k, v in sd.items() if k != "backbone.5.0.downsample.0.weight"}, 18, 32)
    with pytest.raises(backend.ImcuiHipError, match="unexpected"):
        backend.pack_places({**sd, "backbone.4.2.conv1.weight": torch.zeros(64, 64, 3, 3)}, 18, 32)
    with pytest.raises(backend.ImcuiHipError, match="shape"):
        backend.pack_places({**sd, "aggregation.3.weight": sd["aggregation.3.weight"].t().contiguous()}, 18, 32)
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_places(sd, 50, 32)  # another backbone's layout
    with pytest.raises(ValueError, match="VGG16"):
        backend.pack_places(sd, "VGG16", 32)
    with pytest.raises(ValueError, match="unknown backbone"):
        backend.pack_places(sd, "ResNet34", 32)


def test_plugin_contract(lib, tmp_path, monkeypatch):
    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.utils.base_model import BaseModel, dynamic_load

    cos, eig = dynamic_load(extractors, "cosplace"), dynamic_load(extractors, "eigenplaces")
    assert cos.__name__ == "CosPlace" and eig.__name__ == "EigenPlaces" and issubclass(cos, BaseModel) and issubclass(eig, BaseModel)
    # imcui/hloc/extractors/cosplace.py:24-25, eigenplaces.py:33-38, imcui/hloc/configs/extractors.py:382-391
    assert cos.default_conf == {"backbone": "ResNet50", "fc_output_dim": 2048} and list(cos.required_inputs) == ["image"]
    assert eig.default_conf == {"variant": "EigenPlaces", "backbone": "ResNet101", "fc_output_dim": 2048} and list(eig.required_inputs) == ["image"]
    assert ef.confs["cosplace"] == {"output": "global-feats-cosplace", "model": {"name": "cosplace"}, "preprocessing": {"resize_max": 1024}}
    assert ef.confs["eigenplaces"] == {"output": "global-feats-eigenplaces", "model": {"name": "eigenplaces"}, "preprocessing": {"resize_max": 1024}}
    assert cos.takes_rgb and cos.returns_global_descriptor and eig.takes_rgb and eig.returns_global_descriptor
    for cls in (cos, eig):
        with pytest.raises(ValueError, match="VGG16"):
            cls({"backbone": "VGG16", "fc_output_dim": 512, "state_dict": state(18, 32)})
    with pytest.raises(ValueError, match="variant"):
        eig({"variant": "NetVLAD", "backbone": "ResNet18", "fc_output_dim": 32, "state_dict": state(18, 32)})
    with pytest.raises(FileNotFoundError):
        cos({"weights_path": "/nonexistent/ResNet50_2048_cosplace.pth"})
    want = backend.pack_places(state(18, 32), 18, 32)
    m = cos({"backbone": "ResNet18", "fc_output_dim": 32, "state_dict": state(18, 32)})
    assert torch.equal(m.packed, want) and "state_dict" not in m.conf
    # a checkpoint file, by `weights_path` and at the hub cache path of each variant, wrapped and with DataParallel's prefix
    path = tmp_path / "hub" / "checkpoints" / "ResNet18_32_eigenplaces.pth"
    path.parent.mkdir(parents=True)
    torch.save({"model_state_dict": {"module." + k: v for k, v in state(18, 32).items()}}, path)
    assert torch.equal(cos({"backbone": "ResNet18", "fc_output_dim": 32, "weights_path": str(path)}).packed, want)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    assert torch.equal(eig({"backbone": "ResNet18", "fc_output_dim": 32}).packed, want)
    torch.save(state(18, 32), path.with_name("ResNet18_32_cosplace.pth"))
    assert torch.equal(eig({"variant": "CosPlace", "backbone": "ResNet18", "fc_output_dim": 32}).packed, want)
    with pytest.raises(ValueError, match="RGB"):
        backend.places_check_args((1, 1, 64, 64))
    backend.places_check_args((1, 3, 1, 1))


@pytest.mark.parametrize("hw,want", [((1, 1), ((1, 1),) * 5), ((5, 7), ((3, 4), (2, 2), (1, 1), (1, 1), (1, 1))),
                                     ((32, 48), ((16, 24), (8, 12), (4, 6), (2, 3), (1, 2))), ((50, 70), ((25, 35), (13, 18), (7, 9), (4, 5), (2, 3)))],
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v[0], int) else None)  # fmt: skip
def test_map_sizes_follow_the_formulas(hw, want):
    assert backend.places_map_size(*hw) == want
    out = R.forward(net(18, 512), torch.rand(1, 3, *hw, generator=torch.Generator().manual_seed(1)))
    assert tuple(out["stem"].shape[2:]) == want[1]
    for L in range(1, 5):
        assert tuple(out["blocks"][(L, 1)].shape[2:]) == want[L]
    assert tuple(out["backbone"].shape) == (1, 512, *want[4]) and out["global_descriptor"].shape == (1, 512)


@pytest.mark.parametrize("cfg", list(SPREAD), ids=lambda c: f"resnet{c[0]}-{c[1]}-{c[2][0]}x{c[2][1]}")
def test_float32_restatement_against_its_float64_self(cfg):
    """The spread the end-to-end bar refers to.  The recorded figure must not understate what is measured (CPU float32 sums differ a
    little with the thread count and the BLAS: a factor of 4 is allowed)."""
    backbone, dim, hw = cfg
    f32 = reference32(backbone, dim, hw)
    f64 = R.forward(R.build(state(backbone, dim), backbone, dim, torch.float64), image(hw))
    e_map, e_desc = rel(f32["backbone"], f64["backbone"]), rel(f32["global_descriptor"], f64["global_descriptor"])
    print(f"[places-cpu] ResNet-{backbone}/{dim} {hw}: float32 against float64: layer4 map {e_map:.2e}, descriptor {e_desc:.2e}; "
          f"map max {f64['backbone'].abs().max().item():.2f}, mean {f64['backbone'].mean().item():.3f}")  # fmt: skip
    assert torch.allclose(f64["global_descriptor"].norm(dim=1), torch.ones(2, dtype=torch.float64), atol=1e-12)
    assert 0.05 < f64["backbone"].abs().max().item() < 1e3, "the synthetic activations left O(1)"
    assert e_map <= 4 * SPREAD[cfg][0] and e_desc <= 4 * SPREAD[cfg][1], (e_map, e_desc, SPREAD[cfg])
    assert BAR == 1e-4
