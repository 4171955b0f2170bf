"""D2-Net / RoRD without a GPU: the restatement's two detector forms against each other, its float32 run against its float64 run at the
GPU test sizes (where the position bar of tests/test_gpu_d2net.py comes from), the strict packer and both containers, the packed
digest, the plugins' contract against values recorded in tests/golden/d2net_confs.json, the level sizes and the refusals."""
import functools
import hashlib
import json
import os

import pytest
import torch

import d2net_reference as R
from imcui_hip import backend
from imcui_hip.synth_weights import d2net_state_dict

SIZES = ((32, 48), (50, 70), (96, 128))


def image(h, w, seed=0):
    """A seeded uniform-random RGB image [1,3,h,w]."""
    return torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(100 + seed))


@functools.lru_cache(maxsize=None)
def sd():
    return d2net_state_dict(0)


@functools.lru_cache(maxsize=None)
def reference(hw, dtype=torch.float32, multiscale=False, use_relu=True):
    return R.extract(sd(), image(*hw), {"multiscale": multiscale, "use_relu": use_relu, "max_keypoints": 0}, dtype)


def ident(r):
    return list(zip(r["level"].tolist(), r["channel"].tolist(), r["i"].tolist(), r["j"].tolist()))


def position_spread(a, b):
    """Largest |position difference| (image pixels) over the key-points two runs share."""
    ia, ib = {k: n for n, k in enumerate(ident(a))}, {k: n for n, k in enumerate(ident(b))}
    common = [k for k in ia if k in ib]
    if not common:
        return 0.0
    ka, kb = a["keypoints"][[ia[k] for k in common]].double(), b["keypoints"][[ib[k] for k in common]].double()
    return (ka - kb).abs().max().item()


@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_explicit_order_and_conv2d_forms_detect_the_same(hw):
    """Every difference between the two forms is listed and must be a round-off event: the edge ratio within 1e-4 of 7.2, or the
    determinant within 1e-5 of zero relative to its two products, in float64."""
    f = reference(hw)["dense_features"][0].permute(2, 0, 1).contiguous()
    de, sie, sje = R.detect(f, R.hessian_explicit)
    dc, sic, sjc = R.detect(f, R.hessian_conv)
    diff = torch.nonzero(de ^ dc)
    dii, djj, dij, _, _ = R.hessian_explicit(f.double())
    for c, i, j in diff.tolist():
        a, b = (dii[c, i, j] * djj[c, i, j]).item(), (dij[c, i, j] ** 2).item()
        det, tr = a - b, (dii[c, i, j] + djj[c, i, j]).item()
        print(f"{hw}: forms differ at {(c, i, j)}: det {det:.6g}, ratio {tr * tr / det if det else float('nan'):.8g}")
        assert abs(det) < 1e-5 * (abs(a) + b) or abs(tr * tr / det - 7.2) < 7.2e-4, (c, i, j)
    both = de & dc
    n = int(both.sum())
    e = max((sie[both] - sic[both]).abs().max().item(), (sje[both] - sjc[both]).abs().max().item()) if n else 0.0
    print(f"{hw}: {n} detections in both forms, {diff.shape[0]} differ, steps differ by at most {e:.1e}")
    assert n >= 3 and e < 1e-3


@pytest.mark.parametrize("hw,ms", [((50, 70), False), ((96, 128), False), ((50, 70), True)], ids=["50x70-ss", "96x128-ss", "50x70-ms"])
def test_float32_and_float64_restatements_agree(hw, ms):
    a, b = reference(hw, torch.float32, ms), reference(hw, torch.float64, ms)
    sa, sb = set(ident(a)), set(ident(b))
    e_map = max((x.double() - y).abs().max().item() / y.abs().max().item() for x, y in zip(a["dense_features"], b["dense_features"]))
    e_pos = position_spread(a, b)
    print(f"{hw} multiscale={ms}: {len(sa)} key-points, float32 / float64 differ in {len(sa ^ sb)}; maps {e_map:.1e}; positions {e_pos:.2e} px")
    assert len(sa) >= 10 and len(sa ^ sb) == 0
    assert e_map < 1e-5
    assert torch.all(a["scores"][1:] >= a["scores"][:-1])
    if ms:
        assert len(set(a["level"].tolist())) >= 2


def test_multiscale_48x64_float32_and_float64_agree():
    a, b = reference((48, 64), torch.float32, True), reference((48, 64), torch.float64, True)
    print(f"48x64 multiscale: {len(ident(a))} key-points, positions {position_spread(a, b):.2e} px")
    assert set(ident(a)) == set(ident(b)) and len(ident(a)) >= 10


def test_pack_is_strict(lib):
    names, shapes = backend.d2net_tensor_names(), backend.d2net_tensor_shapes()
    assert names == list(sd()) and len(names) == 20
    assert {k: tuple(t.shape) for k, t in sd().items()} == shapes
    packed = backend.pack_d2net(sd())
    assert packed.numel() == lib.imcui_hip_d2net_packed_floats() > 0 and packed.dtype == torch.float32
    assert torch.equal(backend.pack_d2net(d2net_state_dict(0, checkpoint=True)), packed)  # upstream's {'model': ...} container
    k = "dense_feature_extraction.model.19.weight"
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_d2net({n: t for n, t in sd().items() if n != k})
    with pytest.raises(backend.ImcuiHipError, match="unexpected"):
        backend.pack_d2net({**sd(), "detection.dii_filter": torch.ones(1, 1, 3, 3)})
    with pytest.raises(backend.ImcuiHipError, match="shape"):
        backend.pack_d2net({**sd(), k: torch.zeros(512, 256, 3, 3)})


def test_packed_buffer_is_byte_identical(lib, golden_dir):
    with open(os.path.join(golden_dir, "d2net_packed_digest.json")) as f:
        golden = json.load(f)
    buf = backend.pack_d2net(sd()).numpy()
    assert buf.size == golden["floats"]
    assert hashlib.sha256(buf.tobytes()).hexdigest() == golden["sha256"]


def test_first_layer_is_packed_tap_major():
    """The packed buffer begins with model.0 as [9 taps][3 input channels][64]."""
    packed = backend.pack_d2net(sd())
    w = packed[: 27 * 64].reshape(3, 3, 3, 64).permute(3, 2, 0, 1)
    assert torch.equal(w, sd()["dense_feature_extraction.model.0.weight"])


def test_level_sizes_and_refusals():
    assert backend.d2net_levels(480, 640) == [(480, 640)]
    assert backend.d2net_levels(50, 70, backend.D2NET_SCALES_MS) == [(25, 35), (50, 70), (100, 140)] == R.level_sizes(50, 70, [0.5, 1, 2])
    assert backend.d2net_levels(1201, 1599, backend.D2NET_SCALES_MS) == [(600, 799), (1201, 1599), (2402, 3198)]
    assert backend.d2net_levels(8, 8) == [(8, 8)]
    with pytest.raises(ValueError, match="empty"):
        backend.d2net_levels(7, 64)
    with pytest.raises(ValueError, match="empty"):
        backend.d2net_levels(15, 64, backend.D2NET_SCALES_MS)  # 7 x 32 at scale 0.5
    with pytest.raises(ValueError, match="RGB"):
        backend.d2net_check_args((1, 1, 64, 64))
    f = R.trunk(sd(), torch.zeros(1, 3, 50, 70))
    assert f.shape == (1, 512, 11, 16)  # odd halves: 25x35 -> 12x17 -> 11x16


def test_cut_keeps_the_later_of_tied_scores():
    s = torch.tensor([0.5, 0.9, 0.5, 0.5, 0.1])
    assert R.cut(s, 3).tolist() == [2, 3, 1] and R.cut(s, 0).tolist() == [4, 0, 2, 3, 1]


def test_plugin_contract_and_refusals(golden_dir):
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.utils.base_model import dynamic_load

    with open(os.path.join(golden_dir, "d2net_confs.json")) as f:
        golden = json.load(f)
    for module, cls_name in golden["class_names"].items():
        cls = dynamic_load(extractors, module)
        assert cls.__name__ == cls_name
        assert cls.default_conf == golden["default_conf"][module]
        assert cls.required_inputs == golden["required_inputs"] and cls.takes_rgb
        assert cls.hub_folder == golden["hub_folders"][module]
        for name, conf in golden["extractor_confs"].items():
            if conf["model"]["name"] != module:
                continue
            m = cls({**conf["model"], "state_dict": d2net_state_dict(0, checkpoint=True)})
            assert "state_dict" not in m.conf and m.packed.dtype == torch.float32 and not m.packed.is_cuda
            assert m.conf["max_keypoints"] == 5000 and m.conf["multiscale"] == (name == "d2net-ms") and m.conf["use_relu"] is True
    with pytest.raises(backend.ImcuiHipError, match="ROCm device"):  # no CPU fallback
        m({"image": torch.zeros(1, 3, 64, 64)})
    with pytest.raises(ValueError, match="RGB"):
        m({"image": torch.zeros(1, 1, 64, 64)})
    with pytest.raises(ValueError, match="empty"):
        m({"image": torch.zeros(1, 3, 6, 64)})
    with pytest.raises(FileNotFoundError):
        cls({"weights_path": "/nonexistent/rord.pth"})
