"""LISRD without a GPU: the restatement (tests/lisrd_reference.py) in float32 against itself in float64; the layer table of the library
against the restatement's modules; the strict packer, its round trips and refusals; the seeded weights' operating point; the golden
file's own invariants (recomputed from what it stores with the wrapper's formulas, restated here); the plugin's host-side pieces.

Measured here (float32 against float64, CPU, seed 0, uint8 images of 24x32 / 50x70 / 96x128): dense maps within 3.3e-6 of each map's
largest magnitude (asserted: 1e-5), the (1024, 3, 3) meta descriptors within 7e-7 absolute (asserted: 2e-6)."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lisrd_reference as R
from imcui_hip import backend
from imcui_hip.synth_weights import lisrd_synth_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lisrd_golden.npz")
SIZES = ((24, 32), (50, 70), (96, 128))


@functools.lru_cache(maxsize=None)
def state():
    return lisrd_synth_state(0)


@functools.lru_cache(maxsize=None)
def net(double=False):
    m = R.LisrdNet().eval()
    m.load_state_dict(state())
    return m.double() if double else m


def image(h, w, seed=0):
    return torch.randint(0, 256, (1, 3, h, w), generator=torch.Generator().manual_seed(seed + h), dtype=torch.uint8).float()


@pytest.mark.parametrize("h,w", SIZES)
def test_float32_against_float64(h, w):
    img = image(h, w)
    with torch.no_grad():
        o32, o64 = net()(img), net(True)(img.double())
    for v in R.VARIANCES:
        for key in ("descriptors", "meta_maps"):
            assert o32[key][v].shape == (1, 128, h // 8, w // 8)
            err = float((o32[key][v] - o64[key][v]).abs().max() / o64[key][v].abs().max())
            assert err < 1e-5, (key, v, err)
        m = o32["meta_descriptors"][v]
        assert m.shape == (1, 1024, 3, 3)
        assert float((m - o64["meta_descriptors"][v]).abs().max()) < 2e-6
        assert float((m.norm(dim=1) - 1).abs().max()) < 1e-5  # every region's vector is a unit vector


def test_relu_before_batchnorm_and_dropped_remainder():
    """the two facts of the definition a fold would get wrong: the BatchNorm sees ReLU's output; remainder cells do not reach NetVLAD"""
    n = net()
    x = torch.randn(1, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    bb = n._backbone
    with torch.no_grad():
        want = bb._bn1_1(F.relu(bb._conv1_1(x)))
        folded = F.relu(bb._bn1_1(bb._conv1_1(x)))
    assert float((want - folded).abs().max()) > 1e-2
    assert float(want.min()) < 0  # (an affine of a ReLU output goes negative: no ReLU follows it)
    meta = torch.randn(1, 128, 7, 11, generator=torch.Generator().manual_seed(2))  # regions of 2 x 3 cells; row 6 and columns 9, 10 dropped
    meta2 = meta.clone()
    meta2[:, :, 6:], meta2[:, :, :, 9:] = float("nan"), float("nan")
    with torch.no_grad():
        assert torch.equal(n.regional_vlad(meta, R.VARIANCES[0]), n.regional_vlad(meta2, R.VARIANCES[0]))


def test_layer_table():
    layers = backend.lisrd_layers()
    assert [L["name"] for L in layers[:8]] == [f"conv{t}" for t, *_ in R.BACKBONE]
    for L, (tag, cin, cout, pool) in zip(layers, R.BACKBONE):
        assert (L["cin"], L["cout"], bool(L["pool"])) == (cin, cout, pool)
        assert L["kind"] == ("stem" if tag == "1_1" else "conv3x3")
    assert layers[8] == {"name": "heads_1", "kind": "heads", "cin": 256, "cout": 2048, "pool": 0, "in_off": 0}
    assert [L["in_off"] for L in layers[9:]] == [256 * j for j in range(8)] and all(L["kind"] == "conv1x1" and (L["cin"], L["cout"]) == (256, 128) for L in layers[9:])
    assert len(layers) == 17
    assert list(backend.lisrd_variances()) == R.VARIANCES  # the library's order is the restatement's
    # the tensors the packer takes are exactly the restatement's parameters and buffers (without the counters), shape for shape
    want = {k: tuple(t.shape) for k, t in net().state_dict().items() if not k.endswith("num_batches_tracked")}
    assert backend.lisrd_tensor_shapes() == want
    assert sorted(backend.lisrd_tensor_names()) == sorted(want)


def test_pack_round_trips_and_refusals():
    sd = state()
    packed = backend.pack_lisrd(sd)
    assert packed.dtype == torch.float32 and packed.numel() == backend.load_library().imcui_hip_lisrd_packed_floats() and float(packed[0]) == 19538.0
    assert bool(torch.isfinite(packed).all())
    assert torch.equal(packed, backend.pack_lisrd({k: v.double() for k, v in sd.items()}))  # dtype does not matter
    assert torch.equal(packed, backend.pack_lisrd(dict(reversed(list(sd.items())))))  # nor does the order of the keys
    # the affine behind block 0 is BatchNorm folded in double and rounded once: find it in the buffer
    g, b, m, v = (sd[f"_backbone._bn1_1.{k}"].double() for k in ("weight", "bias", "running_mean", "running_var"))
    a = (g / torch.sqrt(v + 1e-5)).float()
    sh = (b - m * (g / torch.sqrt(v + 1e-5))).float()
    flat = packed.unfold(0, 64, 64)
    assert bool((flat == a).all(1).any()) and bool((flat == sh).all(1).any())
    changed = dict(sd)
    changed["vlad_rot_var_illum_var.centroids"] = sd["vlad_rot_var_illum_var.centroids"] + 1.0
    assert not torch.equal(packed, backend.pack_lisrd(changed))
    for bad, word in (({k: v for k, v in sd.items() if k != "conv_meta_rot_invar_illum_var_2.bias"}, "missing"), ({**sd, "extra.weight": torch.zeros(1)}, "unexpected")):
        with pytest.raises(backend.ImcuiHipError, match=word):
            backend.pack_lisrd(bad)
    with pytest.raises(backend.ImcuiHipError, match="shape"):  # another n_clusters
        backend.pack_lisrd({**sd, "vlad_rot_var_illum_var.centroids": torch.zeros(16, 128)})


def test_seeded_weights_operating_point():
    """activations stay alive through the ten blocks and NetVLAD's soft assignment is neither uniform nor one-hot"""
    n = net()
    img = image(96, 128, 3)
    with torch.no_grad():
        out = n(img)
        feat = n._backbone(img / 255.0)
    assert 0.5 < float(feat.std()) < 2.0 and float((feat.abs() < 1e-6).float().mean()) < 0.01
    for v in R.VARIANCES:
        assert 0.3 < float(out["descriptors"][v].std()) < 3.0
        a = F.softmax(getattr(n, f"vlad_{v}").conv(F.normalize(out["meta_maps"][v], dim=1)), dim=1)
        top = float(a.max(1).values.median())
        assert 0.3 < top < 0.9, (v, top)


def test_golden_file_invariants():
    """the file is what its maker says: margins, shapes, unit vectors; matches and mconf follow from the stored vectors"""
    assert os.path.getsize(GOLDEN) < 1 << 20
    g = np.load(GOLDEN)
    rows = int(g["meta_rows"])
    for p in range(2):
        assert float(g[f"margin_{p}"]) >= 1e-4
        k0, k1 = g[f"keypoints0_{p}"], g[f"keypoints1_{p}"]
        (h0, w0), (h1, w1) = g[f"image0_u8_{p}"].shape[2:], g[f"image1_u8_{p}"].shape[2:]
        assert {(h0, w0), (h1, w1)} == {(40, 56), (50, 70)} and g[f"image0_u8_{p}"].dtype == np.uint8
        assert k0.shape == (60, 2) and k1.shape == (55, 2)
        for k, (h, w) in ((k0, (h0, w0)), (k1, (h1, w1))):
            assert (k[0] == 0).all() and (k[1] == (w - 1, h - 1)).all()
            assert (k == np.round(k)).all(1).sum() >= 15 and (k != np.round(k)).any(1).sum() >= 15  # integer and sub-pixel positions
        d0, d1 = torch.from_numpy(g[f"desc0_{p}"]), torch.from_numpy(g[f"desc1_{p}"])
        assert d0.shape == (60, 4, 128) and d1.shape == (55, 4, 128) and g[f"meta0_{p}"].shape == (rows, 4, 1024) and d0.dtype == torch.float32
        for t in (d0, d1, torch.from_numpy(g[f"meta0_{p}"]), torch.from_numpy(g[f"meta1_{p}"])):
            assert float((t.norm(dim=-1) - 1).abs().max()) < 1e-5
        m0, m1 = g[f"mkeypoints0_{p}"], g[f"mkeypoints1_{p}"]
        assert m0.shape == m1.shape and m0.shape[0] == g[f"mconf_{p}"].shape[0] > 5
        i0 = [int((k0 == q).all(1).argmax()) for q in m0]
        assert i0 == sorted(i0) and len(set(i0)) == len(i0)  # ascending image-0 index, as the reference's mask yields them
        assert all((k0[i] == q).all() for i, q in zip(i0, m0))
    # the restatement reproduces the stored vectors from the stored images (the wrapper called the same modules)
    with torch.no_grad():
        img = torch.from_numpy(g["image0_u8_0"]).float()
        out = net()(img)
        d, m = R.extract_descriptors(torch.from_numpy(g["keypoints0_0"]), out, tuple(img.shape[2:]))
    assert float((d - torch.from_numpy(g["desc0_0"])).abs().max()) < 1e-6 and float((m[:rows] - torch.from_numpy(g["meta0_0"])).abs().max()) < 1e-6


def test_plugin_host_pieces():
    """what the plugin does on the host, without a device: the gray weights, the reference's defaults, the unknown-detector refusal, the
    checkpoint container"""
    from imcui_hip.hloc.matchers import lisrd as P
    from imcui_hip.hloc.utils.weights import unwrap_checkpoint

    assert P.Lisrd.default_conf == {"name": "two_view_pipeline", "model_name": "lisrd_aachen", "max_keypoints": 2048, "detector": "superpoint"}
    assert P.Lisrd.required_inputs == ["image0", "image1"]
    assert sorted(P._DETECTOR_BUILDERS) == ["aliked", "sift", "superpoint"]
    x = torch.rand(2, 3, 5, 7, generator=torch.Generator().manual_seed(0))
    gray = P.rgb_to_grayscale(x)
    assert gray.shape == (2, 1, 5, 7) and torch.allclose(gray[:, 0], 0.299 * x[:, 0] + 0.587 * x[:, 1] + 0.114 * x[:, 2])
    with pytest.raises(ValueError, match="Unknown LISRD detector: orb"):
        P.Lisrd({"detector": "orb", "state_dict": state()})
    sd = state()
    assert unwrap_checkpoint({"model_state_dict": sd, "epoch": 3}) is sd
    with pytest.raises(ValueError, match="at least 24"):
        backend.lisrd_check_args((1, 3, 23, 64))
    with pytest.raises(ValueError, match="3-channel"):
        backend.lisrd_check_args((1, 1, 64, 64))
