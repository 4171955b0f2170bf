"""LANet without a GPU: the restatement (tests/lanet_reference.py) against the golden file written by the reference's own wrapper, the
linearity the sparse descriptor head rests on, the seeded weights' operating point, the strict packer with its BatchNorm folds and the
refusals of the host layer."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lanet_reference as R
from imcui_hip import backend
from imcui_hip.synth_weights import lanet_synth_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lanet_golden.npz")
SIZES = ((32, 48), (50, 70), (96, 128))  # the images of the GPU tests; 50x70 is odd at every pool


def image(h, w, seed=0, batch=1):
    return torch.rand(batch, 3, h, w, generator=torch.Generator().manual_seed(3000 + 10 * h + seed))


@functools.lru_cache(maxsize=None)
def state(seed=0, k=3, bias=True, bn=False, widths=R.WIDTHS):
    return lanet_synth_state(seed, k=k, bias=bias, bn=bn, widths=widths)


@functools.lru_cache(maxsize=None)
def net(seed=0, k=3, bias=True, bn=False, double=False, leaky=False, widths=R.WIDTHS):
    m = R.build(state(seed, k, bias, bn, widths), leaky=leaky)
    return m.double() if double else m


def lib_state(sd):
    """The state dict under the library's names (what the plugin's key table produces)."""
    from imcui_hip.hloc.extractors.lanet import map_lanet_keys

    return map_lanet_keys(sd)


@functools.lru_cache(maxsize=None)
def parts(h, w, seed=0, double=False):
    img = image(h, w, seed)
    with torch.no_grad():
        return net(double=double).parts(img.double() if double else img)


def cells_of(o):
    """Per-cell values of image 0 in row-major cell order: score [np], coord [np,2], desc [np,256], aware [np,3]."""
    return (o["score"][0, 0].flatten(), o["coord"][0].flatten(1).t(), o["desc"][0].flatten(1).t(), o["aware"][0].flatten(1).t())


# ------------------------------------------------------------------ the golden file of the reference's wrapper
@pytest.mark.parametrize("tag", ["40x56", "50x70"])
def test_restatement_and_rule_reproduce_the_wrapper_golden(tag):
    """tests/golden/lanet_golden.npz was written by imcui/hloc/extractors/lanet.py itself around the restated network
    (make_lanet_golden.py).  The restatement + `wrapper_rule` reproduce count and order exactly, and key-points, scores and
    descriptors to float32 round-off (the convolutions may be summed in another order on another host)."""
    g = np.load(GOLDEN)
    img = torch.from_numpy(g[f"image_u8_{tag}"]).float() / 255.0
    with torch.no_grad():
        score, coord, desc, _ = cells_of(net(int(g["seed"])).parts(img))
    full = torch.from_numpy(g[f"descriptors_all_{tag}"])
    for name, thr, k in (("all", 0.1, 0), ("median", float(g[f"median_{tag}"]), 0), ("top7", 0.1, 7)):
        _, kp, sc, de = R.wrapper_rule(score, coord, desc, thr, k)
        want_kp, want_sc = torch.from_numpy(g[f"keypoints_{name}_{tag}"]), torch.from_numpy(g[f"scores_{name}_{tag}"])
        want_de = full if name == "all" else full[torch.from_numpy(g[f"desc_rows_{name}_{tag}"])]
        assert kp.shape == want_kp.shape and sc.shape == want_sc.shape, (name, kp.shape, want_kp.shape)
        assert len(sc) > 0 and bool((sc[1:] >= sc[:-1]).all()), "ascending score"
        errs = ((kp - want_kp).abs().max().item(), (sc - want_sc).abs().max().item(), (de - want_de).abs().max().item())
        print(f"{tag} {name}: {len(sc)} key-points; max |difference| positions {errs[0]:.2e} px, scores {errs[1]:.2e}, descriptors {errs[2]:.2e}")
        assert errs[0] <= 1e-4 and errs[1] <= 1e-5 and errs[2] <= 1e-5
        if k:
            assert len(sc) == k


def test_rule_stable_order_and_refusal():
    score = torch.tensor([0.5, 0.2, 0.5, 0.05, 0.5, 0.9])
    coord = torch.arange(12.0).view(6, 2)
    cells, kp, sc, _ = R.wrapper_rule(score, coord, None, 0.1, 0)
    assert cells.tolist() == [1, 0, 2, 4, 5]  # ascending score, equal scores in cell order
    assert R.wrapper_rule(score, coord, None, 0.1, 3)[0].tolist() == [2, 4, 5]  # the cut keeps the highest cell indices among equals
    assert R.wrapper_rule(score, coord, None, 0.5, 0)[0].tolist() == [5]  # strict threshold
    assert R.wrapper_rule(score, coord, None, 0.95, 0)[0].numel() == 0
    with pytest.raises(ValueError, match="negative"):
        R.wrapper_rule(score, coord, None, 0.1, -2)


# ------------------------------------------------------------------ the linearity the sparse head rests on
def probe_points(W, H, n=40, seed=0):
    """Positions in pixels of a W x H image: the corners, exact pixel centres of the level maps, points whose bilinear corners fall
    outside the maps, then uniform ones."""
    g = torch.Generator().manual_seed(seed)
    fixed = torch.tensor([[0.0, 0.0], [W - 1.0, H - 1.0], [0.0, H - 1.0], [W - 1.0, 0.0], [0.5, 0.5], [2.5, 6.5], [1.5, 1.5], [W - 1.5, H - 2.5]])
    rnd = torch.rand(max(n - len(fixed), 0), 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])
    return torch.cat([fixed, rnd])[:n]


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("with_bias", [False, True])
def test_sample_then_convolve_equals_convolve_then_sample_in_float64(k, with_bias):
    g = torch.Generator().manual_seed(5)
    H, W, h, w, C = 33, 47, 16, 23, 8
    x = torch.randn(1, C, h, w, generator=g, dtype=torch.float64)
    weight = torch.randn(256, C, k, k, generator=g, dtype=torch.float64)
    bias = torch.randn(256, generator=g, dtype=torch.float64) if with_bias else None
    pts = probe_points(W, H).double()
    grid = R.normalised_grid(pts, H, W).view(1, 1, -1, 2)
    fx = ((grid[0, 0, :, 0] + 1) * w - 1) / 2
    assert fx.min() < 0 and fx.max() > w - 1, "some corners lie outside the map"
    dense = R.sample(F.conv2d(x, weight, bias, padding=k // 2), grid)[0, :, 0].t()
    sparse = R.sparse_level(x, weight, bias, grid)
    err = (dense - sparse).abs().max().item() / dense.abs().max().item()
    print(f"k={k} bias={with_bias}: sample-then-convolve against convolve-then-sample in float64: {err:.2e}")
    assert err < 1e-12


# ------------------------------------------------------------------ the seeded weights
def test_seeded_weights_operating_point():
    """lanet_synth_state's promises on the GPU tests' images: the sigmoid spreads over (0, 1), the tanh stays out of saturation on most
    cells, the three level weights stay well away from one-hot."""
    for h, w in SIZES:
        o = parts(h, w)
        s = o["score"][0, 0, 1:-1, 1:-1].flatten()
        t, a = o["tanh"].flatten(), o["aware"]
        q = torch.quantile(s, torch.tensor([0.1, 0.9]))
        print(f"{h}x{w}: interior score 10 % / 90 % quantiles {q[0]:.3f} / {q[1]:.3f}, |tanh| > 0.99 on {(t.abs() > 0.99).float().mean():.3f}, largest level weight {a.max():.3f}")
        assert q[0] < 0.5 < q[1] and q[1] - q[0] > 0.3
        assert (t.abs() > 0.99).float().mean() < 0.1
        assert a.max() < 0.95 and a.min() > 0.005
        assert bool((o["score"][0, 0, 0] == 0).all()) and bool((o["score"][0, 0, :, -1] == 0).all())


@pytest.mark.parametrize("hw", SIZES)
def test_float32_restatement_selects_like_its_float64_self(hw):
    """The end-to-end GPU test allows key-points to differ only where the score lies within the score bar of the threshold or of the
    k-th score, at most 2 % of the cells.  Seed 0 is relied on there: the float32 restatement against its float64 self stays inside
    that cap at every setting the GPU test uses."""
    s32, s64 = cells_of(parts(*hw))[0], cells_of(parts(*hw, double=True))[0]
    coord = torch.zeros(len(s32), 2)
    med = R.median_threshold(s64)
    for thr, k in ((0.1, 0), (med, 0), (0.1, 7)):
        a = set(R.wrapper_rule(s32, coord, None, thr, k)[0].tolist())
        b = set(R.wrapper_rule(s64, coord.double(), None, thr, k)[0].tolist())
        print(f"{hw}: threshold {thr:.4f} k {k}: {len(a)} / {len(b)} key-points, {len(a ^ b)} differ; score spread {(s32.double() - s64).abs().max():.2e}")
        assert len(a ^ b) <= 0.02 * len(s32)


# ------------------------------------------------------------------ the packer
def test_pack_is_strict(lib):
    sd = lib_state(state())
    packed, cfg = backend.pack_lanet(sd)
    assert cfg == {"widths": (32, 64, 128, 256), "k": (3, 3), "bias": (1, 1), "bn": (0, 0), "activation": "relu", "conv_bias": 0}
    ca = backend.lanet_cfg_array(cfg)
    assert packed.numel() == lib.imcui_hip_lanet_packed_floats(ca) > 0 and packed.dtype == torch.float32
    assert packed[0].item() == 19521.0 and packed[1:13].tolist() == [32, 64, 128, 256, 3, 3, 1, 1, 0, 0, 1, 0] and packed[13:15].tolist() == [0.5, 0.22499999403953552]
    names = backend.lanet_tensor_names(cfg)
    assert sorted(names) == sorted(sd) and len(names) == 58
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_lanet({k: t for k, t in sd.items() if k != "bn3a.running_var"})
    with pytest.raises(backend.ImcuiHipError, match="unexpected"):
        backend.pack_lanet({**sd, "conv5a.weight": torch.zeros(1)})
    with pytest.raises(backend.ImcuiHipError, match="shape"):
        backend.pack_lanet({**sd, "convPb.weight": torch.zeros(3, 256, 3, 3)})
    with pytest.raises(backend.ImcuiHipError, match="1x1 or 3x3"):
        backend.pack_lanet({**sd, "des_conv2.weight": torch.zeros(256, 64, 5, 5)})
    with pytest.raises(backend.ImcuiHipError, match="multiples of 32"):
        backend.pack_lanet(lib_state(lanet_synth_state(0, widths=(32, 48, 128, 256))))
    with pytest.raises(backend.ImcuiHipError, match="level 4"):
        backend.pack_lanet(lib_state(lanet_synth_state(0, widths=(32, 64, 128, 128))))
    with pytest.raises(backend.ImcuiHipError, match="activation"):
        backend.pack_lanet(sd, "gelu")
    bad = (backend.C.c_int * 12)(32, 64, 128, 256, 2, 3, 1, 1, 0, 0, 1, 0)
    assert lib.imcui_hip_lanet_packed_floats(bad) == 0 and lib.imcui_hip_lanet_num_tensors(bad) == 0 and lib.imcui_hip_lanet_workspace_bytes(bad, 1, 64, 64, 8) == 0
    assert lib.imcui_hip_lanet_workspace_bytes(ca, 1, 7, 64, 8) == 0 and lib.imcui_hip_lanet_workspace_bytes(ca, 1, 8, 8, 1) > 0


@pytest.mark.parametrize("k,bias,bn", [(3, True, False), (1, False, True), (3, True, True), (1, True, False)])
def test_packer_round_trips_the_batchnorm_folds(lib, k, bias, bn):
    """The packed layout of csrc/lanet.hip read back at its offsets (every array starts at a multiple of 64 floats) and evaluated in
    float64: conv1a [tap][cin][c1] + bias equals F.batch_norm(conv1a(x)); the K-major weights [k k C][256] and the bias of des_conv2
    equal des_bn2(des_conv2(x)) (bias through the BatchNorm, or plain where there is none), to the float32 rounding of the fold."""
    sd = state(0, k, bias, bn)
    packed, cfg = backend.pack_lanet(lib_state(sd))
    assert cfg["k"] == (k, k) and cfg["bias"] == (int(bias),) * 2 and cfg["bn"] == (int(bn),) * 2
    pk = packed.double()
    off = [64]  # the header

    def get(n):
        o = off[0]
        off[0] += (n + 63) // 64 * 64
        return o

    p = R.PREFIX
    c1, c2, c3, c4 = cfg["widths"]
    w0, b0 = get(27 * c1), get(c1)
    for cin, cout in ((32, c1), (c1, c1), (c1, c2), (c2, c2), (c2, c3), (c3, c3), (c3, c4), (c4, c4), (c4, 256), (c4, 256)):
        K = 9 * cin
        get(cout * K), get(cout), get(cout * K // 2), get(cout * K // 2), get(1)
    get(9 * 256 * 4), get(9 * 256 * 2), get(6)
    K2 = k * k * c2
    dw, db = get(K2 * 256), get(256)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 3, 12, 14, generator=g, dtype=torch.float64)
    w = pk[w0 : w0 + 27 * c1].reshape(3, 3, 3, c1).permute(3, 2, 0, 1).contiguous()
    want = F.batch_norm(F.conv2d(x, sd[f"{p}conv1a.weight"].double(), padding=1), sd[f"{p}bn1a.running_mean"].double(), sd[f"{p}bn1a.running_var"].double(),
                        sd[f"{p}bn1a.weight"].double(), sd[f"{p}bn1a.bias"].double(), False, 0.0, 1e-5)  # fmt: skip
    err0 = ((want - F.conv2d(x, w, pk[b0 : b0 + c1], padding=1)).abs().max() / want.abs().max()).item()
    x2 = torch.randn(1, c2, 9, 11, generator=g, dtype=torch.float64)
    w2 = pk[dw : dw + K2 * 256].reshape(k, k, c2, 256).permute(3, 2, 0, 1).contiguous()
    want2 = F.conv2d(x2, sd[f"{p}des_conv2.weight"].double(), sd[f"{p}des_conv2.bias"].double() if bias else None, padding=k // 2)
    if bn:
        want2 = F.batch_norm(want2, *(sd[f"{p}des_bn2.{n}"].double() for n in ("running_mean", "running_var", "weight", "bias")), False, 0.0, 1e-5)
    err2 = ((want2 - F.conv2d(x2, w2, pk[db : db + 256], padding=k // 2)).abs().max() / want2.abs().max()).item()
    print(f"k={k} bias={bias} bn={bn}: folded conv1a {err0:.2e}, folded des_conv2 {err2:.2e} against F.batch_norm in float64")
    assert err0 < 1e-6 and err2 < 1e-6


# ------------------------------------------------------------------ the host layer
def test_check_args_refusals():
    with pytest.raises(ValueError, match="RGB"):
        backend.lanet_check_args((1, 1, 64, 64))
    with pytest.raises(ValueError, match="at least 8"):
        backend.lanet_check_args((1, 3, 7, 64))
    with pytest.raises(ValueError, match="at least 8"):
        backend.lanet_check_args((1, 3, 64, 6))
    with pytest.raises(ValueError, match="negative"):
        backend.lanet_check_args((1, 3, 64, 64), -1)
    backend.lanet_check_args((2, 3, 8, 8), 0)


def test_plugin_contract_and_refusals(lib):
    from imcui_hip.hloc import extract_features, extractors
    from imcui_hip.hloc.extractors.lanet import LANet
    from imcui_hip.hloc.utils.base_model import dynamic_load

    assert dynamic_load(extractors, "lanet") is LANet
    assert LANet.default_conf == {"model_name": "PointModel_v0.pth", "keypoint_threshold": 0.1, "max_keypoints": 1024}
    assert LANet.required_inputs == ["image"] and LANet.takes_rgb
    assert extract_features.confs["lanet"] == {"output": "feats-lanet-n5000-r1600", "model": {"name": "lanet", "keypoint_threshold": 0.1, "max_keypoints": 5000},
                                               "preprocessing": {"grayscale": False, "resize_max": 1600}}  # fmt: skip
    m = LANet({"name": "lanet", "state_dict": {"model_state": state()}})  # the reference's container key
    assert "state_dict" not in m.conf and m.packed.dtype == torch.float32 and not m.packed.is_cuda
    assert torch.equal(LANet({"state_dict": state()}).packed, m.packed)
    assert LANet({"state_dict": state(), "activation": "leaky_relu"}).packed[11].item() == 2.0
    with pytest.raises(backend.ImcuiHipError, match="ROCm device"):  # no CPU fallback
        m({"image": torch.zeros(1, 3, 64, 64)})
    with pytest.raises(ValueError, match="RGB"):
        m({"image": torch.zeros(1, 1, 64, 64)})
    with pytest.raises(ValueError, match="at least 8"):
        m({"image": torch.zeros(1, 3, 7, 64)})
    m.conf["max_keypoints"] = -3  # read on every call
    with pytest.raises(ValueError, match="negative"):
        m({"image": torch.zeros(1, 3, 64, 64)})
    with pytest.raises(ValueError, match="negative"):
        LANet({"state_dict": state(), "max_keypoints": -1})
    with pytest.raises(backend.ImcuiHipError, match="key table"):
        LANet({"state_dict": {**state(), "interestpoint_module.conv5a.weight": torch.zeros(1)}})
    with pytest.raises(backend.ImcuiHipError, match="key table"):
        LANet({"state_dict": {k.replace("interestpoint_module.", ""): t for k, t in state().items()}})
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        LANet({"state_dict": {k: t for k, t in state().items() if not k.endswith("convDb.bias")}})
    with pytest.raises(backend.ImcuiHipError, match="multiples of 32"):
        LANet({"state_dict": lanet_synth_state(0, widths=(32, 64, 100, 256))})
    with pytest.raises(backend.ImcuiHipError, match="activation"):
        LANet({"state_dict": state(), "activation": "elu"})
