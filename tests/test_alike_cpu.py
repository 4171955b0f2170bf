"""ALIKE without a GPU: the restatement (tests/alike_reference.py) itself, the seeded weights' operating point, upstream's float32
coordinate round trip, the refusals of the host layer and the strict packer with its BatchNorm fold."""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

from alike_reference import CFG, ALIKEReference, banded_nms, bilinear_zero, keypoints_from, select
from imcui_hip import backend
from imcui_hip.synth_weights import alike_state_dict
from test_aliked_cpu import image

BASE = dict(top_k=-1, detection_threshold=0.5, max_keypoints=5000, sub_pixel=False)
SEEDED = [(64, 64, 1), (100, 150, 2), (160, 224, 3)]  # the images of the GPU tests
VARIANTS = ("alike-t", "alike-s", "alike-n")


@functools.lru_cache(maxsize=None)
def _sd(variant, fallback=False):
    return alike_state_dict(variant, 0, fallback=fallback)


@functools.lru_cache(maxsize=None)
def _ref(variant, fallback=False):
    return ALIKEReference(_sd(variant, fallback), variant)


@functools.lru_cache(maxsize=None)
def _score(variant, hws, fallback=False):
    return _ref(variant, fallback).dense(image(*hws))["score_map"][0, 0]


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("variant,count", [("alike-t", 82728), ("alike-s", 175992), ("alike-n", 329168)])
def test_parameter_count_and_strict_load(variant, count):
    """3x3 convolutions without bias, BatchNorm weight and bias, shortcuts with bias, four 1x1 branch heads and convhead2 (dim + 1 rows):
    counted by hand from the channel table."""
    c1, c2, c3, c4, dim = CFG[variant]
    ch = [3, c1, c2, c3, c4]
    by_hand = sum(9 * ch[b - 1] * ch[b] + 9 * ch[b] * ch[b] + 4 * ch[b] + (ch[b - 1] * ch[b] + ch[b] if b >= 2 else 0) for b in range(1, 5))
    by_hand += sum(dim // 4 * c for c in ch[1:]) + (dim + 1) * dim
    ref = ALIKEReference(None, variant)
    assert sum(p.numel() for p in ref.parameters()) == by_hand == count
    missing, unexpected = ref.load_state_dict({k: v for k, v in _sd(variant).items() if not k.endswith("num_batches_tracked")}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)


def test_padded_and_cropped_shapes_at_100x150():
    d = _ref("alike-t").dense(image(100, 150, 2))
    assert d["score_map"].shape == (1, 1, 100, 150) and d["descriptor_map"].shape == (1, 64, 100, 150)
    assert d["x4"].shape == (1, 64, 4, 5) and d["f2"].shape == (1, 16, 64, 80) and d["f3"].shape == (1, 16, 16, 20) and d["f4"].shape == (1, 16, 4, 5)
    assert (d["descriptor_map"].norm(dim=1) - 1).abs().max().item() < 1e-5
    with pytest.raises(AssertionError):
        _ref("alike-t").dense(torch.zeros(1, 1, 64, 64))


def test_translation_by_32_pixels_moves_interior_keypoints_by_32_pixels():
    """Two 128 x 256 windows of one image, 32 px apart.  The full-resolution branch and the convolutions are translation-equivariant in
    steps of the stride away from the borders; the align_corners up-sampling is not quite: a branch at 1/s maps pixel x to
    x (W / s - 1) / (W - 1), so a 32 px shift registers the 1/32 branch 31 / (W - 1) = 0.12 cells (4 px) off and the 1/8 branch 1 px off.
    Those branches are smooth, they tilt a local maximum of the score by a pixel at most, so an interior key-point of one window has a
    key-point of the other within 1 px of its shifted position, and a large share sits exactly 32 px further.  Measured with the seeded
    alike-t: 475 interior key-points, 262 (55 %) exactly 32 px further, 389 (82 %) within 1 px; required: 40 % and 75 %.  (Unrelated
    lists would pair far less often: NMS survivors are at least 3 px apart, so a 3 x 3 window holds at most one of them.)"""
    W = 256
    big = image(128, W + 32, 9)
    a, b = big[..., :W], big[..., 32:]
    ref = _ref("alike-t")
    conf = {**BASE, "detection_threshold": -1.0}
    ia = select(ref.dense(a)["score_map"][0, 0], conf)[0]
    ib = select(ref.dense(b)["score_map"][0, 0], conf)[0]
    pa = {(int(i) // W, int(i) % W) for i in ia}
    pb = {(int(i) // W, int(i) % W + 32) for i in ib}  # in a's coordinates
    inner_a = {p for p in pa if 40 <= p[1] < W - 8 and 8 <= p[0] < 120}
    exact = len(inner_a & pb)
    near = sum(any((p[0] + dy, p[1] + dx) in pb for dy in (-1, 0, 1) for dx in (-1, 0, 1)) for p in inner_a)
    print(f"{len(inner_a)} interior key-points of window a: {exact} found exactly 32 px further in window b, {near} within 1 px of that")
    assert len(inner_a) > 100 and exact >= 0.4 * len(inner_a) and near >= 0.75 * len(inner_a)


def test_selection_rules_on_hand_made_maps():
    sm = torch.full((24, 32), 0.1)
    pts = {(2, 10): 0.9, (10, 2): 0.9, (22, 14): 0.97, (14, 30): 0.98, (3, 14): 0.95, (14, 3): 0.96, (21, 10): 0.9, (10, 29): 0.9,
           (12, 16): 0.7, (16, 8): 0.7, (6, 20): 0.6, (18, 24): 0.5}  # fmt: skip
    for (y, x), v in pts.items():
        sm[y, x] = v
    # rows / columns 0..2 and the last two are outside the band: row 2 / column 2 / row 22 / column 30 leave, row 3 / column 3 / row 21 / column 29 stay
    idx, branch, cut = select(sm, BASE)
    assert branch == "threshold" and not cut  # 0.5 itself is not > 0.5
    assert idx.tolist() == [3 * 32 + 14, 6 * 32 + 20, 10 * 32 + 29, 12 * 32 + 16, 14 * 32 + 3, 16 * 32 + 8, 21 * 32 + 10]
    idx, _, cut = select(sm, {**BASE, "max_keypoints": 4})  # the cut reorders by score; the two 0.9s tie: the lower index first
    assert cut and idx.tolist() == [14 * 32 + 3, 3 * 32 + 14, 10 * 32 + 29, 21 * 32 + 10]
    idx, _, cut = select(sm, {**BASE, "max_keypoints": 5})  # of the two 0.7s the lower index stays
    assert cut and idx.tolist() == [14 * 32 + 3, 3 * 32 + 14, 10 * 32 + 29, 21 * 32 + 10, 12 * 32 + 16]
    idx, branch, cut = select(sm, {**BASE, "top_k": 6})
    assert branch == "topk" and cut and idx.tolist() == [14 * 32 + 3, 3 * 32 + 14, 10 * 32 + 29, 21 * 32 + 10, 12 * 32 + 16, 16 * 32 + 8]
    idx, branch, cut = select(sm, {**BASE, "top_k": 5000})  # more than the positive survivors: only those, never zero-score pixels
    assert branch == "topk" and not cut and (banded_nms(sm).reshape(-1)[idx] > 0).all() and len(idx) == int((banded_nms(sm) > 0).sum())
    low = torch.full((24, 32), 0.05)
    low[8, 8], low[16, 20] = 0.15, 0.12
    idx, branch, _ = select(low, BASE)
    assert branch == "mean" and idx.tolist() == [8 * 32 + 8, 16 * 32 + 20]
    assert select(low, {**BASE, "detection_threshold": -1.0})[1] == "mean"


def test_explicit_bilinear_is_grid_sample():
    """`bilinear_zero` against F.grid_sample(align_corners=True) in float64, where the two operation orders agree to round-off."""
    g = torch.Generator().manual_seed(3)
    x = torch.rand(5, 20, 30, generator=g, dtype=torch.float64)
    fx, fy = torch.rand(200, generator=g, dtype=torch.float64) * 31 - 1, torch.rand(200, generator=g, dtype=torch.float64) * 21 - 1
    grid = torch.stack([fx / 29 * 2 - 1, fy / 19 * 2 - 1], 1).view(1, 1, -1, 2)
    want = F.grid_sample(x[None], grid, mode="bilinear", align_corners=True)[0, :, 0].t()
    assert (bilinear_zero(x, fx, fy) - want).abs().max().item() < 1e-12


# ------------------------------------------------------------------ the seeded weights' operating point
@pytest.mark.parametrize("variant", VARIANTS)
def test_default_threshold_decides_on_the_seeded_networks(variant):
    """On the seeded images the 0.5 threshold keeps between 10 % and 90 % of the NMS survivors; the fallback weights leave nothing above
    it and take the mean route; n_limit 50 is exceeded where the GPU test takes the cut."""
    for hws in SEEDED:
        sm = _score(variant, hws)
        nms = banded_nms(sm)
        surv, above = int((nms > 0).sum()), int((nms > 0.5).sum())
        print(f"{variant} {hws[0]}x{hws[1]}: {surv} NMS survivors, {above} above 0.5, score mean {sm.mean().item():.3f}")
        assert 0.1 * surv < above < 0.9 * surv
        assert select(sm, BASE)[1] == "threshold"
        low = _score(variant, hws, True)
        idx, branch, _ = select(low, BASE)
        assert branch == "mean" and low.max().item() < 0.5 and 0 < idx.numel() < surv
        if hws[0] >= 100:
            idx, _, cut = select(sm, {**BASE, "max_keypoints": 50})
            assert cut and idx.numel() == 50 and above > 50


@pytest.mark.parametrize("variant", VARIANTS)
def test_float32_round_trip_truncates_a_coordinate_of_every_seeded_image(variant):
    """`idx / (w - 1) * 2 - 1` -> `(n + 1) / 2 * (w - 1)` in float32 comes back below the integer for some coordinates, and the descriptor
    pixel is the truncation: if no key-point of a seeded image were affected, the GPU test would not see the quirk."""
    for hws in SEEDED:
        sm = _score(variant, hws)
        h, w = sm.shape
        idx = select(sm, BASE)[0]
        _, kp, _, pix = keypoints_from(sm, idx, False)
        cand = torch.stack([idx % w, idx // w], 1)
        moved = (pix != cand).any(dim=1)
        assert int(moved.sum()) >= 1, hws
        assert ((cand - pix)[moved].max().item() == 1) and ((cand - pix).min().item() == 0)  # one pixel lower, never higher
        assert (kp - cand).abs().max().item() < 1e-3
        _, kp64, _, pix64 = keypoints_from(sm.double(), idx, False)
        print(f"{variant} {hws[0]}x{hws[1]}: {int(moved.sum())} of {len(idx)} key-points read the neighbouring pixel ({int((pix64 != cand).any(dim=1).sum())} in float64)")


# ------------------------------------------------------------------ host layer
def test_check_args_refusals():
    with pytest.raises(backend.ImcuiHipError, match="alike-l.*second head layer"):
        backend.alike_check_args((1, 3, 64, 64), "alike-l")
    with pytest.raises(backend.ImcuiHipError, match="not served"):
        backend.alike_check_args((1, 3, 64, 64), "alike-x")
    with pytest.raises(ValueError, match="RGB"):
        backend.alike_check_args((1, 1, 64, 64), "alike-t")
    with pytest.raises(ValueError, match="at least 32"):
        backend.alike_check_args((1, 3, 31, 64), "alike-t")
    backend.alike_check_args((2, 3, 32, 40), "alike-n")


def test_plugin_contract_and_refusals():
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.extractors.alike import Alike
    from imcui_hip.hloc.utils.base_model import dynamic_load

    assert dynamic_load(extractors, "alike") is Alike
    assert Alike.default_conf == {"model_name": "alike-t", "use_relu": True, "multiscale": False, "max_keypoints": 1000,
                                  "detection_threshold": 0.5, "top_k": -1, "sub_pixel": False}  # fmt: skip
    assert Alike.required_inputs == ["image"] and Alike.takes_rgb
    m = Alike({"name": "alike", "state_dict": _sd("alike-t"), "use_relu": False, "multiscale": True})  # accepted and unused
    assert "state_dict" not in m.conf and m.packed.dtype == torch.float32 and not m.packed.is_cuda
    with pytest.raises(backend.ImcuiHipError, match="alike-l"):
        Alike({"model_name": "alike-l", "state_dict": _sd("alike-n")})
    with pytest.raises(backend.ImcuiHipError, match="ROCm device"):  # no CPU fallback
        m({"image": torch.zeros(1, 3, 64, 64)})
    with pytest.raises(ValueError, match="RGB"):
        m({"image": torch.zeros(1, 1, 64, 64)})


# ------------------------------------------------------------------ the packer
@pytest.mark.parametrize("variant", VARIANTS)
def test_pack_is_strict(lib, variant):
    sd = dict(_sd(variant))
    v = backend.ALIKE_MODELS[variant]
    names = backend.alike_tensor_names(variant)
    assert names == [k for k in ALIKEReference(None, variant).state_dict() if not k.endswith("num_batches_tracked")]
    shapes = backend.alike_tensor_shapes(variant)
    assert {k: tuple(t.shape) for k, t in ALIKEReference(None, variant).state_dict().items() if k in shapes} == shapes and len(shapes) == len(names) == 51
    packed = backend.pack_alike(sd, variant)
    assert packed.numel() == lib.imcui_hip_alike_packed_floats(v) > 0
    assert torch.equal(backend.pack_alike({k: t for k, t in sd.items() if not k.endswith("num_batches_tracked")}, variant), packed)  # counters ignored
    with pytest.raises(backend.ImcuiHipError, match="missing"):
        backend.pack_alike({k: t for k, t in sd.items() if k != "block3.downsample.bias"}, variant)
    with pytest.raises(backend.ImcuiHipError, match="unexpected"):
        backend.pack_alike({**sd, "convhead1.weight": torch.zeros(1)}, variant)
    with pytest.raises(backend.ImcuiHipError, match="shape"):
        backend.pack_alike({**sd, "conv4.weight": torch.zeros(7, 3, 1, 1)}, variant)
    with pytest.raises(backend.ImcuiHipError, match="not served"):
        backend.pack_alike(sd, "alike-l")
    assert lib.imcui_hip_alike_packed_floats(3) == 0 and lib.imcui_hip_alike_num_tensors(3) == 0 and lib.imcui_hip_alike_workspace_bytes(3, 1, 64, 64) == 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_batchnorm_is_folded_into_the_first_convolution(lib, variant):
    """The packed buffer begins with block1.conv1 folded with block1.bn1 as [9][3][c1] + c1 biases (include/imcui_hip.h): a convolution
    with those equals F.batch_norm(conv1(x)) evaluated in float64 to float32 round-off."""
    sd = _sd(variant)
    c1 = CFG[variant][0]
    packed = backend.pack_alike(sd, variant)
    nw = 9 * 3 * c1
    off_b = (nw + 63) // 64 * 64
    w = packed[:nw].reshape(3, 3, 3, c1).permute(3, 2, 0, 1).contiguous().double()  # [ky][kx][ci][co] -> OIHW
    b = packed[off_b : off_b + c1].double()
    x = torch.randn(1, 3, 20, 24, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    want = F.batch_norm(F.conv2d(x, sd["block1.conv1.weight"].double(), padding=1), sd["block1.bn1.running_mean"].double(),
                        sd["block1.bn1.running_var"].double(), sd["block1.bn1.weight"].double(), sd["block1.bn1.bias"].double(), False, 0.0, 1e-5)  # fmt: skip
    got = F.conv2d(x, w, b, padding=1)
    err = (want - got).abs().max().item() / want.abs().max().item()
    print(f"{variant}: folded block1.conv1 against F.batch_norm in float64: {err:.2e}")
    assert err < 1e-6


@pytest.mark.parametrize("variant", VARIANTS)
def test_packed_buffer_evaluated_with_torch_reproduces_the_dense_maps(lib, variant):
    """The whole packed layout of csrc/alike.hip (block 1 as [tap][cin][cout], the six GEMM layers [N stored][tap][cin stored] with the
    BatchNorm fold and zero padding, the shortcuts, the transposed branch heads, the score row and the K-major descriptor rows), read
    back at the offsets the layout comment gives (every array starts at a multiple of 64 floats) and evaluated in float64 with
    F.conv2d: x4, f4, the score map and the descriptor map equal the restatement's to the float32 rounding of the folded weights."""
    c1, c2, c3, c4, dim = CFG[variant]
    dq = dim // 4
    P = [0, 32] + [(c + 31) // 32 * 32 for c in (c2, c3, c4)]
    sd = _sd(variant)
    pk = backend.pack_alike(sd, variant).double()
    off = [0]

    def get(n):
        o = off[0]
        off[0] += (n + 63) // 64 * 64
        return o

    vw0, vb0, vw1, vb1 = get(27 * c1), get(c1), get(9 * c1 * c1), get(c1)
    gcin, gn, G = [P[1], P[2], P[2], P[3], P[3], P[4]], [P[2], P[2], P[3], P[3], P[4], P[4]], []
    for g in range(6):
        K = 9 * gcin[g]
        G.append((get(gn[g] * K), get(gn[g]), K))
        get(gn[g] * K // 2), get(gn[g] * K // 2), get(1)  # the two f16 planes and their scale
    D = [(get(P[i + 1] * P[i + 2]), get(P[i + 2])) for i in range(3)]
    cw = [get(c1 * dq)] + [get(P[i + 1] * dq) for i in range(1, 4)]
    sw, wdt = get(dim), get(dim * dim)
    assert off[0] == pk.numel()

    def conv_valu(x, wo, bo, cin, cout):
        w = pk[wo : wo + 9 * cin * cout].reshape(3, 3, cin, cout).permute(3, 2, 0, 1)
        return F.relu(F.conv2d(x, w, pk[bo : bo + cout], padding=1))

    def conv_gemm(x, g, resid=None):
        gw, gb, K = G[g]
        w = pk[gw : gw + gn[g] * K].reshape(gn[g], 3, 3, gcin[g]).permute(0, 3, 1, 2)
        y = F.conv2d(x, w, pk[gb : gb + gn[g]], padding=1)
        return F.relu(y if resid is None else y + resid)

    def shortcut(x, i):
        wo, bo = D[i]
        w = pk[wo : wo + P[i + 1] * P[i + 2]].reshape(P[i + 1], P[i + 2]).t()[:, :, None, None]
        return F.conv2d(x, w, pk[bo : bo + P[i + 2]])

    img = image(100, 150, 2).double()
    ref = ALIKEReference(sd, variant).double()
    d = ref.dense(img)
    x1 = conv_valu(conv_valu(ref.pad(img * 255.0 / 255.0), vw0, vb0, 3, c1), vw1, vb1, c1, c1)
    p = F.pad(F.max_pool2d(x1, 2), (0, 0, 0, 0, 0, 32 - c1))
    xs = []
    for b, k in ((0, 4), (1, 4), (2, None)):
        xs.append(conv_gemm(conv_gemm(p, 2 * b), 2 * b + 1, shortcut(p, b)))
        p = F.max_pool2d(xs[-1], k) if k else None
    assert not xs[2][:, c4:].any()  # the channel padding stays zero
    fs = []
    for i, xm in enumerate([x1] + xs):
        cin = c1 if i == 0 else P[i + 1]
        fs.append(F.relu(F.conv2d(xm, pk[cw[i] : cw[i] + cin * dq].reshape(cin, dq).t()[:, :, None, None])))
    x1234 = torch.cat([fs[0]] + [F.interpolate(t, scale_factor=s, mode="bilinear", align_corners=True) for t, s in zip(fs[1:], (2, 8, 32))], 1)
    score = torch.sigmoid(F.conv2d(x1234, pk[sw : sw + dim][None, :, None, None]))[:, :, :100, :150]
    desc = F.normalize(F.conv2d(x1234, pk[wdt : wdt + dim * dim].reshape(dim, dim).t()[:, :, None, None]), dim=1)[:, :, :100, :150]
    errs = {"x4": (xs[2][:, :c4] - d["x4"]).abs().max().item() / d["x4"].abs().max().item(), "f4": (fs[3] - d["f4"]).abs().max().item() / d["f4"].abs().max().item(),
            "score": (score - d["score_map"]).abs().max().item(), "descriptor": (desc - d["descriptor_map"]).abs().max().item()}  # fmt: skip
    print(variant, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < 1e-5  # float32 weights, ~100 roundings deep; measured 4e-8 .. 2e-6 absolute


def test_workspace_and_bound(lib):
    for v, (c1, c2, c3, c4, dim) in zip((0, 1, 2), (CFG[k] for k in VARIANTS)):
        for H, W in ((32, 40), (100, 150), (480, 640)):
            Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
            ws = lib.imcui_hip_alike_workspace_bytes(v, 4, H, W)
            assert 0 < ws < 4 * Hp * Wp * (dim + 1) * 4, (v, H, W)  # less than the dense (dim + 1)-channel map it never writes
    sm = _score("alike-t", SEEDED[2])
    assert int((banded_nms(sm) > 0).sum()) <= lib.imcui_hip_alike_max_keypoints_bound(160, 224)


def test_alike_conf_runs_on_the_device_resize():
    """The `alike` conf (grayscale False, resize_max 1600): the batch extractor's device preprocessing takes it."""
    from types import SimpleNamespace

    from imcui_hip.hloc import extract_features as ef

    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, "grayscale": False, "resize_max": 1600})
    assert ef.target_size((3200, 2400), pconf) == (1600, 1200)
    assert ef.target_size((640, 480), pconf) is None
