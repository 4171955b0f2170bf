"""XFeat on the MI355X (imcui/hloc/extractors/xfeat.py:26-34 -> upstream's XFeat.detectAndCompute) against the CPU restatement
(tests/xfeat_reference.py), in both arithmetic modes: the dense maps, the selection rule on the HIP maps (exact), the end-to-end
key-point sets (equal, or every difference an audited round-off tie), descriptors at common key-points, the three sampling rules at
every integer pixel, batch independence, graph replay, the edge cases of the rule and the plugin's output contract.

Measured on one MI355X, both arithmetic modes, all five sizes (profiles/xfeat_parity.txt keeps the lines this file prints): dense maps
within 5.2e-6 of the restatement relative to the map's largest magnitude (M1 1.2e-6, K1h 1.5e-6, reliability 5.2e-6; the bar
max(1e-4, 3 x oracle spread) is 1e-4 everywhere, the restatement's own spread up to 2.3e-6), descriptors at common key-points within
4.8e-7, scores within 5.0e-7, no end-to-end key-point difference at any size; sampling rules on the 64 x 96 image: nearest and bilinear
bit for bit, bicubic within 2.6e-7."""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

import xfeat_reference as xr
from parity_utils import oracle_spread

pytestmark = pytest.mark.gpu

THR = xr.DETECTION_THRESHOLD
# size -> (H, W, seed, top_k of the parity case)
SIZES = {"64x64": (64, 64, 0, -1), "96x128": (96, 128, 1, -1), "100x150": (100, 150, 2, -1), "160x224": (160, 224, 3, 5000), "480x640": (480, 640, 0, 1000)}


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


@functools.lru_cache(maxsize=None)
def _net():
    return xr.load_model(_sd())


@functools.lru_cache(maxsize=None)
def _oracle(size: str):
    """(image, the restatement's dense maps, their fp32 spread over intra-op thread counts)."""
    h, w, seed, _ = SIZES[size]
    img = _image(h, w, seed)
    spread, maps = oracle_spread(lambda: xr.dense_maps(_net(), img), threads=(1, 8), keys=("M1", "K1h", "reliability"))
    return img, maps, spread


def _model(top_k=-1, sd=None):
    from imcui_hip.hloc.extractors.xfeat import XFeat

    return XFeat({"max_keypoints": top_k, "state_dict": sd if sd is not None else _sd()}).eval().to("cuda:0")


def _hip(model, img, **kw):
    out = model.forward_batched(img.cuda(), want_dense=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _hip_maps(out, b=0):
    """The HIP dense maps of image b in the restatement's layout."""
    return out["feats_norm"][b].permute(2, 0, 1)[None].contiguous(), out["kpt_heat"][b][None, None], out["reliability"][b][None, None]


def _lists(out, b=0):
    n = int(out["num_keypoints"][b])
    return out["keypoints"][b, :n], out["scores"][b, :n], out["descriptors"][b, :n], n


def _assert_rule(out, rh, rw, top_k, b=0, threshold=THR):
    """(2) The restatement's rule applied to the HIP maps reproduces the HIP list: coordinates, order up to exact score ties, scores."""
    kp, sc, de, n = _lists(out, b)
    rule = xr.select(*_hip_maps(out, b), rh, rw, top_k, threshold)
    assert n == len(rule["scores"]), (n, len(rule["scores"]))
    assert torch.all(out["keypoints"][b, n:] == 0) and torch.all(out["scores"][b, n:] == 0) and torch.all(out["descriptors"][b, n:] == 0)
    if n == 0:
        return rule
    assert (sc - rule["scores"]).abs().max().item() <= 1e-6
    assert torch.all(sc[1:] <= sc[:-1]) and sc[-1] > 0
    if not torch.equal(kp, rule["keypoints"]):  # only members of an exact score tie may sit elsewhere
        where = {tuple(p): i for i, p in enumerate(rule["keypoints"].tolist())}
        for i, p in enumerate(kp.tolist()):
            assert tuple(p) in where, p
            assert rule["scores"][where[tuple(p)]] == rule["scores"][i], (i, p)
        assert len({tuple(p) for p in kp.tolist()}) == n
    else:
        assert (de - rule["descriptors"]).abs().max().item() <= 1e-5
    return rule


def _audit(rule_h, sel_r, maps_h, maps_r, top_k, tag):
    """(3) Every key-point in one set but not the other must be a round-off tie: its margin against the threshold or a pixel of its NMS
    window (on K1h), or against the cut-off / zero (on the score = K1h x reliability, whose error is at most the sum of the two maps'
    errors, both maps being at most 1), below twice the measured map difference.  Returns the number of audited differences."""
    K_r, K_h = maps_r["K1h"][0, 0], maps_h[1][0, 0]
    d_k = (K_h - K_r).abs().max().item()
    d_s = d_k + (maps_h[2] - maps_r["reliability"]).abs().max().item()
    sh = {tuple(p) for p in rule_h["xy"].tolist()}
    sr = {tuple(p) for p in sel_r["xy"].tolist()}
    H, W = K_r.shape
    every = xr.select(maps_r["M1"], maps_r["K1h"], maps_r["reliability"], 1.0, 1.0, H * W)  # the reference's uncut list
    score_of = {tuple(p): s for p, s in zip(every["xy"].tolist(), every["scores"].tolist())}
    cuts = [s["scores"][-1].item() for s in (rule_h, sel_r) if len(s["scores"])] if len(every["scores"]) > len(sel_r["scores"]) else []
    for x, y in sorted(sh ^ sr):
        v = K_r[y, x].item()
        win = K_r[max(0, y - 2) : y + 3, max(0, x - 2) : x + 3].clone()
        win[y - max(0, y - 2), x - max(0, x - 2)] = float("inf")  # the pixel itself; an exactly equal neighbour is a tie (margin 0)
        m_map = min(abs(v - THR), (win - v).abs().min().item())
        s = score_of.get((x, y))
        m_score = min([abs(s - c) for c in cuts] + [abs(s)]) if s is not None else float("inf")
        if not (m_map < 2 * d_k or m_score < 2 * d_s):
            raise AssertionError(f"{tag}: key-point ({x}, {y}) differs with margins {m_map:.3e} (map) / {m_score:.3e} (score) >= 2 x {d_k:.3e} / {d_s:.3e}")
    assert len(sh ^ sr) <= max(2, 0.01 * len(sr)), (tag, len(sh ^ sr), len(sr))
    return len(sh ^ sr)


@pytest.mark.parametrize("size", list(SIZES))
def test_xfeat_vs_restatement(precision, size):
    h, w, _, top_k = SIZES[size]
    img, maps_r, spread = _oracle(size)
    out = _hip(_model(top_k), img)
    assert int(out["status"][0]) == 0
    bar = max(1e-4, 3 * spread)
    # (1) dense maps
    maps_h = _hip_maps(out)
    errs = {}
    for name, got in zip(("M1", "K1h", "reliability"), maps_h):
        assert got.shape == maps_r[name].shape, (name, got.shape, maps_r[name].shape)
        errs[name] = (got - maps_r[name]).abs().max().item() / maps_r[name].abs().max().item()
        assert errs[name] <= bar, (size, name, errs[name], bar)
    # (2) the restated rule on the HIP maps
    rule_h = _assert_rule(out, maps_r["rh"], maps_r["rw"], top_k)
    # (3) end to end: the reference's key-points, or audited ties
    sel_r = xr.select(maps_r["M1"], maps_r["K1h"], maps_r["reliability"], maps_r["rh"], maps_r["rw"], top_k)
    ties = _audit(rule_h, sel_r, maps_h, maps_r, top_k, f"{size}")
    kp, sc, de, n = _lists(out)
    assert n > (3 if size == "64x64" else 20), n
    # (4) descriptors and scores at the common key-points
    pos_r = {tuple(p): i for i, p in enumerate(sel_r["xy"].tolist())}
    common = [(i, pos_r[tuple(p)]) for i, p in enumerate(rule_h["xy"].tolist()) if tuple(p) in pos_r]
    ih, ir = (torch.tensor(t, dtype=torch.long) for t in zip(*common))
    derr = (de[ih] - sel_r["descriptors"][ir]).abs().max().item()
    serr = (sc[ih] - sel_r["scores"][ir]).abs().max().item()
    assert derr <= bar and serr <= bar, (derr, serr, bar)
    assert torch.equal(kp[ih], sel_r["keypoints"][ir])
    assert torch.allclose(de.norm(dim=1), torch.ones(n), atol=1e-5)
    print(f"[xfeat] {size} top_k={top_k} precision={precision}: n={n} M1 {errs['M1']:.2e} K1h {errs['K1h']:.2e} reliability {errs['reliability']:.2e} "
          f"(bar {bar:.1e}, spread {spread:.1e}) desc {derr:.2e} score {serr:.2e} ties {ties}")  # fmt: skip


def test_xfeat_sampling_rules_at_every_integer_pixel():
    """(5) nearest / bilinear / bicubic of the kernels against F.grid_sample on the CPU at EVERY integer (x, y) of a 64 x 96 image:
    nearest bit for bit, the others to 1e-6."""
    from imcui_hip import backend

    H, W = 64, 96
    g = torch.Generator().manual_seed(5)
    K1h = torch.rand(1, 1, H, W, generator=g)
    rel = torch.rand(1, 1, H // 8, W // 8, generator=g)
    M1 = F.normalize(torch.randn(1, 64, H // 8, W // 8, generator=g), dim=1)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    xy = torch.stack([xs.reshape(-1), ys.reshape(-1)], -1)
    want_n = xr.sample(K1h, xy[None], H, W, "nearest")[0, :, 0]
    want_b = xr.sample(rel, xy[None], H, W, "bilinear")[0, :, 0]
    want_c = xr.sample(M1, xy[None], H, W, "bicubic")[0]
    near, bil, cub = backend.XFeatHIP().sample_probe(K1h[0, 0].cuda(), rel[0, 0].cuda(), M1[0].permute(1, 2, 0).contiguous().cuda(), xy)
    torch.cuda.synchronize()
    assert torch.equal(near.cpu(), want_n)
    assert torch.all(want_n.reshape(H, W)[:, -1] == 0) and torch.all(want_n.reshape(H, W)[-1] == 0)  # the last column / row read zero
    eb, ec = (bil.cpu() - want_b).abs().max().item(), (cub.cpu() - want_c).abs().max().item()
    print(f"[xfeat] sampling 64x96: bilinear {eb:.2e} bicubic {ec:.2e}")
    assert eb <= 1e-6 and ec <= 1e-6, (eb, ec)


def test_xfeat_batch_independence(precision):
    """(6) bit for bit: an image alone against the same image as item 1 of a batch of three different images."""
    m = _model(-1)
    img = _oracle("160x224")[0]
    one = _hip(m, img)
    three = _hip(m, torch.cat([_image(160, 224, 11), img, _image(160, 224, 12)]))
    assert int(one["num_keypoints"][0]) > 20
    for k in ("keypoints", "scores", "descriptors", "num_keypoints", "kpt_heat", "reliability", "feats_norm"):
        n = min(one[k].shape[1], three[k].shape[1]) if k in ("keypoints", "scores", "descriptors") else None
        a, b = (one[k][0], three[k][1]) if n is None else (one[k][0, :n], three[k][1, :n])
        assert torch.equal(a, b), k


def test_xfeat_graph_replay_bitwise(precision):
    """(7)"""
    from imcui_hip.pipeline import GraphedCall

    m = _model(5000)
    img = _oracle("160x224")[0].cuda()
    eager = _hip(m, img)
    g = GraphedCall(lambda x: m.forward_batched(x, want_dense=True), img)
    img2 = _image(160, 224, 21).cuda()
    rep2 = {k: v.cpu() for k, v in g(img2).items()}
    rep = {k: v.cpu() for k, v in g(img).items()}
    eager2 = _hip(m, img2)
    for k in eager:
        assert torch.equal(rep[k], eager[k]), k
        assert torch.equal(rep2[k], eager2[k]), k


def test_xfeat_constant_image_gives_the_restatements_count(precision):
    """(8) A constant image normalises to a constant: every 8x8 cell sees the same input, K1h repeats with period 8 and interior scores tie
    exactly.  The count equals the restatement's, and the restated rule on the HIP maps reproduces the list."""
    m = _model(-1)
    img = torch.full((1, 3, 64, 96), 0.25)
    out, counts = m.forward_checked(img.cuda())
    out = {k: v.cpu() for k, v in m.forward_batched(img.cuda(), want_dense=True, kcap=out["keypoints"].shape[1]).items()}
    want = xr.detect_and_compute(_net(), img, top_k=-1)[0]
    assert counts[0] == int(out["num_keypoints"][0]) == len(want["scores"]), (counts, len(want["scores"]))
    _assert_rule(out, 1.0, 1.0, -1)
    # at the detection threshold the near-uniform soft-max of a blank image yields nothing; with the threshold at zero every local
    # maximum of the periodic map is a candidate
    from imcui_hip import backend

    out0 = {k: v.cpu() for k, v in backend.XFeatHIP().forward(m.packed, img.cuda(), {"max_keypoints": -1}, want_dense=True, kcap=64 * 96, threshold=0.0).items()}
    want0 = xr.detect_and_compute(_net(), img, top_k=-1, threshold=0.0)[0]
    assert int(out0["status"][0]) == 0 and int(out0["num_keypoints"][0]) == len(want0["scores"]) > 8 * 12, (int(out0["num_keypoints"][0]), len(want0["scores"]))
    _assert_rule(out0, 1.0, 1.0, -1, threshold=0.0)


def test_xfeat_flat_keypoint_map_overflows_and_is_retried(precision):
    """(8) One plateau: the last key-point convolution is zero, so K1h is 1/65 everywhere and, at a threshold below it, every pixel is a
    candidate -- more than the NMS bound.  Status bit 1 is raised; with room for every pixel the count is the restatement's."""
    from imcui_hip import backend

    sd = {k: v.clone() for k, v in _sd().items()}
    sd["keypoint_head.3.weight"].zero_()
    sd["keypoint_head.3.bias"].zero_()
    m = _model(-1, sd)
    img = _image(64, 96, 7)
    impl, conf = backend.XFeatHIP(), {"max_keypoints": -1}
    first = impl.forward(m.packed, img.cuda(), conf, threshold=0.01)
    assert int(first["status"][0]) & 2 and int(first["num_keypoints"][0]) == first["keypoints"].shape[1]
    out = {k: v.cpu() for k, v in impl.forward(m.packed, img.cuda(), conf, want_dense=True, kcap=64 * 96, threshold=0.01).items()}
    assert int(out["status"][0]) == 0
    assert torch.all(out["kpt_heat"] == out["kpt_heat"][0, 0, 0]) and abs(out["kpt_heat"][0, 0, 0].item() - 1 / 65) < 1e-6
    rule = _assert_rule(out, 1.0, 1.0, -1, threshold=0.01)
    # every pixel but the last column / row (the nearest sample reads zero) and (0, 0); what [:-1] drops is one of those non-positive entries
    assert len(rule["scores"]) == 63 * 95 - 1
    want = xr.select(*(xr.dense_maps(xr.load_model(sd), img)[k] for k in ("M1", "K1h", "reliability")), 1.0, 1.0, -1, 0.01)
    assert len(want["scores"]) == len(rule["scores"])


def test_xfeat_top_k_rules(precision):
    """(8) top_k = 7 with a distinct eighth score, top_k = -1 (Python's [:-1]), a threshold above every score."""
    from imcui_hip import backend

    img = _oracle("96x128")[0]
    full = _hip(_model(10**6), img)
    kp_f, sc_f, de_f, n_f = _lists(full)
    assert n_f > 8 and sc_f[6] != sc_f[7]
    for top_k, want_n in ((7, 7), (-1, n_f - 1)):
        out = _hip(_model(top_k), img)
        kp, sc, de, n = _lists(out)
        assert n == want_n and int(out["status"][0]) == 0
        assert torch.equal(kp, kp_f[:n]) and torch.equal(sc, sc_f[:n]) and torch.equal(de, de_f[:n])
        _assert_rule(out, 1.0, 1.0, top_k)
    m = _model(-1)
    out = {k: v.cpu() for k, v in backend.XFeatHIP().forward(m.packed, img.cuda(), {"max_keypoints": -1}, threshold=2.0).items()}
    assert int(out["num_keypoints"][0]) == 0 and int(out["status"][0]) == 0
    assert torch.all(out["keypoints"] == 0) and torch.all(out["scores"] == 0) and torch.all(out["descriptors"] == 0)


def test_xfeat_gray_input_equals_three_equal_channels(precision):
    """(8) [B,1,H,W] against the same image repeated to three channels (the channel mean of three equal values is the value)."""
    m = _model(-1)
    for h, w in ((96, 128), (100, 150)):
        gray = _image(h, w, 9)[:, :1].contiguous()
        a, b = _hip(m, gray), _hip(m, gray.repeat(1, 3, 1, 1))
        assert int(a["num_keypoints"][0]) > 5
        for k in a:
            assert torch.equal(a[k], b[k]), (k, h, w)


def test_xfeat_plugin_output_contract():
    """(9) `_forward` returns [1,N,2], [1,N], [1,64,N] on the device, key-points scaled by (rw, rh)."""
    m = _model(-1)
    img = _oracle("100x150")[0].cuda()
    out = m({"image": img})
    n = out["keypoints"].shape[1]
    assert n > 20 and out["keypoints"].shape == (1, n, 2) and out["scores"].shape == (1, n) and out["descriptors"].shape == (1, 64, n)
    assert all(v.dtype == torch.float32 and v.is_contiguous() and v.device.type == "cuda" for v in out.values())
    scale = torch.tensor([150 / 128, 100 / 96])
    kp = out["keypoints"][0].cpu()
    px = (kp / scale).round()
    assert torch.equal(px * scale, kp) and px[:, 0].max() <= 126 and px[:, 1].max() <= 94 and kp[:, 0].max() > 128
    sc = out["scores"][0].cpu()
    assert torch.all(sc[1:] <= sc[:-1]) and sc[-1] > 0
    # the conf is re-read on every call (the UI mutates max_keypoints)
    m.conf["max_keypoints"] = 10
    assert m({"image": img})["keypoints"].shape[1] == 10
    m.conf["max_keypoints"] = -1
    assert m({"image": img})["keypoints"].shape[1] == n
    with pytest.raises(ValueError):
        m({"image": img[:, :2]})
