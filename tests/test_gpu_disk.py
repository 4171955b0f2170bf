"""DISK on the MI355X (imcui/hloc/extractors/disk.py:18-36 -> kornia DISK) against the CPU restatement (tests/disk_reference.py),
in both arithmetic modes: the dense heatmap, the selection rule on the HIP heatmap (bit-exact), the end-to-end key-point sets (equal,
or every difference an audited round-off tie), descriptors / scores at common key-points, batch independence, graph replay and the
plugin's output contract."""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

from disk_reference import DISKReference, descriptors_at, heatmap_to_keypoints
from parity_utils import oracle_spread

pytestmark = pytest.mark.gpu

SIZES = {"480x640": (480, 640, 0), "472x632": (472, 632, 1), "1200x1600": (1200, 1600, 2)}
CONFS = {
    "all-w5": dict(max_keypoints=None, nms_window_size=5, detection_threshold=0.0),
    "n5000-w5": dict(max_keypoints=5000, nms_window_size=5, detection_threshold=0.0),
    "n300-w3-thr": dict(max_keypoints=300, nms_window_size=3, detection_threshold=0.5),
}
CASES = [("480x640", c) for c in CONFS] + [("472x632", "n300-w3-thr"), ("472x632", "all-w5"), ("1200x1600", "n5000-w5")]


def _image(h, w, seed):
    """Seeded RGB in [0, 1]: smooth structure at several scales + a little pixel noise."""
    g = torch.Generator().manual_seed(seed)
    img = torch.zeros(1, 3, h, w)
    for s, a in ((8, 0.5), (32, 0.3), (128, 0.2)):
        low = torch.rand(1, 3, max(2, h // s), max(2, w // s), generator=g)
        img += a * F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)
    return (img + 0.02 * torch.rand(1, 3, h, w, generator=g)).clamp(0, 1)


@functools.lru_cache(maxsize=None)
def _sd():
    from imcui_hip.synth_weights import disk_state_dict

    return disk_state_dict(0)


@functools.lru_cache(maxsize=None)
def _oracle(size: str):
    """(image, reference heatmap [h,w], reference dense descriptors [128,h,w], fp32 spread of the heatmap)."""
    h, w, seed = SIZES[size]
    img = _image(h, w, seed)
    ref = DISKReference(_sd())
    if h * w <= 480 * 640:
        spread, (heat, desc) = oracle_spread(lambda: ref.heatmap_and_dense_descriptors(img), threads=(1, 8))
    else:  # one evaluation at this size; the spread of the 480 x 640 case stands in
        heat, desc = ref.heatmap_and_dense_descriptors(img)
        spread = _oracle("480x640")[3]
    return img, heat[0, 0], desc[0], spread


def _bar(size):
    return max(1e-4, 3 * _oracle(size)[3])


def _model(conf):
    from imcui_hip.hloc.extractors.disk import DISK

    return DISK({**conf, "state_dict": _sd()}).eval().to("cuda:0")


def _hip(model, img, want_heatmap=True):
    out = model.forward_batched(img.cuda(), want_heatmap=want_heatmap)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _rule(heat, conf):
    (xy, lp), = heatmap_to_keypoints(heat[None, None], n=conf["max_keypoints"], window_size=conf["nms_window_size"],
                                     score_threshold=conf["detection_threshold"])  # fmt: skip
    return xy, lp


def _cutoff(heat, conf):
    """The (n + 1)-th largest NMS survivor (None without n)."""
    if conf["max_keypoints"] is None:
        return None
    (xy, lp), = heatmap_to_keypoints(heat[None, None], n=None, window_size=conf["nms_window_size"], score_threshold=conf["detection_threshold"])
    if lp.numel() == 0:
        return None
    return torch.sort(lp, descending=True).values[min(conf["max_keypoints"], lp.numel() - 1)].item()


def audit_disk_differences(xy_h, xy_r, heat_h, heat_r, conf, tag=""):
    """Every key-point in one set but not the other must be a round-off tie: the margin that decides it -- against the threshold,
    against a pixel of its NMS window, or against the selection cut-off of either heatmap -- below twice the measured heatmap
    difference.  Returns the number of audited differences."""
    H, W = heat_r.shape
    diff = (heat_h - heat_r).abs().max().item()
    sh = {(int(x), int(y)) for x, y in xy_h.tolist()}
    sr = {(int(x), int(y)) for x, y in xy_r.tolist()}
    cuts = [c for c in (_cutoff(heat_r, conf), _cutoff(heat_h, conf)) if c is not None]
    r = conf["nms_window_size"] // 2
    for x, y in sorted(sh ^ sr):
        v = heat_r[y, x].item()
        margins = [abs(v - conf["detection_threshold"])] + [abs(v - c) for c in cuts]
        y0, x0 = max(0, y - r), max(0, x - r)
        win = heat_r[y0 : y + r + 1, x0 : x + r + 1].clone()
        win[y - y0, x - x0] = float("inf")  # the pixel itself; an exactly equal neighbour is a tie (margin 0)
        margins.append((win - v).abs().min().item())
        if not min(margins) < 2 * diff:
            raise AssertionError(f"{tag}: key-point ({x}, {y}) differs with margin {min(margins):.3e} >= 2 x heatmap difference {diff:.3e}")
    assert len(sh ^ sr) <= max(2, 0.01 * len(sr)), (tag, len(sh ^ sr), len(sr))
    return len(sh ^ sr)


@pytest.mark.parametrize("size,cname", CASES, ids=[f"{s}-{c}" for s, c in CASES])
def test_disk_vs_restatement(precision, size, cname):
    conf = CONFS[cname]
    img, heat_r, desc_r, _ = _oracle(size)
    out = _hip(_model(conf), img)
    bar = _bar(size)
    heat_h = out["heatmap"][0]
    # (1) dense heatmap
    err = (heat_h - heat_r).abs().max().item() / heat_r.abs().max().item()
    assert err <= bar, (size, cname, err, bar)
    n = int(out["num_keypoints"][0])
    assert int(out["status"][0]) == 0
    xy_h, sc_h, de_h = out["keypoints"][0, :n], out["scores"][0, :n], out["descriptors"][0, :n]
    # (2) the restated selection on the HIP heatmap: bit-exact, row-major
    xy_rule, lp_rule = _rule(heat_h, conf)
    assert torch.equal(xy_h, xy_rule.float()) and torch.equal(sc_h, lp_rule), (size, cname, n, len(xy_rule))
    assert torch.all(out["keypoints"][0, n:] == 0) and torch.all(out["descriptors"][0, n:] == 0)
    # (3) end to end: the reference's key-points, or audited ties
    xy_r, lp_r = _rule(heat_r, conf)
    ties = audit_disk_differences(xy_h, xy_r, heat_h, heat_r, conf, tag=f"{size}/{cname}")
    assert n > 50, n
    # descriptors and scores at the common key-points
    xy_hl, xy_rl = xy_h.long(), xy_r.long()
    flat_h = xy_hl[:, 1] * 10**5 + xy_hl[:, 0]
    flat_r = xy_rl[:, 1] * 10**5 + xy_rl[:, 0]
    common_h = torch.isin(flat_h, flat_r)
    common_r = torch.isin(flat_r, flat_h)
    assert torch.equal(flat_h[common_h], flat_r[common_r])  # both row-major
    d_ref = descriptors_at(desc_r, xy_r[common_r])
    derr = (de_h[common_h] - d_ref).abs().max().item()
    serr = (sc_h[common_h] - lp_r[common_r]).abs().max().item() / heat_r.abs().max().item()
    assert derr <= bar and serr <= bar, (derr, serr, bar)
    norms = de_h.norm(dim=1)
    assert torch.allclose(norms, torch.ones_like(norms), atol=1e-5)
    print(f"[disk] {size} {cname} precision={precision}: n={n} heat err {err:.2e} (bar {bar:.1e}) desc err {derr:.2e} ties {ties}")


def test_disk_batch_independence(precision):
    conf = CONFS["n300-w3-thr"]
    m = _model(conf)
    img = _oracle("472x632")[0]
    others = [_image(472, 632, s) for s in (11, 12, 13)]
    one = _hip(m, img)
    four = _hip(m, torch.cat([others[0], img, others[1], others[2]]))
    for k in ("keypoints", "scores", "descriptors", "heatmap", "num_keypoints"):
        assert torch.equal(one[k][0], four[k][1]), k


def test_disk_graph_replay_bitwise(precision):
    from imcui_hip.pipeline import GraphedCall

    conf = CONFS["n5000-w5"]
    m = _model(conf)
    img = _oracle("480x640")[0].cuda()
    eager = _hip(m, img)
    g = GraphedCall(lambda x: m.forward_batched(x, want_heatmap=True), img)
    img2 = _image(480, 640, 21).cuda()
    rep2 = {k: v.cpu() for k, v in g(img2).items()}
    rep = {k: v.cpu() for k, v in g(img).items()}
    eager2 = _hip(m, img2)
    for k in eager:
        assert torch.equal(rep[k], eager[k]), k
        assert torch.equal(rep2[k], eager2[k]), k


def test_disk_plugin_output_contract():
    conf = CONFS["n300-w3-thr"]
    m = _model(conf)
    img = _oracle("472x632")[0].cuda()
    out = m({"image": img})
    n = out["keypoints"].shape[1]
    assert out["keypoints"].shape == (1, n, 2) and out["scores"].shape == (1, n) and out["descriptors"].shape == (1, 128, n)
    assert all(v.dtype == torch.float32 and v.is_contiguous() and torch.is_tensor(v) for v in out.values())
    kp = out["keypoints"][0].cpu()
    assert 0 < n <= 300 and torch.equal(kp, kp.round())
    flat = kp[:, 1] * img.shape[-1] + kp[:, 0]
    assert torch.all(flat[1:] > flat[:-1])  # row-major, not by score
    # the conf is re-read on every call (the UI mutates max_keypoints)
    m.conf["max_keypoints"] = 50
    assert m({"image": img})["keypoints"].shape[1] <= 50
    m.conf["max_keypoints"] = None
    assert m({"image": img})["keypoints"].shape[1] >= n
    with pytest.raises(ValueError):
        m({"image": img[:, :1]})


@pytest.mark.parametrize("window", [1, 3, 5])
def test_disk_device_tie_rules_on_a_flat_heatmap(precision, window):
    """The device's tie rules, driven on purpose: the heatmap row of the last convolution has zero weights and bias 1, so every pixel
    ties with every pixel of its window.  NMS (first maximum in row-major order wins): window 1 keeps every pixel, a wider window keeps
    only (0, 0) -- every other pixel has an equal, earlier pixel in its window.  The strict threshold (1.0) drops everything; with
    `max_keypoints` set every candidate equals the (n + 1)-th value and is dropped (fewer than n + 1 candidates: the minimum goes).
    Each case also equals the restated rule on the same heatmap."""
    from imcui_hip.hloc.extractors.disk import DISK

    sd = {k: v.clone() for k, v in _sd().items()}
    sd["unet.path_up.3.conv.3.weight"][128] = 0.0
    sd["unet.path_up.3.conv.3.bias"][128] = 1.0
    H, W = 72, 88
    img = _image(H, W, 5)
    flat = torch.ones(H, W)
    for maxk, thr in ((None, 0.0), (None, 1.0), (10, 0.0), (H * W, 0.0)):
        conf = dict(max_keypoints=maxk, nms_window_size=window, detection_threshold=thr)
        out = _hip(DISK({**conf, "state_dict": sd}).eval().to("cuda:0"), img)
        assert torch.equal(out["heatmap"][0], flat)
        n = int(out["num_keypoints"][0])
        xy_rule, lp_rule = _rule(flat, conf) if maxk is None or thr < 1.0 else (torch.zeros(0, 2), torch.zeros(0))
        assert torch.equal(out["keypoints"][0, :n], xy_rule.float()) and torch.equal(out["scores"][0, :n], lp_rule)
        if maxk is not None or thr >= 1.0:
            assert n == 0, (window, maxk, thr, n)
        elif window == 1:
            assert n == H * W
        else:
            assert n == 1 and out["keypoints"][0, 0].tolist() == [0.0, 0.0]
        assert int(out["status"][0]) == 0
        if n:
            assert torch.allclose(out["descriptors"][0, :n].norm(dim=1), torch.ones(n), atol=1e-5)
