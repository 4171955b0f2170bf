"""DarkFeat on the MI355X (imcui/hloc/extractors/darkfeat.py around the restated network, tests/darkfeat_reference.py) in both
arithmetic modes, synthetic weights seed 0, uniform-random images of 32x48, 50x70 (odd behind both stride-2 layers) and 96x128:

  crafted     score maps through imcui_hip_darkfeat_detect_probe, exact: a peak either side of the border band's edge; a ridge that
              fails the edge ratio and a blob that passes it, the ratio just either side of 121 / 10; det <= 0; a plateau (every pixel a
              candidate: the list holds H W entries); all below the threshold; a score equal to the threshold; nms_size 0; a cut
              through equal scores; k = 1
  rule        the restated detector and cut on the device's OWN score map reproduce count, order, key-points and scores bit for bit at
              the default conf, at a threshold midway between the two middle candidate scores, at max_keypoints 7 and above the count
  end to end  score and descriptor maps within max(1e-4, 3 x the restatement's float32-vs-float64 spread) of the map's largest
              magnitude; the only key-points that may differ from the float32 restatement's are those whose score lies within the score
              bar of the threshold or of the k-th score (listed; at most 2 % -- tests/test_darkfeat_cpu.py checks on the CPU that the
              float32 restatement against its float64 self stays inside that cap with seed 0); descriptors at the common key-points
              within the map bar, norms 1 within 1e-5; the golden fixture of the reference's wrapper through the plugin's `_forward`
  determinism rows past the count are zero; an image alone against inside a batch of 3 and a HIP-graph replay are bitwise equal; a
              flat image gives zero key-points and status bit 4 and leaves its batch neighbours alone

Measured on one MI355X, both arithmetic modes: score map within 1.6e-06 .. 3.6e-06 and descriptor map within 1.7e-06 .. 2.3e-06 of the
restatement (bars 1e-4; the restatement's own float32-vs-float64 spreads are 1.5e-06 .. 2.4e-06 and 1.0e-06 .. 1.2e-06); the rule on the
device's own score map bit for bit at every setting; end to end no key-point differs from the restatement's (7 / 17 / 90 at the default
conf; 4 / 14 / 78 at the midway threshold), descriptors at the common key-points within 2.1e-06, norms 1 within 9.0e-08; the golden
fixture: the same key-points in the same order, scores within 7.0e-06 (bars 3.7e-04 / 2.1e-04), descriptors within 2.2e-06.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import darkfeat_reference as R
from test_darkfeat_cpu import CRAFT_H, CRAFT_W, GOLDEN, SIZES, check_crafted, crafted_cases, image, median_threshold, net, parts, relmax, state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KEYS = ("keypoints", "scores", "descriptors", "num_keypoints")


@functools.lru_cache(maxsize=None)
def _plugin():
    from imcui_hip.hloc.extractors.darkfeat import DarkFeat

    return DarkFeat({"state_dict": state()}).eval().to(DEV)


def _run(img, thr, k, want_maps=False):
    m = _plugin()
    m.conf.update(score_thld=thr, max_keypoints=k)
    out = m.forward_batched(img.to(DEV), want_maps=want_maps)
    torch.cuda.synchronize()
    m.conf.pop("score_thld")
    return {key: v.cpu() for key, v in out.items()}


def _bars(hw):
    o32, o64 = parts(*hw), parts(*hw, double=True)
    spread = {k: relmax(o32[k], o64[k]) for k in ("score", "desc_map")}
    return {k: max(1e-4, 3 * v) for k, v in spread.items()}, spread


def _settings(hw):
    return ((0.5, 1000), (median_threshold(hw), 0), (0.5, 7), (0.5, 100000))


# ------------------------------------------------------------------ crafted score maps
def _detect(score, **conf):
    from imcui_hip import backend

    out = backend.DarkFeatHIP().detect_probe(score.to(DEV), conf)
    torch.cuda.synchronize()
    return {key: v.cpu() for key, v in out.items()}


def test_crafted_score_maps():
    """Every crafted case of tests/test_darkfeat_cpu.py (whose expectations the CPU suite checks on the restated detector): the device
    reproduces the restated detector and cut bit for bit -- count, order, key-points, scores -- and the expectation itself."""
    H, W = CRAFT_H, CRAFT_W
    walk = []
    for name, s, conf, expect in crafted_cases():
        out = _detect(s[None], **conf)
        det = dict(R.DET, **{k: v for k, v in conf.items() if k != "max_keypoints"})
        k = conf.get("max_keypoints", 0)
        pix, kp, sc = R.select(s, det, k)
        n = int(out["num_keypoints"][0])
        kout = out["keypoints"].shape[1]
        assert kout == max(1, min(H * W, det["kpt_n"], k or H * W)) and int(out["status"][0]) == 0, name
        assert n == len(pix) and torch.equal(out["keypoints"][0, :n], kp) and torch.equal(out["scores"][0, :n], sc), name
        assert not out["keypoints"][0, n:].any() and not out["scores"][0, n:].any(), name
        got = (out["keypoints"][0, :n, 1] * W + out["keypoints"][0, :n, 0]).long()
        check_crafted(name, got, expect)
        cand = torch.nonzero(R.detect_mask(s, det).flatten()).flatten()
        assert int(out["num_candidates"][0]) == len(cand) and torch.equal(torch.nonzero(out["det_map"][0].flatten() > -float("inf")).flatten(), cand), name
        if expect.get("walk"):
            walk.append(n)
    assert walk[0] == 1 and walk[-1] == 0, walk
    # B = 2: two different maps in one call
    (_, s0, c0, _), (_, s1, _, _) = [c for c in crafted_cases() if c[0] in ("nms_size 3", "equal scores, all")]
    out = _detect(torch.stack([s0, s1]), **c0)
    for b, s in enumerate((s0, s1)):
        pix, kp, sc = R.select(s, dict(R.DET, **c0), 0)
        n = int(out["num_keypoints"][b])
        assert n == len(pix) and torch.equal(out["keypoints"][b, :n], kp) and torch.equal(out["scores"][b, :n], sc)
    # refusals by value
    with pytest.raises(ValueError, match="negative"):
        _detect(s0[None], max_keypoints=-1)
    with pytest.raises(ValueError, match="nms_size"):
        _detect(s0[None], nms_size=5)


# ------------------------------------------------------------------ maps, the rule on the device's own score map, end to end
@pytest.mark.parametrize("hw", SIZES)
def test_rule_bitwise_and_end_to_end(hw, precision):
    H, W = hw
    bars, spread = _bars(hw)
    o32 = parts(*hw)
    s32 = o32["score"][0]
    top = float(s32.abs().max())
    for thr, k in _settings(hw):
        out = _run(image(*hw), thr, k, want_maps=True)
        n = int(out["num_keypoints"][0])
        errs = {"score": relmax(out["score"], o32["score"]), "desc_map": relmax(out["desc_map"].permute(0, 3, 1, 2), o32["desc_map"])}
        assert errs["score"] <= bars["score"] and errs["desc_map"] <= bars["desc_map"], errs
        assert int(out["status"][0]) == 0 and out["keypoints"].shape[1] == min(H * W, 5000, k or H * W)
        # ---- bit for bit against the restated detector and cut on the device's own score map
        det = dict(R.DET, score_thld=thr)
        pix, kp, sc = R.select(out["score"][0], det, k)
        assert n == len(pix) and n > 0
        assert torch.equal(out["keypoints"][0, :n], kp) and torch.equal(out["scores"][0, :n], sc)
        assert not out["keypoints"][0, n:].any() and not out["scores"][0, n:].any() and not out["descriptors"][0, n:].any(), "rows past the count are zero"
        # ---- end to end against the float32 restatement
        rpix, rkp, rsc = R.select(s32, det, k)
        differ = sorted(set(pix.tolist()) ^ set(rpix.tolist()))
        kth = float(rsc[0]) if (k and len(rsc) == k) else None  # the lowest kept score when the cut was taken
        for p in differ:
            s = float(s32.flatten()[p])
            near = abs(s - thr) <= bars["score"] * top or (kth is not None and abs(s - kth) <= bars["score"] * top)
            assert near, f"pixel {p} (score {s}) differs away from the threshold {thr} / the k-th score {kth}"
        print(f"{hw} precision {precision} threshold {thr:.4f} k {k}: {n} key-points, differing pixels {differ}; score map {errs['score']:.2e} (bar "
              f"{bars['score']:.2e}), descriptor map {errs['desc_map']:.2e} (bar {bars['desc_map']:.2e}); restatement spreads {spread}")  # fmt: skip
        assert len(differ) <= 0.02 * max(len(rpix), 1)
        common = [p for p in pix.tolist() if p in set(rpix.tolist())]
        rows = torch.tensor([pix.tolist().index(p) for p in common])
        rrows = torch.tensor([rpix.tolist().index(p) for p in common])
        d = out["descriptors"][0, :n][rows]
        rdesc = R.describe(o32["desc_map"][0], rkp)[rrows]
        derr = relmax(d, rdesc)
        norm = (d.double().norm(dim=1) - 1).abs().max().item()
        print(f"    descriptors at {len(common)} common key-points {derr:.2e} (bar {bars['desc_map']:.2e}), |norm - 1| {norm:.1e}")
        assert derr <= bars["desc_map"] and norm < 1e-5


@pytest.mark.parametrize("tag", ["40x56", "50x70"])
def test_golden_of_the_reference_wrapper_through_the_plugin(tag, precision):
    """tests/golden/darkfeat_golden.npz (the reference's own darkfeat.py around the restated network) through `_forward`: the same
    counts and order, scores and descriptors within the bars."""
    g = np.load(GOLDEN)
    img = torch.from_numpy(g[f"image_u8_{tag}"]).float() / 255.0
    m = _plugin()
    full = torch.from_numpy(g[f"descriptors_all_{tag}"])
    with torch.no_grad():
        o32, o64 = net().parts(img), net(double=True).parts(img.double())
    top = float(o64["score"].abs().max())
    sbar = max(1e-4, 3 * relmax(o32["score"], o64["score"])) * top
    dbar = max(1e-4, 3 * relmax(o32["desc_map"], o64["desc_map"]))
    for name, k in (("all", 0), ("top7", 7), ("above", 1000)):
        m.conf.update(max_keypoints=k)
        with torch.no_grad():
            pred = {key: v.cpu() for key, v in m({"image": img.to(DEV)}).items()}
        want_kp, want_sc = torch.from_numpy(g[f"keypoints_{name}_{tag}"]), torch.from_numpy(g[f"scores_{name}_{tag}"])
        want_de = full if name == "all" else full[torch.from_numpy(g[f"desc_rows_{name}_{tag}"])]
        n = len(want_sc)
        assert pred["keypoints"].shape == (1, n, 2) and pred["scores"].shape == (1, n) and pred["descriptors"].shape == (1, 128, n), (name, pred["scores"].shape)
        errs = ((pred["scores"][0] - want_sc).abs().max().item(), relmax(pred["descriptors"][0].t(), want_de))
        print(f"{tag} {name} precision {precision}: {n} key-points, scores {errs[0]:.2e} (bar {sbar:.2e}), descriptors {errs[1]:.2e} (bar {dbar:.2e})")
        assert torch.equal(pred["keypoints"][0], want_kp), "the same key-points in the same order"
        assert errs[0] <= sbar and errs[1] <= dbar


# ------------------------------------------------------------------ determinism, the flat image
def test_batch_independence_and_graph_replay_are_bitwise(precision):
    from imcui_hip import backend

    m = _plugin()
    m.conf.update(max_keypoints=12)
    a, b, c = (image(50, 70, s).to(DEV) for s in (0, 1, 2))
    solo = m.forward_batched(a)
    trio = m.forward_batched(torch.cat([b, a, c]))
    assert int(solo["num_keypoints"][0]) > 5
    for k in KEYS:
        assert torch.equal(solo[k][0], trio[k][1]), k
    batch = torch.cat([a, b])
    eager = m.forward_batched(batch)
    table = {}
    with backend.workspace_owner(table):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.forward_batched(batch)  # warm-up: allocates the graph-owned workspace
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = m.forward_batched(batch)
    for _ in range(2):
        for v in cap.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(eager[k], cap[k]), k


def test_flat_image_gives_zero_keypoints_and_the_status_bit(precision):
    from imcui_hip import backend

    m = _plugin()
    m.conf.update(max_keypoints=1000)
    a = image(50, 70, 0).to(DEV)
    flat = torch.full_like(a, 0.375)
    solo = m.forward_batched(a)
    out = m.forward_batched(torch.cat([flat, a]))
    torch.cuda.synchronize()
    assert int(out["status"][0]) == backend.DARKFEAT_STATUS_FLAT and int(solo["status"][0]) == 0
    assert int(out["num_keypoints"][0]) == 0 and not out["keypoints"][0].any() and not out["scores"][0].any() and not out["descriptors"][0].any()
    for k in KEYS:
        assert torch.equal(out[k][1], solo[k][0]), k  # the neighbour of a flat image is untouched
    pred = m({"image": flat})  # through `_forward`: a result, not an error
    assert pred["keypoints"].shape == (1, 0, 2) and pred["scores"].shape == (1, 0) and pred["descriptors"].shape == (1, 128, 0)
    with pytest.raises(ValueError, match="RGB"):
        m.forward_batched(a[:, :1])
    with pytest.raises(ValueError, match="at least 16"):
        m.forward_batched(a[:, :, :15])
