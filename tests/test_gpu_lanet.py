"""LANet on the MI355X (imcui/hloc/extractors/lanet.py around the restated PointModel, tests/lanet_reference.py) in both arithmetic
modes, synthetic weights seed 0, uniform-random images of 32x48, 50x70 (odd at every pool) and 96x128:

  maps        per-cell score, coordinates, level weights and x4 against the float32 CPU restatement, maps relative to their largest
              magnitude: bar max(1e-4, 3 x the restatement's float32-vs-float64 spread); positions in pixels: 3 x the restatement's
              own float32-vs-float64 position difference on the same input (printed)
  rule        the restated wrapper rule on the device's OWN per-cell scores and coordinates reproduces count, order, key-points and
              scores bit for bit at threshold 0.1 / k = 0, the median score / k = 0 (midway between the two middle scores, so that
              no cell sits on the threshold), k = 7 and k above the count
  end to end  against the restatement: the only key-points that may differ are those whose score lies within the score bar of the
              threshold or of the k-th score (listed; at most 2 % of the cells -- tests/test_lanet_cpu.py checks on the CPU that the
              float32 restatement against its float64 self stays inside that cap with seed 0); descriptors at the common key-points
              within the map bar, norms 1 within 1e-5; the golden fixture of the reference's wrapper through the plugin's `_forward`
  crafted     through imcui_hip_lanet_select_probe: equal scores, all below the threshold, a score equal to the threshold, Hc = 2, k = 1
  determinism rows past the count are zero; an image alone against inside a batch of 3 and a HIP-graph replay are bitwise equal

Measured on one MI355X, both arithmetic modes: score within 4.3e-06, level weights 1.7e-06, x4 1.7e-06 of the restatement (bars 1e-4; the
restatement's own float32-vs-float64 spreads are 9.3e-07 .. 1.5e-06, 4.4e-07 .. 8.5e-07, 5.8e-07 .. 8.3e-07); positions 2.1e-05 / 3.1e-05 /
2.3e-05 px split and 1.7e-05 / 2.3e-05 / 2.3e-05 px exact at 32x48 / 50x70 / 96x128 (bars 2.4e-05 / 4.4e-05 / 3.0e-05 px); the rule on the
device's own cells bit for bit at every setting; end to end no key-point differs from the restatement's (8 / 23 / 136 at threshold 0.1),
descriptors within 2.4e-06; the golden fixture: positions within 1.9e-05 px (bars 3.6e-05 / 4.8e-05), scores 2.8e-06, descriptors 2.2e-06.
"""
from __future__ import annotations

import functools
import math
import os

import numpy as np
import pytest
import torch

import lanet_reference as R
from test_lanet_cpu import GOLDEN, SIZES, cells_of, image, net, parts, state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KEYS = ("keypoints", "scores", "descriptors", "num_keypoints")


@functools.lru_cache(maxsize=None)
def _plugin():
    from imcui_hip.hloc.extractors.lanet import LANet

    return LANet({"state_dict": state()}).eval().to(DEV)


def _run(img, thr, k, want_maps=False):
    m = _plugin()
    m.conf.update(keypoint_threshold=thr, max_keypoints=k)
    out = m.forward_batched(img.to(DEV), want_maps=want_maps)
    torch.cuda.synchronize()
    return {key: v.cpu() for key, v in out.items()}


def relmax(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


def _bars(hw):
    """(score bar, map bar of x4, aware bar, position bar in pixels) from the restatement's own float32-vs-float64 spread."""
    o32, o64 = parts(*hw), parts(*hw, double=True)
    spread = {k: relmax(o32[k], o64[k]) for k in ("score", "aware", "x4", "desc")}
    pos = (o32["coord"].double() - o64["coord"]).abs().max().item()
    return {k: max(1e-4, 3 * v) for k, v in spread.items()}, 3 * pos, spread, pos


def _settings(hw):
    s64 = cells_of(parts(*hw, double=True))[0]
    return ((0.1, 0), (R.median_threshold(s64), 0), (0.1, 7), (0.1, 100000))


# ------------------------------------------------------------------ maps
@pytest.mark.parametrize("hw", SIZES)
def test_cell_maps_against_the_restatement(hw, precision):
    H, W = hw
    out = _run(image(*hw), 0.1, 0, want_maps=True)
    o32 = parts(*hw)
    bars, pos_bar, spread, pos_spread = _bars(hw)
    score, coord, _, aware = cells_of(o32)
    errs = {"score": relmax(out["cell_score"][0], score), "aware": relmax(out["cell_aware"][0], aware),
            "x4": relmax(out["x4"][0].permute(2, 0, 1), o32["x4"][0])}  # fmt: skip
    pos = (out["cell_coord"][0].double() - coord.double()).abs().max().item()
    print(f"{hw} precision {precision}: score {errs['score']:.2e} (bar {bars['score']:.2e}), level weights {errs['aware']:.2e} (bar {bars['aware']:.2e}), "
          f"x4 {errs['x4']:.2e} (bar {bars['x4']:.2e}); positions {pos:.2e} px (bar {pos_bar:.2e} px = 3 x the restatement's own float32-vs-float64 "
          f"difference {pos_spread:.2e} px); restatement spreads {spread}")  # fmt: skip
    for k, e in errs.items():
        assert e <= bars[k], k
    assert pos <= pos_bar
    # the decode on the device's own tanh values, bit for bit, on real maps too
    Hc, Wc = H // 8, W // 8
    t = out["cell_tanh"][0].view(Hc, Wc, 2).permute(2, 0, 1)[None].contiguous()
    assert torch.equal(out["cell_coord"][0], R.coord_from_tanh(t, H, W)[0].flatten(1).t())


# ------------------------------------------------------------------ the rule on the device's own cells, and end to end
@pytest.mark.parametrize("hw", SIZES)
def test_rule_bitwise_and_end_to_end(hw, precision):
    H, W = hw
    np_ = (H // 8) * (W // 8)
    bars, _, _, _ = _bars(hw)
    score32, coord32, desc32, _ = cells_of(parts(*hw))
    for thr, k in _settings(hw):
        out = _run(image(*hw), thr, k, want_maps=True)
        n = int(out["num_keypoints"][0])
        kout = out["keypoints"].shape[1]
        assert kout == (np_ if k == 0 else min(k, np_)) and int(out["status"][0]) == 0
        # ---- bit for bit against the restated rule on the device's own per-cell values
        cells, kp, sc, _ = R.wrapper_rule(out["cell_score"][0], out["cell_coord"][0], None, thr, k)
        assert n == len(cells) and n > 0
        assert torch.equal(out["keypoints"][0, :n], kp) and torch.equal(out["scores"][0, :n], sc)
        assert not out["keypoints"][0, n:].any() and not out["scores"][0, n:].any() and not out["descriptors"][0, n:].any(), "rows past the count are zero"
        # ---- end to end against the float32 restatement
        rcells, _, rsc, rdesc = R.wrapper_rule(score32, coord32, desc32, thr, k)
        differ = sorted(set(cells.tolist()) ^ set(rcells.tolist()))
        kth = float(rsc[0]) if (k and len(rsc) == k) else None  # the lowest kept score when the cut was taken
        for c in differ:
            s = float(score32[c])
            near = abs(s - thr) <= bars["score"] or (kth is not None and abs(s - kth) <= bars["score"])
            assert near, f"cell {c} (score {s}) differs away from the threshold {thr} / the k-th score {kth}"
        print(f"{hw} precision {precision} threshold {thr:.4f} k {k}: {n} key-points, differing cells {differ}")
        assert len(differ) <= 0.02 * np_
        common = [c for c in cells.tolist() if c in set(rcells.tolist())]
        rows = torch.tensor([cells.tolist().index(c) for c in common])
        rrows = torch.tensor([rcells.tolist().index(c) for c in common])
        d = out["descriptors"][0, :n][rows]
        derr = relmax(d, rdesc[rrows])
        norm = (d.double().norm(dim=1) - 1).abs().max().item()
        print(f"    descriptors at {len(common)} common key-points {derr:.2e} (bar {bars['desc']:.2e}), |norm - 1| {norm:.1e}")
        assert derr <= bars["desc"] and norm < 1e-5


@pytest.mark.parametrize("tag", ["40x56", "50x70"])
def test_golden_of_the_reference_wrapper_through_the_plugin(tag, precision):
    """tests/golden/lanet_golden.npz (the reference's own lanet.py around the restated network) through `_forward`: the same count and
    order unless a score lies within the score bar of the threshold or the k-th score; positions, scores and descriptors within the bars."""
    g = np.load(GOLDEN)
    img = (torch.from_numpy(g[f"image_u8_{tag}"]).float() / 255.0)
    m = _plugin()
    full = torch.from_numpy(g[f"descriptors_all_{tag}"])
    with torch.no_grad():
        o32, o64 = net().parts(img), net(double=True).parts(img.double())
    sbar = max(1e-4, 3 * relmax(o32["score"], o64["score"]))
    dbar = max(1e-4, 3 * relmax(o32["desc"], o64["desc"]))
    pbar = 3 * (o32["coord"].double() - o64["coord"]).abs().max().item()
    for name, thr, k in (("all", 0.1, 0), ("median", float(g[f"median_{tag}"]), 0), ("top7", 0.1, 7)):
        m.conf.update(keypoint_threshold=thr, max_keypoints=k)
        with torch.no_grad():
            pred = {key: v.cpu() for key, v in m({"image": img.to(DEV)}).items()}
        want_kp, want_sc = torch.from_numpy(g[f"keypoints_{name}_{tag}"]), torch.from_numpy(g[f"scores_{name}_{tag}"])
        want_de = full if name == "all" else full[torch.from_numpy(g[f"desc_rows_{name}_{tag}"])]
        n = len(want_sc)
        assert pred["keypoints"].shape == (1, n, 2) and pred["scores"].shape == (1, n) and pred["descriptors"].shape == (1, 256, n), (name, pred["scores"].shape)
        errs = ((pred["keypoints"][0] - want_kp).abs().max().item(), (pred["scores"][0] - want_sc).abs().max().item(),
                relmax(pred["descriptors"][0].t(), want_de))  # fmt: skip
        print(f"{tag} {name} precision {precision}: {n} key-points, positions {errs[0]:.2e} px (bar {pbar:.2e}), scores {errs[1]:.2e} (bar {sbar:.2e}), "
              f"descriptors {errs[2]:.2e} (bar {dbar:.2e})")  # fmt: skip
        assert errs[0] <= pbar and errs[1] <= sbar and errs[2] <= dbar


# ------------------------------------------------------------------ crafted head outputs
def _logit(p):
    return math.log(p / (1 - p))


def _select(raw, H, W, thr, k):
    from imcui_hip import backend

    impl = backend.LanetHIP({"widths": R.WIDTHS, "k": (3, 3), "bias": (1, 1), "bn": (0, 0), "activation": "relu", "conv_bias": 0})
    out = impl.select_probe(raw.to(DEV), H, W, thr, k)
    torch.cuda.synchronize()
    return {key: v.cpu() for key, v in out.items()}


def test_crafted_selection_cases():
    H, W, Hc, Wc = 40, 56, 5, 7
    interior = [cy * Wc + cx for cy in range(1, Hc - 1) for cx in range(1, Wc - 1)]  # 15 cells
    raw = torch.zeros(1, Hc, Wc, 6)
    # ---- all scores equal (sigmoid(0) = 0.5): the stable order is ascending (score, cell index), the output is its tail, so the cut keeps
    # the HIGHEST cell indices and returns them in ascending cell order
    out = _select(raw, H, W, 0.1, 0)
    assert int(out["num_keypoints"][0]) == 15 and bool((out["scores"][0, :15] == 0.5).all()) and not out["scores"][0, 15:].any()
    base = torch.tensor([[(c % Wc) * 8 + 3.5, (c // Wc) * 8 + 3.5] for c in interior])  # tanh(0) = 0: the cell centres
    assert torch.equal(out["keypoints"][0, :15], base)
    out = _select(raw, H, W, 0.1, 4)
    assert int(out["num_keypoints"][0]) == 4 and torch.equal(out["keypoints"][0], base[-4:])
    assert torch.equal(out["cell_aware"][0], torch.full((Hc * Wc, 3), 1 / 3)) or (out["cell_aware"][0] - 1 / 3).abs().max() < 1e-7
    # ---- all below the threshold: zero key-points, zero rows
    out = _select(raw, H, W, 0.6, 0)
    assert int(out["num_keypoints"][0]) == 0 and not out["keypoints"].any() and not out["scores"].any() and int(out["status"][0]) == 0
    # ---- a score exactly equal to the threshold is dropped (strict >); the device's own score of that cell is the threshold
    raw2 = raw.clone()
    raw2[0, 2, 3, 3] = _logit(0.8)
    probe = _select(raw2, H, W, 0.1, 0)
    s_eq = float(probe["cell_score"][0, 2 * Wc + 3])
    out = _select(raw2, H, W, s_eq, 0)
    assert int(out["num_keypoints"][0]) == 0
    out = _select(raw2, H, W, float(np.nextafter(np.float32(s_eq), np.float32(0))), 0)
    assert int(out["num_keypoints"][0]) == 1 and out["keypoints"][0, 0].tolist() == [3 * 8 + 3.5, 2 * 8 + 3.5]
    # ---- k = 1: the single highest score; among equals the highest cell index
    out = _select(raw2, H, W, 0.1, 1)
    assert int(out["num_keypoints"][0]) == 1 and out["keypoints"].shape == (1, 1, 2) and float(out["scores"][0, 0]) == s_eq
    out = _select(raw, H, W, 0.1, 1)
    assert out["keypoints"][0, 0].tolist() == base[-1].tolist()
    # ---- Hc = 2: nothing survives the border; B = 2
    out = _select(torch.full((2, 2, 7, 6), 3.0), 16, 56, 0.1, 0)
    assert out["num_keypoints"].tolist() == [0, 0] and not out["cell_score"].any() and not out["keypoints"].any()
    # ---- a negative max_keypoints is refused by value
    with pytest.raises(ValueError, match="negative"):
        _select(raw, H, W, 0.1, -1)


# ------------------------------------------------------------------ determinism
def test_batch_independence_and_graph_replay_are_bitwise(precision):
    from imcui_hip import backend

    m = _plugin()
    m.conf.update(keypoint_threshold=0.1, max_keypoints=40)
    a, b, c = (image(50, 70, s).to(DEV) for s in (0, 1, 2))
    solo = m.forward_batched(a)
    trio = m.forward_batched(torch.cat([b, a, c]))
    assert int(solo["num_keypoints"][0]) > 10
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
