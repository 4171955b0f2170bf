"""SFD2 end to end on the GPU (csrc/sfd2.hip behind the `sfd2` plugin) against the restatement tests/sfd2_reference.py, at 32x48, 50x70
(odd behind both stride-2 layers; the score map, 52x72, is larger than the image) and 96x128, in both arithmetic modes.

  maps        score map and descriptor map within 1e-4 of the float32 CPU restatement, relative to the map's largest magnitude (the
              project's bar); the restatement's own float32-vs-float64 spread is printed beside it
  the rule    `R.select` on the device's OWN score map reproduces count, order, key-points and scores bit for bit at the default conf, at
              a threshold midway between the two middle candidate scores, at max_keypoints 7 and at a min_keypoints above the count
  end to end  against the restatement's own key-points a key-point may be left out only if its score is closer to the threshold than the
              measured score-map difference, or that close to a rival inside its NMS window; at most 2 % of the key-points (a condition;
              tests/test_sfd2_cpu.py checks that float32 against float64 stays within it for the seed).  Descriptors at the common
              key-points within the layers-file bar of the sampler plus the trunk's (the descriptor-map bar); norms 1
  golden      tests/golden/sfd2_golden.npz through the plugin's `_forward`: the same key-points in the same order, scores and
              descriptors within the map bars
  bitwise     rows past the count zero; an image alone against inside a batch of 3; a HIP-graph replay
  refusals    sides of 15 and C = 1, with a message

Measured on one MI355X (both modes): score map 2.4e-06 .. 4.0e-06, descriptor map 1.2e-06 .. 1.7e-06 (bars 1e-4; the restatement's own
float32-vs-float64 spread 9.5e-07 .. 1.1e-06 / 5.9e-07 .. 8.1e-07); no key-point differs (19 / 53 / 198 at the default conf); descriptors
within 1.5e-06, norms 1 within 8.0e-08; golden: scores within 2.3e-06 (bars 9.3e-05 / 9.0e-05), descriptors within 1.4e-06.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import sfd2_reference as R
from test_sfd2_cpu import CAP, GOLDEN, SIZES, compare_keypoints, image, median_threshold, net, parts, relmax, state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KEYS = ("keypoints", "scores", "descriptors", "num_keypoints")
ULP_HALF = 6e-8


@functools.lru_cache(maxsize=None)
def _plugin():
    from imcui_hip.hloc.extractors.sfd2 import SFD2

    return SFD2({"state_dict": state()}).eval().to(DEV)


def _run(img, conf, want_maps=False):
    m = _plugin()
    saved = dict(m.conf)
    m.conf.update(conf)
    try:
        out = m.forward_batched(img.to(DEV), want_maps=want_maps)
        torch.cuda.synchronize()
    finally:
        m.conf.clear()
        m.conf.update(saved)
    return {key: v.cpu() for key, v in out.items()}


def _bars(hw):
    o32, o64 = parts(*hw), parts(*hw, double=True)
    spread = {k: relmax(o32[k], o64[k]) for k in ("score", "desc_map")}
    return {k: 1e-4 for k in spread}, spread


def _settings(hw):
    return ({}, {"conf_th": median_threshold(hw), "min_keypoints": 0}, {"max_keypoints": 7}, {"min_keypoints": 100000, "conf_th": median_threshold(hw)})


@pytest.mark.parametrize("hw", SIZES)
def test_rule_bitwise_and_end_to_end(hw, precision):
    H, W = hw
    bars, spread = _bars(hw)
    o32 = parts(*hw)
    s32 = o32["score"][0]
    Hs, Ws = s32.shape
    assert (Hs, Ws) == (4 * R.down(R.down(H)), 4 * R.down(R.down(W)))
    nms32 = R.simple_nms(s32[None])[0]
    for conf in _settings(hw):
        out = _run(image(*hw), conf, want_maps=True)
        n = int(out["num_keypoints"][0])
        errs = {"score": relmax(out["score"], o32["score"]), "desc_map": relmax(out["desc_map"].permute(0, 3, 1, 2), o32["desc_map"])}
        assert errs["score"] <= bars["score"] and errs["desc_map"] <= bars["desc_map"], errs
        k = conf.get("max_keypoints", 4096)
        assert int(out["status"][0]) == 0 and out["keypoints"].shape[1] == min(Hs * Ws, k)
        # ---- bit for bit against the restated rule on the device's own score map
        pix, kp, sc, th = R.select(out["score"][0], hw, conf)
        assert n == len(pix) and n > 0
        assert torch.equal(out["keypoints"][0, :n], kp) and torch.equal(out["scores"][0, :n], sc)
        assert bool((kp[:, 0] <= W - 5).all() and (kp[:, 1] <= H - 5).all() and (kp >= 4).all()), "no key-point outside the image's band"
        assert not out["keypoints"][0, n:].any() and not out["scores"][0, n:].any() and not out["descriptors"][0, n:].any(), "rows past the count are zero"
        if "min_keypoints" in conf and conf["min_keypoints"] > n:
            assert th == 0.0, "the fallback fired"
        # ---- end to end against the float32 restatement
        rpix, rkp, rsc, rth = R.select(s32, hw, conf)
        diff = (out["score"][0].double() - s32.double()).abs().max().item()
        common, excused, unexplained = compare_keypoints(pix, sc, rpix, rsc, nms32, Ws, rth, diff)
        print(f"{hw} precision {precision} {conf or 'default'}: {n} key-points (threshold {th:g}), {excused} excused, {unexplained} unexplained; score map "
              f"{errs['score']:.2e}, descriptor map {errs['desc_map']:.2e} (bars 1e-4); restatement float32-vs-float64 spreads {spread}")  # fmt: skip
        assert unexplained == 0 and excused <= CAP * max(len(rpix), 1)
        rows = torch.tensor([pix.tolist().index(p) for p in common])
        rrows = torch.tensor([rpix.tolist().index(p) for p in common])
        d = out["descriptors"][0, :n][rows]
        r32 = R.sample_descriptors(rkp, o32["desc_map"])[0].t()
        r64 = R.sample_descriptors(rkp.double(), parts(*hw, double=True)["desc_map"])[0].t()
        dbar = 3 * max(relmax(r32, r64), ULP_HALF) + bars["desc_map"]  # the sampler's layer bar plus the trunk's
        derr = relmax(d, r32[rrows])
        norm = (d.double().norm(dim=1) - 1).abs().max().item()
        print(f"    descriptors at {len(common)} common key-points {derr:.2e} (bar {dbar:.2e}), |norm - 1| {norm:.1e}")
        assert derr <= dbar and norm <= 3e-7


@pytest.mark.parametrize("tag", ["40x56", "50x70"])
def test_golden_of_the_reference_wrapper_through_the_plugin(tag, precision):
    """tests/golden/sfd2_golden.npz (the reference's own sfd2.py around the restated network) through `_forward`: the same counts and
    order, scores and descriptors within the bars (1e-4 of the map's largest magnitude, the project's bar; the descriptors add the
    sampler's 3 x float32-vs-float64 error)."""
    g = np.load(GOLDEN)
    img = torch.from_numpy(g[f"image_u8_{tag}"]).float() / 255.0
    m = _plugin()
    full = torch.from_numpy(g[f"descriptors_default_{tag}"])
    with torch.no_grad():
        o32, o64 = net().parts(R.normalise_image(img)), net(double=True).parts(R.normalise_image(img.double()))
    sbar = 1e-4 * float(o64["score"].abs().max())
    saved = dict(m.conf)
    for name, k in (("default", None), ("top7", 7), ("above", 1000)):
        if k is not None:
            m.conf.update(max_keypoints=k)
        with torch.no_grad():
            pred = {key: v.cpu() for key, v in m({"image": img.to(DEV)}).items()}
        m.conf.clear()
        m.conf.update(saved)
        want_kp, want_sc = torch.from_numpy(g[f"keypoints_{name}_{tag}"]), torch.from_numpy(g[f"scores_{name}_{tag}"])
        want_de = full if name == "default" else full[torch.from_numpy(g[f"desc_rows_{name}_{tag}"])]
        n = len(want_sc)
        assert pred["keypoints"].shape == (1, n, 2) and pred["scores"].shape == (1, n) and pred["descriptors"].shape == (1, 128, n), (name, pred["scores"].shape)
        r64 = R.sample_descriptors(want_kp.double(), o64["desc_map"])[0].t()
        dbar = 3 * max(relmax(want_de, r64), ULP_HALF) + 1e-4
        errs = ((pred["scores"][0] - want_sc).abs().max().item(), relmax(pred["descriptors"][0].t(), want_de))
        print(f"{tag} {name} precision {precision}: {n} key-points, scores {errs[0]:.2e} (bar {sbar:.2e}), descriptors {errs[1]:.2e} (bar {dbar:.2e})")
        assert torch.equal(pred["keypoints"][0], want_kp), "the same key-points in the same order"
        assert errs[0] <= sbar and errs[1] <= dbar


def test_batch_independence_and_graph_replay_are_bitwise(precision):
    from imcui_hip import backend

    m = _plugin()
    saved = dict(m.conf)
    m.conf.update(max_keypoints=12)
    try:
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
    finally:
        m.conf.clear()
        m.conf.update(saved)


def test_refusals():
    m = _plugin()
    a = image(50, 70, 0).to(DEV)
    with pytest.raises(ValueError, match="RGB"):
        m.forward_batched(a[:, :1])
    with pytest.raises(ValueError, match="at least 16"):
        m.forward_batched(a[:, :, :15])
    with pytest.raises(ValueError, match="at least 16"):
        m.forward_batched(a[:, :, :, :15])
    # the library's own message, behind the binding's check
    from imcui_hip import backend

    hd = backend.get_handle(DEV)
    for shape, word in (((1, 1, 32, 32), "RGB"), ((1, 3, 15, 32), "at least 16")):
        rc = hd.launch(hd.lib.imcui_hip_sfd2_forward, m._impl._ca, None, None, shape[0], shape[1], shape[2], shape[3], 0.001, 4, 128, 7, 7, *([None] * 7), -1,
                       None, None, 0, check=False)  # fmt: skip
        assert rc != 0 and word in hd.lib.imcui_hip_last_error(hd.h).decode()
