"""R2D2 on the GPU against tests/r2d2_reference.py (synthetic weights seed 0, both arithmetic modes): the per-level maps, the probe's
descriptors, the selection rule applied to the HIP maps (exact), the end-to-end key-point sets (equal, or every difference an audited
round-off event, at most 1 %), a flat image (plateau, capacity overflow, retry), zero key-points, a cut through tied scores,
max_keypoints = 0, batch independence, graph replay, the plugin's output contract and the routes of the shared GEMM.

Sizes: 24 x 40 (min_size 8: the last levels are smaller than the dilation-16 tap span), 48 x 64 (min_size 16), 100 x 150 (min_size 24:
odd level sizes on both axes, 11 levels).  The thresholds are the defaults 0.7 / 0.7, which cut through both maps of the seeded
network (tests/test_r2d2_cpu.py).  Map bar: max(1e-4, 3 x the restatement's own fp32 spread), relative to the map's largest magnitude.

Measured on one MI355X, both arithmetic modes: maps within 5.3e-06 of the restatement (its own spread over 1 / 8 threads at most
2.2e-06); the rule on the HIP maps exact in every case; end to end 0 key-points differ, descriptors within 4.5e-07 and scores within
1.9e-06 at the common key-points, positions bitwise equal."""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

import r2d2_reference as R
from parity_utils import oracle_spread
from test_r2d2_cpu import image

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES = {(24, 40): 8, (48, 64): 16, (100, 150): 24}  # (H, W) -> min_size
IDS = [f"{h}x{w}" for h, w in SIZES]


def _sd():
    from imcui_hip.synth_weights import r2d2_state_dict

    return r2d2_state_dict(0)


@functools.lru_cache(maxsize=None)
def _plugin():
    from imcui_hip.hloc.extractors.r2d2 import R2D2

    return R2D2({"state_dict": _sd()}).eval().to(DEV)


def _conf(hw, **kw):
    return {**R.DEFAULT_CONF, "min_size": SIZES.get(hw, max(hw)), "max_keypoints": 0, **kw}  # (a size outside the table: one level)


def _run(hw, img=None, kcap="all", want_maps=True, **kw):
    m = _plugin()
    m.conf.update(_conf(hw, **kw))
    out = m.forward_batched((image(*hw) if img is None else img).to(DEV), want_maps=want_maps, kcap=kcap)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _reference(hw):
    """(restatement's fp32 spread over thread counts, its result) at max_keypoints = 0; computed once per size."""
    sd, img, conf = _sd(), image(*hw), _conf(hw)
    spread, ref = oracle_spread(lambda: R.extract(sd, img, conf), threads=(1, 8), keys=("reliability", "repeatability", "final_map"))
    return spread, ref


def _rel_err(a, b):
    return (a.double().cpu() - b.double()).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _rule_on(out, b, hw, conf):
    """The restated detector + cut on image b's HIP maps."""
    maps = [(rl[b].cpu(), rp[b].cpu()) for rl, rp in zip(out["reliability"], out["repeatability"])]
    x, y, s, lev, idx = R.candidates(maps, hw[0], hw[1], conf["reliability_threshold"], conf["repetability_threshold"])
    keep = R.cut(s, int(conf["max_keypoints"] or 0))
    return torch.stack([x[keep], y[keep]], 1), s[keep], lev[keep], idx[keep]


def _assert_rule(out, b, hw, conf):
    kp, s, lev, idx = _rule_on(out, b, hw, conf)
    n = int(out["num_keypoints"][b])
    assert n == kp.shape[0], (n, kp.shape[0])
    assert torch.equal(out["keypoints"][b, :n].cpu(), kp), "coordinates are the float32 (x * W) / nw, in the rule's order"
    assert torch.equal(out["scores"][b, :n].cpu(), s), "scores are the float32 product"
    if n:
        want = torch.stack([F.normalize(out["final_map"][l][b].reshape(-1, 128)[i].cpu(), dim=0) for l, i in zip(lev.tolist(), idx.tolist())])
        assert (out["descriptors"][b, :n].cpu() - want).abs().max().item() < 1e-6
    assert not out["keypoints"][b, n:].any() and not out["scores"][b, n:].any() and not out["descriptors"][b, n:].any()  # rows past the count
    return n, lev


# ------------------------------------------------------------------ maps
@pytest.mark.parametrize("hw", list(SIZES), ids=IDS)
def test_per_level_maps_against_the_restatement(hw, precision):
    spread, ref = _reference(hw)
    bar = max(1e-4, 3 * spread)
    out = _run(hw)
    assert out["levels"] == ref["levels"] and len(ref["levels"]) >= 4
    worst = {}
    for key in ("reliability", "repeatability", "final_map"):
        worst[key] = max(_rel_err(a[0], b) for a, b in zip(out[key], ref[key]))
    print(f"[r2d2] {hw} mode {precision}: {len(ref['levels'])} levels, restatement spread {spread:.1e}, bar {bar:.1e}; errors "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))  # fmt: skip
    assert int(out["status"][0]) == 0
    for k, v in worst.items():
        assert v < bar, (k, v)


def test_probe_descriptors_are_the_normalised_map(precision):
    hw = (24, 40)
    spread, ref = _reference(hw)
    m = _plugin()
    ys, xs = torch.meshgrid(torch.arange(hw[0]), torch.arange(hw[1]), indexing="ij")
    xy = torch.stack([xs.flatten(), ys.flatten()], 1)
    d = m._impl.desc_probe(m.packed, image(*hw).to(DEV), xy).cpu()
    out = _run(hw)
    own = F.normalize(out["final_map"][0][0].reshape(-1, 128), dim=1).cpu()
    want = F.normalize(ref["final_map"][0].reshape(-1, 128), dim=1)
    e_own, e_ref = (d - own).abs().max().item(), (d - want).abs().max().item()
    print(f"[r2d2] probe mode {precision}: against F.normalize of the HIP map {e_own:.2e}, of the restatement's {e_ref:.2e}")
    assert e_own < 1e-6 and e_ref < max(1e-4, 3 * spread)
    assert (d.norm(dim=1) - 1).abs().max().item() < 1e-5


# ------------------------------------------------------------------ selection
@pytest.mark.parametrize("maxk", [0, 30], ids=["all", "cut30"])
@pytest.mark.parametrize("hw", list(SIZES), ids=IDS)
def test_selection_is_the_rule_on_the_hip_maps(hw, maxk, precision):
    conf = _conf(hw, max_keypoints=maxk)
    out = _run(hw, max_keypoints=maxk)
    assert int(out["status"][0]) == 0
    n, lev = _assert_rule(out, 0, hw, conf)
    print(f"[r2d2] {hw} max_keypoints {maxk} mode {precision}: {n} key-points over {len(set(lev.tolist()))} levels, rule exact")
    assert n > 20 and (maxk == 0 or n == maxk)
    s = out["scores"][0, :n]
    assert torch.all(s[1:] >= s[:-1])


def test_end_to_end_against_the_restatement(precision):
    hw = (100, 150)
    spread, ref = _reference(hw)
    bar = max(1e-4, 3 * spread)
    conf = _conf(hw)
    out = _run(hw)
    n = int(out["num_keypoints"][0])
    _, _, lev, idx = _rule_on(out, 0, hw, conf)
    hip = list(zip(lev.tolist(), idx.tolist()))
    want = list(zip(ref["level"].tolist(), ref["index"].tolist()))
    diff = set(hip) ^ set(want)
    for l, i in diff:  # a threshold crossed, or the 3x3 maximum decided, by less than the map bar
        rel, rep = ref["reliability"][l].flatten(), ref["repeatability"][l]
        y, x = divmod(i, rep.shape[1])
        nb = rep[max(y - 1, 0) : y + 2, max(x - 1, 0) : x + 2]
        srt = torch.sort(nb.flatten(), descending=True).values
        v = rep[y, x].item()
        margin = (srt[0] - srt[1]).item() if v == srt[0].item() else srt[0].item() - v  # how clearly the pixel is (not) the 3x3 maximum
        ok = abs(v - conf["repetability_threshold"]) < bar or abs(rel[i].item() - conf["reliability_threshold"]) < bar or margin < bar
        assert ok, f"level {l} pixel {i}: rep {v}, rel {rel[i].item()}, neighbourhood max {nb.max().item()}: not a round-off event"
    print(f"[r2d2] end to end mode {precision}: {n} key-points (restatement {len(want)}) over {len(set(ref['level'].tolist()))} levels, {len(diff)} differ (audited)")
    assert len(want) >= 200 and len(set(ref["level"].tolist())) >= 4
    assert len(diff) <= 0.01 * len(want)
    pos = {k: j for j, k in enumerate(hip)}
    common = [(j, pos[k]) for j, k in enumerate(want) if k in pos]
    jr, jh = torch.tensor([c[0] for c in common]), torch.tensor([c[1] for c in common])
    e_d = (out["descriptors"][0, :n].cpu()[jh] - ref["descriptors"][jr]).abs().max().item()
    e_s = (out["scores"][0, :n].cpu()[jh] - ref["scores"][jr]).abs().max().item()
    e_k = (out["keypoints"][0, :n].cpu()[jh] - ref["keypoints"][jr]).abs().max().item()
    print(f"[r2d2] common key-points: descriptors {e_d:.2e}, scores {e_s:.2e}, positions {e_k:.1e}")
    assert e_d < bar and e_s < bar and e_k == 0.0


# ------------------------------------------------------------------ plateaus, capacity, ties, none
def test_flat_image_overflows_the_default_capacity_and_is_retried(precision):
    """A constant image, one level of 160 x 160: more than 25 pixels from the border (the sum of the paddings) every map is constant
    and every pixel of that 110 x 110 plateau is a 3x3 maximum.  With both thresholds at 0 the candidates outnumber the default
    capacity (a quarter of the pixels): status bit 1; forward_checked retries with room for every pixel and returns what the rule
    gives on the HIP maps."""
    hw = (160, 160)
    flat = torch.full((1, 3, *hw), 0.4)
    kw = dict(reliability_threshold=0.0, repetability_threshold=0.0)
    first = _run(hw, flat, kcap=None, **kw)
    assert int(first["status"][0]) & 2
    m = _plugin()
    m.conf.update(_conf(hw, **kw))
    out, counts = m.forward_checked(flat.to(DEV))
    full = _run(hw, flat, **kw)
    n, _ = _assert_rule(full, 0, hw, _conf(hw, **kw))
    npix = sum(a * b for a, b in full["levels"])
    print(f"[r2d2] flat image mode {precision}: {n} key-points of {npix} pixels after the retry")
    assert counts == [n] and n > npix // 4  # (more than the default capacity: what made the first call overflow)
    for k in ("keypoints", "scores", "descriptors"):
        assert torch.equal(out[k][0, :n], full[k][0, :n]), k


def test_max_keypoints_cuts_through_a_tie(precision):
    """The flat image again: the plateau's scores tie exactly; of equal scores the LATER candidates survive the cut and come later."""
    hw = (160, 160)
    flat = torch.full((1, 3, *hw), 0.4)
    kw = dict(reliability_threshold=0.0, repetability_threshold=0.0)
    every = _run(hw, flat, want_maps=False, **kw)
    s = every["scores"][0, : int(every["num_keypoints"][0])].cpu()
    plateau = s.mode().values.item()
    assert (s == plateau).sum().item() > 150  # (the plateau: its exact size depends on how far round-off leaves the interior constant)
    maxk = int((s > plateau).sum()) + 150  # everything above the plateau and 150 of its tied candidates
    out = _run(hw, flat, max_keypoints=maxk, **kw)
    n, _ = _assert_rule(out, 0, hw, _conf(hw, max_keypoints=maxk, **kw))
    assert n == maxk and (out["scores"][0, :n].cpu() == plateau).sum().item() == 150, "the cut must pass through tied scores"


def test_zero_keypoints(precision):
    hw = (24, 40)
    out = _run(hw, reliability_threshold=1.5)
    assert int(out["num_keypoints"][0]) == 0 and int(out["status"][0]) == 0
    assert not out["keypoints"].any() and not out["scores"].any() and not out["descriptors"].any()
    m = _plugin()
    pred = m({"image": image(*hw).to(DEV)})
    assert pred["keypoints"].shape == (1, 0, 2) and pred["descriptors"].shape == (1, 128, 0) and pred["scores"].shape == (1, 0)


# ------------------------------------------------------------------ batches, graphs, the plugin
def test_batch_independence_and_graph_replay_are_bitwise(precision):
    from imcui_hip import backend

    hw = (48, 64)
    m = _plugin()
    m.conf.update(_conf(hw, max_keypoints=100))
    a, b, c = (image(*hw, seed=s).to(DEV) for s in (0, 3, 4))
    keys = ("keypoints", "scores", "descriptors", "num_keypoints")
    solo = m.forward_batched(a)
    trio = m.forward_batched(torch.cat([b, a, c]))
    assert int(solo["num_keypoints"][0]) > 20
    for k in keys:
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
        for k in keys:
            assert torch.equal(eager[k], cap[k]), k


def test_plugin_output_contract(precision):
    hw = (48, 64)
    m = _plugin()
    m.conf.update(_conf(hw, max_keypoints=50))
    pred = m({"image": image(*hw).to(DEV)})
    kp, de, sc = pred["keypoints"], pred["descriptors"], pred["scores"]
    assert kp.shape == (1, 50, 2) and de.shape == (1, 128, 50) and sc.shape == (1, 50)
    assert kp.dtype == de.dtype == sc.dtype == torch.float32 and kp.is_cuda and de.is_contiguous()
    assert torch.all(sc[0, 1:] >= sc[0, :-1])
    assert (de[0].norm(dim=0) - 1).abs().max().item() < 1e-5
    assert kp[..., 0].min() >= 0 and kp[..., 0].max() < hw[1] and kp[..., 1].min() >= 0 and kp[..., 1].max() < hw[0]


def test_gemm_routes_of_r2d2_have_kernel_level_cases(precision):
    """Every GEMM route R2D2 launches is one tests/test_gpu_gemm_dilated.py enters directly."""
    from imcui_hip import backend

    import test_gpu_gemm_dilated as t

    be = backend
    covered = {be.gemm_route("exact", "conv"), be.gemm_route("exact_dil", "conv"), be.gemm_route("conv_128", "conv"), be.gemm_route("convd_128", "conv")}
    assert {(3, 1, 1, 32, 32), (3, 2, 2, 64, 128), (2, 16, 8, 128, 128)} <= set(t.LAYERS)
    be.gemm_route_reset(DEV)
    _run((48, 64), want_maps=False, kcap=None)
    seen = be.gemm_route_counts(DEV)
    print(f"[r2d2] mode {precision}: routes " + ", ".join(f"{be.gemm_route_name(r)} x{n}" for r, n in sorted(seen.items())))
    assert seen and sum(seen.values()) == 8 * 9  # eight matrix layers on each of the nine levels
    assert not set(seen) - covered, [be.gemm_route_name(r) for r in set(seen) - covered]
