"""D2-Net / RoRD on the GPU against tests/d2net_reference.py (synthetic weights seed 0, both arithmetic modes): every level's dense
features, the selection rule applied to the device's own maps (exact), the end-to-end key-point sets (equal, or every difference an
audited round-off event, at most 1 %), multi-scale (summed features, banned mask, scores / (level + 1), rescaled coordinates), crafted
maps through the detector probe, batch independence, graph replay, the plugin's output contract and the routes of the shared
convolution / GEMM launchers.

Sizes: 32 x 48 (map 7 x 11), 50 x 70 (odd halves: 25 x 35 -> 12 x 17 -> 11 x 16), 96 x 128; multi-scale 48 x 64 and 50 x 70 (levels
25 x 35, 50 x 70, 100 x 140).  Map bar: max(1e-4, 3 x the restatement's own fp32 spread over 1 / 8 threads), relative to the map's
largest magnitude.  Position bar: 3 x the restatement's own float32-against-float64 position difference on the same input, computed by
the test; on these inputs that difference is 3.2e-5 px (96 x 128), 2.3e-5 px (50 x 70 multi-scale) and 1.9e-5 px (48 x 64
multi-scale), so the bars are 9.4e-5, 7.0e-5 and 5.6e-5 px.

Measured on one MI355X, both arithmetic modes: dense features within 1.3e-06 of the restatement (its own spread at most 7.9e-07); the
rule on the device's maps exact in every case; end to end 0 key-points differ (58 / 30 / 28), descriptors within 4.9e-07, scores within
7.0e-07 of the map's magnitude, positions within 5.7e-05 / 8.8e-05 px (split / exact, 96 x 128), 2.5e-05 / 1.9e-05 px (50 x 70
multi-scale) and 3.1e-05 / 2.3e-05 px (48 x 64 multi-scale).  With one float32 summation chain over K = 4608 in the dilated layers the
maps were 3.5e-06 off and the positions up to 2.7e-04 px, three times the bar: the dilated GEMM sums long K in two levels since
(csrc/gemm.hip, GEMM_CHUNK_MIN_K)."""
from __future__ import annotations

import functools

import pytest
import torch

import d2net_reference as R
from parity_utils import oracle_spread
from test_d2net_cpu import ident, image, position_spread, reference, sd

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SS = ((32, 48), (50, 70), (96, 128))
MS = ((48, 64), (50, 70))
CASES = [(hw, False) for hw in SS] + [(hw, True) for hw in MS]
IDS = [f"{h}x{w}-{'ms' if ms else 'ss'}" for (h, w), ms in CASES]
NAN_F32 = 0x7FC00ABC  # float32 NaN with a payload no arithmetic produces
GUARD = 4096


@functools.lru_cache(maxsize=None)
def _plugin():
    from imcui_hip.hloc.extractors.d2net import D2Net

    return D2Net({"state_dict": sd()}).eval().to(DEV)


def _run(hw, ms=False, use_relu=True, maxk=0, img=None, want_maps=True, kcap=None):
    m = _plugin()
    m.conf.update(multiscale=ms, use_relu=use_relu, max_keypoints=maxk)
    out = m.forward_batched((image(*hw) if img is None else img).to(DEV), want_maps=want_maps, kcap=kcap)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _reference(hw, ms=False, use_relu=True):
    """(restatement's fp32 spread over thread counts, its result) at max_keypoints = 0; computed once per case."""
    conf = {"multiscale": ms, "use_relu": use_relu, "max_keypoints": 0}
    return oracle_spread(lambda: R.extract(sd(), image(*hw), conf), threads=(1, 8), keys=("dense_features",))


def _rel_err(a, b):
    return (a.double().cpu() - b.double()).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _level_hw(hw, ms):
    return R.level_sizes(hw[0], hw[1], [0.5, 1, 2] if ms else [1])


def _rule_on(out, b, hw, ms, maxk):
    """The restated explicit-order detector, pyramid bookkeeping and cut on image b's DEVICE maps."""
    maps = [f[b].cpu().permute(2, 0, 1).contiguous() for f in out["dense_features"]]
    return R.select(maps, hw, _level_hw(hw, ms), maxk)


def _assert_rule(out, want, b=0):
    n = int(out["num_keypoints"][b])
    assert n == want["scores"].numel(), (n, want["scores"].numel())
    assert torch.equal(out["keypoints"][b, :n].cpu(), want["keypoints"]), "coordinates (hence the step) are the rule's float32 values, in its order"
    assert torch.equal(out["scores"][b, :n].cpu(), want["scores"]), "scores are f[c, i, j] / (level + 1)"
    if n:
        assert (out["descriptors"][b, :n].cpu() - want["descriptors"]).abs().max().item() < 1e-6
    assert not out["keypoints"][b, n:].any() and not out["scores"][b, n:].any() and not out["descriptors"][b, n:].any()  # rows past the count
    return n


# ------------------------------------------------------------------ dense features
@pytest.mark.parametrize("use_relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dense_features_against_the_restatement(case, use_relu, precision):
    hw, ms = case
    spread, ref = _reference(hw, ms, use_relu)
    bar = max(1e-4, 3 * spread)
    out = _run(hw, ms, use_relu)
    assert out["levels"] == ref["levels"]
    errs = [_rel_err(a[0], b) for a, b in zip(out["dense_features"], ref["dense_features"])]
    print(f"[d2net] {hw} ms={ms} relu={use_relu} mode {precision}: levels {out['levels']}, restatement spread {spread:.1e}, bar {bar:.1e}; "
          "errors " + ", ".join(f"{e:.2e}" for e in errs))  # fmt: skip
    assert int(out["status"][0]) == 0
    if not use_relu:
        assert min(f.min().item() for f in out["dense_features"]) < 0
    for e in errs:
        assert e < bar, errs


# ------------------------------------------------------------------ selection
@pytest.mark.parametrize("cut", [False, True], ids=["all", "cut"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_selection_is_the_rule_on_the_device_maps(case, cut, precision):
    hw, ms = case
    every = _run(hw, ms)
    n_all = int(every["num_keypoints"][0])
    maxk = max(1, n_all // 2) if cut else 0
    out = _run(hw, ms, maxk=maxk) if cut else every
    assert int(out["status"][0]) == 0
    want = _rule_on(out, 0, hw, ms, maxk)
    n = _assert_rule(out, want)
    print(f"[d2net] {hw} ms={ms} max_keypoints {maxk} mode {precision}: {n} key-points over levels {sorted(set(want['level'].tolist()))}, rule exact")
    assert n_all >= 3 and (not cut or n == maxk)
    s = out["scores"][0, :n]
    assert torch.all(s[1:] >= s[:-1])


def _audit(ref64_map, c, i, j, bar):
    """A key-point present on one side only: one of the detector's decisions must lie within first-order round-off (map error bar x
    largest magnitude M per sample) of its threshold, in float64 on the restatement's map."""
    x = ref64_map.permute(2, 0, 1)
    C, h, w = x.shape
    M = x.abs().max().item()
    e1 = bar * M
    v = x[c, i, j].item()
    if x[:, i, j].max().item() - v < 2 * e1:  # the channel-wise maximum
        return "channel maximum"
    nb = x[c, max(i - 1, 0) : i + 2, max(j - 1, 0) : j + 2].flatten()
    top2 = torch.sort(nb, descending=True).values[:2]
    if abs(top2[0].item() - top2[1].item()) < 2 * e1 or 0 < top2[0].item() - v < 2 * e1:
        return "3x3 maximum"
    dii, djj, dij, di, dj = (t[c, i, j].item() for t in R.hessian_explicit(x))
    e2 = 4 * e1  # second differences
    det, tr = dii * djj - dij * dij, dii + djj
    g = e2 * (abs(dii) + abs(djj)) + 2 * e1 * abs(dij) + e2 * e2
    if abs(det) < g:
        return "determinant sign"
    if abs(tr * tr - 7.2 * det) < 4 * abs(tr) * e2 + 7.2 * g:
        return "edge ratio"
    for num, o in ((djj * di - dij * dj, i), (dii * dj - dij * di, j)):
        s = -num / det
        ds = (e2 * (abs(di) + abs(dj)) + e1 * (abs(dii) + abs(djj) + 2 * abs(dij))) / abs(det) + abs(num) * g / det**2
        p = o + s
        if abs(abs(s) - 0.5) < ds or abs(p - round(p)) < ds:
            return "step or corner"
    return None


@pytest.mark.parametrize("case", [((96, 128), False), ((50, 70), True), ((48, 64), True)], ids=["96x128-ss", "50x70-ms", "48x64-ms"])
def test_end_to_end_against_the_restatement(case, precision):
    hw, ms = case
    spread, ref = _reference(hw, ms)
    ref64 = reference(hw, torch.float64, ms)
    bar = max(1e-4, 3 * spread)
    pos_own = position_spread(ref, ref64)
    pos_bar = 3 * pos_own
    out = _run(hw, ms)
    n = int(out["num_keypoints"][0])
    dev = _rule_on(out, 0, hw, ms, 0)
    assert n == dev["scores"].numel()
    hip, want = ident(dev), ident(ref)
    diff = set(hip) ^ set(want)
    for l, c, i, j in diff:
        why = _audit(ref64["dense_features"][l], c, i, j, bar)
        assert why, f"level {l} channel {c} pixel ({i}, {j}): not a round-off event"
        print(f"[d2net] differs at level {l} channel {c} pixel ({i}, {j}): {why}")
    print(f"[d2net] end to end {hw} ms={ms} mode {precision}: {n} key-points (restatement {len(want)}), {len(diff)} differ (audited)")
    assert len(want) >= 10
    assert len(diff) <= 0.01 * len(want)
    pos = {k: q for q, k in enumerate(hip)}
    common = [(q, pos[k]) for q, k in enumerate(want) if k in pos]
    jr, jh = torch.tensor([c[0] for c in common]), torch.tensor([c[1] for c in common])
    M = max(f.abs().max().item() for f in ref["dense_features"])
    e_d = (out["descriptors"][0, :n].cpu()[jh] - ref["descriptors"][jr]).abs().max().item()
    e_s = (out["scores"][0, :n].cpu()[jh] - ref["scores"][jr]).abs().max().item() / M
    e_k = (out["keypoints"][0, :n].cpu()[jh].double() - ref["keypoints"][jr].double()).abs().max().item()
    print(f"[d2net] common key-points: descriptors {e_d:.2e}, scores {e_s:.2e} (relative to the map), positions {e_k:.2e} px "
          f"(restatement float32 / float64 {pos_own:.2e} px, bar {pos_bar:.2e} px)")  # fmt: skip
    assert e_d < bar and e_s < bar
    assert e_k <= pos_bar, (e_k, pos_bar)


@pytest.mark.parametrize("hw", MS, ids=[f"{h}x{w}" for h, w in MS])
def test_multiscale_bookkeeping(hw, precision):
    """On the device's own maps: no pixel carries detections of two levels (the banned mask through ATen's nearest rule), the score is the
    map value divided by 1, 2, 3, coordinates are rescaled into the input image."""
    out = _run(hw, True)
    n = int(out["num_keypoints"][0])
    want = _rule_on(out, 0, hw, True, 0)
    _assert_rule(out, want)
    levels = want["level"].tolist()
    assert len(set(levels)) >= 2 and n >= 10
    sizes = out["levels"]
    assert sizes == [(a // 4 - 1, b // 4 - 1) for a, b in _level_hw(hw, True)]
    for q, (l, c, i, j) in enumerate(ident(want)):
        f = out["dense_features"][l][0, i, j, c].item()
        assert out["scores"][0, q].item() == (torch.tensor(f) / (l + 1)).item()
        for lower in range(l):  # the pixel's source at every earlier level, one nearest step at a time, was not detected there
            ii, jj = i, j
            for k in range(l, lower, -1):
                ii = min(int(torch.floor(torch.tensor(ii, dtype=torch.float32) * torch.tensor(sizes[k - 1][0] / sizes[k][0], dtype=torch.float32))), sizes[k - 1][0] - 1)
                jj = min(int(torch.floor(torch.tensor(jj, dtype=torch.float32) * torch.tensor(sizes[k - 1][1] / sizes[k][1], dtype=torch.float32))), sizes[k - 1][1] - 1)
            assert not want["banned"][lower][ii, jj], (l, i, j, lower)
    kp = out["keypoints"][0, :n]
    assert kp[:, 0].min() >= 0 and kp[:, 0].max() < hw[1] and kp[:, 1].min() >= 0 and kp[:, 1].max() < hw[0]


# ------------------------------------------------------------------ crafted maps through the detector probe
def _blank(h, w, C=64):
    return torch.zeros(1, h, w, C)


def _blob(f, c, ci, cj, amp=1.0, si=1.0, sj=1.0):
    h, w = f.shape[1:3]
    ii, jj = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    f[0, :, :, c] += amp * torch.exp(-((ii - ci) ** 2) / (2 * si * si) - ((jj - cj) ** 2) / (2 * sj * sj))
    return f


def _probe(f, maxk=0, kcap=None):
    from imcui_hip import backend

    out = backend.D2NetHIP().detect_probe(f.to(DEV), maxk, kcap)
    torch.cuda.synchronize()
    return out


def _probe_rule(f, maxk=0):
    h, w = f.shape[1:3]
    return R.select([f[0].permute(2, 0, 1).contiguous()], (h, w), [(h, w)], maxk)


def _probe_checked(f, maxk=0):
    out, want = _probe(f, maxk), _probe_rule(f, maxk)
    assert int(out["status"][0]) == 0
    for k in ("keypoints", "scores", "descriptors"):
        assert torch.isfinite(out[k]).all(), k
    _assert_rule(out, want)
    return out, want


def test_crafted_single_peak(precision):
    out, want = _probe_checked(_blob(_blank(5, 7), 5, 2.2, 2.9))
    assert ident(want) == [(0, 5, 2, 3)]
    p = want["p"][0]
    assert abs(p[0].item() - 2.2) < 0.1 and abs(p[1].item() - 2.9) < 0.1  # the step moves towards the true centre
    assert out["keypoints"][0, 0].tolist() == [((p[1] * 2 + 0.5) * 2 + 0.5).item(), ((p[0] * 2 + 0.5) * 2 + 0.5).item()]


@pytest.mark.parametrize("at", [(0, 0), (0, 3), (2, 0), (8, 4), (4, 8), (8, 8)], ids=lambda a: f"{a[0]}_{a[1]}")
def test_crafted_peak_on_the_border(at, precision):
    """The Hessian filters pad with zeros, the 3x3 maximum looks at the map only; the step of a border peak points inwards."""
    out, want = _probe_checked(_blob(_blank(9, 9), 7, float(at[0]), float(at[1])))
    assert ident(want) == [(0, 7, at[0], at[1])]


def test_crafted_two_channels_tied_for_the_maximum(precision):
    f = _blob(_blob(_blank(5, 7), 5, 2.0, 3.0), 9, 2.0, 3.0)
    out, want = _probe_checked(f)
    assert ident(want) == [(0, 5, 2, 3), (0, 9, 2, 3)]  # both detected, equal scores in channel order


def test_crafted_ridge_is_rejected_and_a_blob_just_inside_is_kept(precision):
    """Separable peaks with curvature ratio r give (tr tr) / det = r + 2 + 1 / r: 7.2 at r = 5 (edge_threshold)."""
    for r, expect in ((6.0, 0), (4.8, 1)):
        b = 0.1
        a = r * b
        f = _blank(9, 9)
        ii, jj = torch.meshgrid(torch.arange(9).float(), torch.arange(9).float(), indexing="ij")
        f[0, :, :, 3] = (1 - a) ** ((ii - 4) ** 2) * (1 - b) ** ((jj - 4) ** 2)
        out, want = _probe_checked(f)
        assert int(out["num_keypoints"][0]) == expect, (r, ident(want))


def test_crafted_plateau_and_all_zero_map(precision):
    """A constant channel: det = 0 inside and on the borders (0 / 0 in the ratio), the four corners are detected with a step of 2 / 3
    and dropped; nothing is written but zeros.  An all-zero map ties all 64 channels everywhere and detects nothing."""
    f = _blank(9, 9)
    f[..., 2] = 1.0
    det, si, sj = R.detect(f[0].permute(2, 0, 1))
    assert det.sum().item() == 4 and si[det].abs().min().item() >= 0.5
    for m in (f, _blank(5, 7)):
        out, want = _probe_checked(m)
        assert int(out["num_keypoints"][0]) == 0 and int(out["status"][0]) == 0
        assert not out["keypoints"].any() and not out["scores"].any() and not out["descriptors"].any()


def test_crafted_step_of_one_half_is_dropped(precision):
    """centre == right neighbour: step_j = ((r - l) / 2) / (2c - l - r) = 1 / 2 exactly, and |step| < 0.5 fails."""
    f = _blank(5, 7)
    f[0, 2, 3, 4], f[0, 2, 4, 4], f[0, 1, 3, 4], f[0, 3, 3, 4] = 1.0, 1.0, 0.5, 0.5
    det, si, sj = R.detect(f[0].permute(2, 0, 1))
    assert det[4, 2, 3] and sj[4, 2, 3].item() == 0.5
    out, want = _probe_checked(f)
    assert (0, 4, 2, 3) not in ident(want)


def test_crafted_ceil_corner_outside_is_dropped(precision):
    """Bottom row, a small positive peak over a negative channel: the step is +0.357 rows, ceil(p_i) = h."""
    f = _blank(5, 7)
    f[...] = -10.0
    f[..., 6] = -0.5
    f[0, 4, 3, 6] = 0.1
    det, si, sj = R.detect(f[0].permute(2, 0, 1))
    assert det[6, 4, 3] and 0 < si[6, 4, 3].item() < 0.5 and abs(sj[6, 4, 3].item()) < 0.5
    out, want = _probe_checked(f)
    assert (0, 6, 4, 3) not in ident(want)


def _sentinel(n):
    return torch.full((n,), NAN_F32, dtype=torch.int32, device=DEV).view(torch.float32)


def test_crafted_capacity_overflow_by_ties(precision):
    """The same peak in all 64 channels: 64 candidates at one pixel against kcap = 10.  The status bit is set, the outputs hold the
    first ten candidates in the rule's order and nothing is written outside the output buffers (NaN-payload guard bands)."""
    from imcui_hip import backend

    f = _blank(5, 7)
    for c in range(64):
        _blob(f, c, 2.0, 3.0)
    want = _probe_rule(f)
    assert ident(want) == [(0, c, 2, 3) for c in range(64)]
    kcap, B, C = 10, 1, 64
    hd = backend.get_handle(DEV)
    sizes = {"keypoints": B * kcap * 2, "scores": B * kcap, "descriptors": B * kcap * C, "num_keypoints": B, "status": 1}
    bufs = {k: _sentinel(2 * GUARD + n) for k, n in sizes.items()}
    view = {k: b[GUARD : GUARD + sizes[k]] for k, b in bufs.items()}
    fd = f.to(DEV)
    ws = torch.empty(hd.lib.imcui_hip_d2net_probe_workspace_bytes(B, 5, 7, C, kcap), dtype=torch.uint8, device=DEV)
    ptr = backend._ptr
    hd.launch(hd.lib.imcui_hip_d2net_detect_probe, ptr(fd), B, 5, 7, C, 0, kcap, kcap, ptr(view["keypoints"]), ptr(view["scores"]), ptr(view["descriptors"]),
              ptr(view["num_keypoints"]), ptr(view["status"]), ptr(ws), ws.numel())  # fmt: skip
    torch.cuda.synchronize()
    for k, b in bufs.items():
        bits = b.view(torch.int32).cpu()
        assert (bits[:GUARD] == NAN_F32).all() and (bits[GUARD + sizes[k] :] == NAN_F32).all(), f"{k}: written outside the buffer"
        assert (bits[GUARD : GUARD + sizes[k]] != NAN_F32).all(), f"{k}: not written completely"
    assert view["status"].view(torch.int32).item() & 2
    assert view["num_keypoints"].view(torch.int32).item() == kcap
    assert torch.equal(view["scores"].cpu(), want["scores"][:kcap])
    assert torch.equal(view["keypoints"].cpu().view(kcap, 2), want["keypoints"][:kcap])
    assert int(_probe(f, kcap=64)["status"][0]) == 0  # room for every tie: no overflow


def test_crafted_equal_scores_across_a_cut_follow_the_stable_rule(precision):
    """Two tied channels at one pixel and a higher peak elsewhere, max_keypoints 2: the LATER of the tied candidates survives."""
    f = _blob(_blob(_blob(_blank(9, 9), 5, 2.0, 2.0), 9, 2.0, 2.0), 1, 6.0, 6.0, amp=2.0)
    out, want = _probe_checked(f, maxk=2)
    assert ident(want) == [(0, 9, 2, 2), (0, 1, 6, 6)]
    every, _ = _probe_checked(f)
    assert int(every["num_keypoints"][0]) == 3


# ------------------------------------------------------------------ batches, graphs, the plugin
def test_batch_independence_and_graph_replay_are_bitwise(precision):
    from imcui_hip import backend

    hw = (48, 64)
    m = _plugin()
    m.conf.update(multiscale=True, use_relu=True, max_keypoints=20)
    a, b, c = (image(*hw, seed=s).to(DEV) for s in (0, 3, 4))
    keys = ("keypoints", "scores", "descriptors", "num_keypoints")
    solo = m.forward_batched(a)
    trio = m.forward_batched(torch.cat([b, a, c]))
    assert int(solo["num_keypoints"][0]) >= 10
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


@pytest.mark.parametrize("module", ["d2net", "rord"])
def test_plugin_output_contract(module, precision):
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.utils.base_model import dynamic_load

    hw = (96, 128)
    m = dynamic_load(extractors, module)({"state_dict": sd(), "max_keypoints": 40}).eval().to(DEV)
    pred = m({"image": image(*hw).to(DEV)})
    kp, de, sc = pred["keypoints"], pred["descriptors"], pred["scores"]
    assert kp.shape == (1, 40, 2) and de.shape == (1, 512, 40) and sc.shape == (1, 40)
    assert kp.dtype == de.dtype == sc.dtype == torch.float32 and kp.is_cuda and de.is_contiguous()
    assert torch.all(sc[0, 1:] >= sc[0, :-1])
    assert (de[0].norm(dim=0) - 1).abs().max().item() < 1e-5
    assert kp[..., 0].min() >= 0 and kp[..., 0].max() < hw[1] and kp[..., 1].min() >= 0 and kp[..., 1].max() < hw[0]
    ref = _plugin()
    ref.conf.update(multiscale=False, use_relu=True, max_keypoints=40)
    same = ref({"image": image(*hw).to(DEV)})
    for k in pred:
        assert torch.equal(pred[k], same[k]), k  # RoRD is D2-Net's code with its own weights: the same weights give the same bits


def test_routes_of_d2net_have_kernel_level_cases(precision):
    """Every (route, feature) pair D2-Net makes through the shared 3x3 launchers is in the case table of tests/test_gpu_conv_variants.py,
    every GEMM route in tests/test_gpu_gemm_dilated.py; tests/test_gpu_d2net_layers.py enters D2-Net's own shapes on these routes."""
    from imcui_hip import backend as be

    import test_gpu_conv_variants as tc
    import test_gpu_gemm_dilated as tg

    dil_routes = {be.gemm_route(r, "conv") for c in tg.OTHER for r in c["routes"].values()} | {be.gemm_route("convd_128", "conv"), be.gemm_route("exact_dil", "conv")}
    for hw, ms in (((50, 70), True), ((96, 128), False)):  # odd maps (un-pooled launches) and even ones (fused pool)
        be.gemm_route_reset(DEV)
        be.conv_route_reset(DEV)
        _run(hw, ms, want_maps=False)
        seen = be.gemm_route_counts(DEV)
        nlev = 3 if ms else 1
        print(f"[d2net] {hw} mode {precision}: GEMM routes " + ", ".join(f"{be.gemm_route_name(r)} x{n}" for r, n in sorted(seen.items())))
        assert sum(seen.values()) == 3 * nlev and not set(seen) - dil_routes, [be.gemm_route_name(r) for r in set(seen) - dil_routes]
        counts, feats = be.conv_route_counts(DEV), be.conv_route_features(DEV)
        assert sum(counts.values()) == 6 * nlev
        pairs = set()
        for r in counts:
            name = be.conv_route_name(r)
            pairs.add((name, 0))
            pairs |= {(name, bit) for bit in tc.FEATURES.values() if feats.get(r, 0) & bit}
        print(f"[d2net] {hw} mode {precision}: conv (route, feature) " + ", ".join(f"{r}+{b}" for r, b in sorted(pairs)))
        assert not pairs - tc.covered_pairs(), pairs - tc.covered_pairs()
        assert all(r.startswith("f32" if precision == 0 else "split") for r, _ in pairs)
