"""ALIKED on the MI355X (imcui/hloc/extractors/aliked.py:24-32 -> LightGlue's ALIKED) against the CPU restatement
(tests/aliked_reference.py), in both arithmetic modes: the dense score map, the DKD rule on the HIP score map (exact candidate set,
refined positions), the end-to-end key-point sets (equal, or every difference an audited round-off tie, at most 1 %), descriptors and
key-point scores at the HIP key-points, the deformable blocks alone, batch independence, graph replay, the plugin's output contract,
the capacity retry and the routes of the shared GEMM."""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

from aliked_reference import ALIKEDReference, dkd_refine, dkd_select, simple_nms
from parity_utils import oracle_spread
from test_aliked_cpu import image

pytestmark = pytest.mark.gpu

SIZES = {"480x640": (480, 640, 0), "472x632": (472, 632, 1), "768x1024": (768, 1024, 2)}
CONFS = {
    "default": dict(max_num_keypoints=-1, detection_threshold=0.2, nms_radius=2),
    "top2048": dict(max_num_keypoints=2048, detection_threshold=-1.0, nms_radius=2),
    "n300-thr": dict(max_num_keypoints=300, detection_threshold=0.2, nms_radius=2),
}
CASES = [(s, c) for s in SIZES for c in CONFS]


@functools.lru_cache(maxsize=None)
def _sd(shift: float = -3.6):
    from imcui_hip.synth_weights import aliked_state_dict

    return aliked_state_dict(0, score_shift=shift)


@functools.lru_cache(maxsize=None)
def _oracle(size: str):
    """(image, the restatement's dense outputs, fp32 spread of those)."""
    h, w, seed = SIZES[size]
    img = image(h, w, seed)
    ref = ALIKEDReference(_sd())
    spread, d = oracle_spread(lambda: ref.dense(img), threads=(1, 8))  # measured at every size the bar is used at
    return img, d, spread


def _bar(size):
    return max(1e-4, 3 * _oracle(size)[2])


@functools.lru_cache(maxsize=None)
def _plugin(shift: float = -3.6):
    from imcui_hip.hloc.extractors.aliked import ALIKED

    return ALIKED({"state_dict": _sd(shift)}).eval().to("cuda:0")


@functools.lru_cache(maxsize=None)
def _hip(size: str, conf: str, precision: int, shift: float = -3.6):
    """One HIP run with the debug maps, on the CPU: per-image slices of image 0."""
    m = _plugin(shift)
    m.conf.update(CONFS[conf])
    out = m.forward_batched(_oracle(size)[0].cuda(), want_maps=True)
    torch.cuda.synchronize()
    assert int(out["status"]) == 0
    n = int(out["num_keypoints"][0])
    o = {k: v[0].cpu() for k, v in out.items() if k not in ("status", "num_keypoints")}
    for k in ("keypoints", "keypoints_norm", "scores", "descriptors"):
        assert not o[k][n:].any(), k  # entries past the count are zero
        o[k] = o[k][:n]
    o["n"] = n
    return o


def _rule(score_map, conf):
    c = CONFS[conf]
    return dkd_select(score_map, c["nms_radius"], c["detection_threshold"], c["max_num_keypoints"])[0]


# ------------------------------------------------------------------ dense maps
@pytest.mark.parametrize("size", list(SIZES))
def test_score_map_matches_the_restatement(size, precision):
    ref = _oracle(size)[1]["score_map"][0, 0]
    got = _hip(size, "default", precision)["score_map"]
    err = (got - ref).abs().max().item()
    print(f"{size} score map: max error {err:.2e} (bar {_bar(size):.1e}, oracle spread {_oracle(size)[2]:.1e})")
    assert got.shape == ref.shape and err <= _bar(size)


@pytest.mark.parametrize("size", list(SIZES))
def test_deformable_blocks_match_the_restatement(size, precision):
    """x3 (1/8) and x4 (1/32), the outputs of the blocks built on deformable convolutions; the seeded offsets reach the clamp of the
    1/32 map and samples fall outside both maps, so the zero-outside rule and the clamp are exercised."""
    img, d, _ = _oracle(size)
    ref = ALIKEDReference(_sd())
    xs, _ = ref.branches(ref.pad(img)[0])
    o4 = ref.block4.conv1.offsets(F.avg_pool2d(xs[2], 4))
    h4, w4 = o4.shape[2:]
    assert (o4.abs() == max(h4, w4) / 4.0).any(), "no offset at the clamp"
    ys = torch.arange(h4)[:, None] + o4[0, 0::2]
    assert ((ys < -1) | (ys > h4)).any(), "no sample outside the map"
    hip = _hip(size, "default", precision)
    for name in ("x3", "x4"):
        want, got = d[name][0], hip[name].permute(2, 0, 1)
        err = (got - want).abs().max().item() / max(1.0, want.abs().max().item())
        print(f"{size} {name}: relative error {err:.2e} at scale {want.abs().max().item():.1f} (bar {_bar(size):.1e})")
        assert got.shape == want.shape and err <= _bar(size)


# ------------------------------------------------------------------ selection
@pytest.mark.parametrize("size,conf", CASES)
def test_selection_is_the_rule_on_the_hip_score_map(size, conf, precision):
    """DKD's rule (tests/aliked_reference.py) applied to the HIP score map returns exactly the HIP candidates, in the same row-major
    order; the refined positions agree within 2e-3 px (the bar of LoFTR's fine key-points) and the sampled scores within the bar."""
    hip = _hip(size, conf, precision)
    sm = hip["score_map"]
    idx = _rule(sm, conf)
    assert hip["n"] == idx.numel() and hip["n"] > 100, (hip["n"], idx.numel())
    if conf == "n300-thr":
        assert hip["n"] == 300 and int((simple_nms(sm[None, None], 2) > 0.2).sum()) > 300  # the n_limit cut is taken
    kn, ks = dkd_refine(sm, idx, CONFS[conf]["nms_radius"])
    h, w = sm.shape
    kp = kn.new_tensor([w - 1, h - 1]) * (kn + 1) / 2
    # a differing candidate would sit at least a pixel away from the rule's
    err = (hip["keypoints"] - kp).abs().max().item()
    print(f"{size} {conf}: {hip['n']} key-points, refined position error {err:.2e} px, score error {(hip['scores'] - ks).abs().max().item():.2e}")
    assert err <= 2e-3  # both sides refine on the SAME score map: fp32 round-off of the soft-argmax only
    assert (hip["keypoints_norm"] - kn).abs().max().item() <= 2 * 2e-3 / (max(h, w) - 1)  # the same bar in [-1, 1] units
    assert (hip["scores"] - ks).abs().max().item() <= _bar(size)


def _cut(sm, idx, conf):
    """The score at which the n_limit / top-k cut fell on this map (None when the rule kept every candidate)."""
    c = CONFS[conf]
    limit = c["max_num_keypoints"] if c["max_num_keypoints"] > 0 else 20000
    return sm.reshape(-1)[idx].min().item() if idx.numel() == limit else None


def _audit(diff, sm_hip, sm_ref, idx_hip, idx_ref, conf):
    """As tests/test_gpu_disk.py audits DISK: every key-point in one set but not the other must be a round-off tie, i.e. the margin
    that decides it -- against the threshold, against the cut of either map, or against a pixel of its own NMS window -- lies
    below twice the MEASURED difference of the two score maps.  simple_nms iterates, so a flipped maximum can free or suppress a
    second one up to 2r away: such a key-point passes only next to a differing key-point that passed on its own margin."""
    c = CONFS[conf]
    r, thr = c["nms_radius"], max(c["detection_threshold"], 0.0)
    h, w = sm_ref.shape
    tol = 2 * (sm_hip - sm_ref).abs().max().item()
    cuts = [v for v in (_cut(sm_ref, idx_ref, conf), _cut(sm_hip, idx_hip, conf)) if v is not None]
    own, margin = set(), {}
    for i in diff:
        y, x = divmod(i, w)
        v = sm_ref[y, x].item()
        y0, x0 = max(0, y - r), max(0, x - r)
        win = sm_ref[y0 : y + r + 1, x0 : x + r + 1].clone()
        win[y - y0, x - x0] = float("inf")  # the pixel itself
        margin[i] = min([abs(v - thr), (win - v).abs().min().item()] + [abs(v - t) for t in cuts])
        if margin[i] < tol:
            own.add(i)
    for i in diff:
        if i not in own:
            y, x = divmod(i, w)
            assert any(abs(y - j // w) <= 2 * r and abs(x - j % w) <= 2 * r for j in own), \
                f"key-point {i} differs with margin {margin[i]:.3e} >= 2 x score-map difference {tol:.3e}"


@pytest.mark.parametrize("size,conf", CASES)
def test_end_to_end_keypoints_descriptors_and_scores(size, conf, precision):
    img, d, _ = _oracle(size)
    bar = _bar(size)
    hip = _hip(size, conf, precision)
    sm_ref = d["score_map"][0, 0]
    idx_ref, idx_hip = _rule(sm_ref, conf), _rule(hip["score_map"], conf)  # (the latter IS the HIP set: the test above)
    diff = sorted(set(idx_ref.tolist()) ^ set(idx_hip.tolist()))
    print(f"{size} {conf}: {idx_hip.numel()} key-points, {len(diff)} differ from the restatement's")
    assert len(diff) <= 0.01 * idx_ref.numel()
    _audit(diff, hip["score_map"], sm_ref, idx_hip, idx_ref, conf)
    # descriptors and scores: the restatement's heads on ITS maps at the HIP key-points (trunc(p) cannot flip)
    ref = ALIKEDReference(_sd())
    kn = hip["keypoints_norm"]
    want = ref.desc_head(d["feature_map"][0], kn)
    derr = (hip["descriptors"] - want).abs().max().item()
    ks = F.grid_sample(sm_ref[None, None], kn.view(1, 1, -1, 2), mode="bilinear", align_corners=True)[0, 0, 0]
    serr = (hip["scores"] - ks).abs().max().item()
    print(f"{size} {conf}: descriptor error {derr:.2e}, score error {serr:.2e} (bar {bar:.1e})")
    assert (hip["descriptors"].norm(dim=1) - 1).abs().max().item() < 1e-5
    assert derr <= bar and serr <= bar


def test_mean_fallback_on_the_device(precision):
    """Seeded weights with the logits 3 lower: nothing passes 0.2, the mean of the score map takes the threshold's place.  The device
    mean is summed in double in a fixed order; candidates within 1e-6 of the mean may fall either way."""
    m = _plugin(-6.6)
    m.conf.update(CONFS["default"])
    out = m.forward_batched(image(96, 128, 3).cuda(), want_maps=True)
    sm = out["score_map"][0].cpu()
    n = int(out["num_keypoints"][0])
    assert sm.max().item() < 0.2 and int(out["status"]) == 0
    idx, branch = dkd_select(sm, 2, 0.2, -1)
    assert branch == "mean"
    kn, _ = dkd_refine(sm, idx, 2)
    kp = kn.new_tensor([127.0, 95.0]) * (kn + 1) / 2
    got = out["keypoints"][0, :n].cpu()
    sure = (sm.reshape(-1)[idx] - sm.double().mean().float()).abs() > 1e-6
    assert n > 10 and abs(n - idx.numel()) <= int((~sure).sum())
    if n == idx.numel():
        assert (got - kp).abs().max().item() <= 2e-3


@functools.lru_cache(maxsize=None)
def _flat_plugin():
    from imcui_hip.hloc.extractors.aliked import ALIKED

    sd = {k: v.clone() for k, v in _sd().items()}
    sd["score_head.6.weight"].zero_()  # the last layer of the score head (no bias): logit 0, score 0.5 at every pixel
    return ALIKED({"state_dict": sd}).eval().to("cuda:0")


@pytest.mark.parametrize("maxk", [300, 1500, -1])
def test_device_ties_at_the_cut_on_a_flat_score_map(precision, maxk):
    """The device's tie rule at the cut, driven on purpose: the score map is 0.5 everywhere, so every pixel is an NMS maximum and the
    (72 - 4) x (88 - 4) = 5712 pixels of the radius band all tie.  With more candidates than `max_num_keypoints` every one of them EQUALS
    the limit-th largest score: the first `limit` in row-major order stay (at 1500 the count of equal candidates is carried across a
    1024-candidate batch of the select kernel); -1 keeps all 5712.  72 x 88 = 6336 pixels are two compaction chunks, the second one
    partial.  Each case equals the restated rule on the same map."""
    H, W, r = 72, 88, 2
    m = _flat_plugin()
    m.conf.update(dict(max_num_keypoints=maxk, detection_threshold=0.2, nms_radius=r))
    out = m.forward_batched(image(H, W, 5).cuda(), want_maps=True, kcap=H * W)
    sm = out["score_map"][0].cpu()
    assert torch.equal(sm, torch.full((H, W), 0.5))
    ys, xs = torch.meshgrid(torch.arange(r, H - r), torch.arange(r, W - r), indexing="ij")
    band = (ys * W + xs).reshape(-1)
    want = band[:maxk] if maxk > 0 else band
    idx, branch = dkd_select(sm, r, 0.2, maxk)
    assert branch == "threshold" and torch.equal(idx, want)
    n = int(out["num_keypoints"][0])
    assert n == want.numel() and int(out["status"]) == 0
    kn, ks = dkd_refine(sm, idx, r)
    kp = kn.new_tensor([W - 1, H - 1]) * (kn + 1) / 2
    got = out["keypoints"][0].cpu()
    err = (got[:n] - kp).abs().max().item()
    print(f"flat map, max_num_keypoints {maxk}: {n} key-points, position error {err:.2e} px")
    assert err <= 2e-3  # a differing candidate would sit at least a pixel away from the rule's
    assert (out["keypoints_norm"][0, :n].cpu() - kn).abs().max().item() <= 2 * 2e-3 / (max(H, W) - 1)
    assert (out["scores"][0, :n].cpu() - ks).abs().max().item() <= 1e-6  # (a bilinear sample of a constant map)
    for k in ("keypoints", "keypoints_norm", "scores", "descriptors"):
        assert not out[k][0, n:].any(), k  # entries past the count are zero


# ------------------------------------------------------------------ determinism
def test_batch_independence_and_graph_replay_are_bitwise(precision):
    m = _plugin()
    m.conf.update(CONFS["default"])
    a, b, c = (image(480, 640, s).cuda() for s in (0, 7, 8))
    keys = ("keypoints", "scores", "descriptors", "num_keypoints")
    solo = m.forward_batched(a, kcap=6000)
    trio = m.forward_batched(torch.cat([b, a, c]), kcap=6000)
    assert int(solo["num_keypoints"][0]) > 1000
    for k in keys:
        assert torch.equal(solo[k][0], trio[k][1]), k
    from imcui_hip import backend

    batch = torch.cat([a, b])
    eager = m.forward_batched(batch, kcap=6000)
    table = {}
    with backend.workspace_owner(table):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.forward_batched(batch, kcap=6000)  # warm-up: allocates the graph-owned workspace
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = m.forward_batched(batch, kcap=6000)
    for _ in range(2):
        for v in cap.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(eager[k], cap[k]), k


# ------------------------------------------------------------------ plugin
def test_plugin_output_contract_and_capacity_retry(precision):
    m = _plugin()
    m.conf.update(CONFS["default"])
    imgs = torch.cat([image(472, 632, 1), image(472, 632, 4)]).cuda()
    with torch.no_grad():
        pred = m({"image": imgs})
    assert set(pred) == {"keypoints", "scores", "descriptors"} and all(isinstance(v, list) and len(v) == 2 for v in pred.values())
    for b in range(2):
        n = pred["keypoints"][b].shape[0]
        assert n > 100 and pred["keypoints"][b].shape == (n, 2) and pred["scores"][b].shape == (n,) and pred["descriptors"][b].shape == (128, n)
        assert all(pred[k][b].dtype == torch.float32 and pred[k][b].is_cuda for k in pred)
        kp = pred["keypoints"][b]
        assert kp[:, 0].min() >= 0 and kp[:, 0].max() <= 631 and kp[:, 1].min() >= 0 and kp[:, 1].max() <= 471
    grey = m({"image": imgs[:1, :1]})  # one channel is repeated to three
    again = m({"image": imgs[:1, :1].expand(-1, 3, -1, -1).contiguous()})
    assert torch.equal(grey["descriptors"][0], again["descriptors"][0])
    # a capacity that is too small: status bit 1, the first kcap key-points in row-major order; forward_checked retries
    small = m.forward_batched(imgs, kcap=50)
    assert int(small["status"]) & 2 and small["num_keypoints"].tolist() == [50, 50]
    assert torch.equal(small["keypoints"][0], pred["keypoints"][0][:50]) and torch.equal(small["descriptors"][1], pred["descriptors"][1][:, :50].t())
    real = m.forward_batched
    calls = []

    def starved(image, want_maps=False, kcap=None):
        calls.append(kcap)
        return real(image, want_maps=want_maps, kcap=50 if kcap is None else kcap)

    m.forward_batched = starved
    try:
        out, counts = m.forward_checked(imgs)
    finally:
        del m.forward_batched
    assert calls == [None, 472 * 632] and counts == [p.shape[0] for p in pred["keypoints"]]
    assert torch.equal(out["keypoints"][0, : counts[0]], pred["keypoints"][0])


# ------------------------------------------------------------------ shared-GEMM routes
def test_every_gemm_route_aliked_launches_is_covered(precision):
    """Reset the route counters, run ALIKED, and require every route launched to be one the float64 variants suite
    (tests/test_gpu_gemm_variants.py: covered_routes()) enters."""
    import test_gpu_gemm_variants as gv
    from imcui_hip import backend

    dev = torch.device("cuda:0")
    backend.gemm_route_reset(dev)
    m = _plugin()
    m.conf.update(CONFS["default"])
    m.forward_batched(torch.cat([image(480, 640, 0), image(480, 640, 7)]).cuda())
    m.forward_batched(image(96, 128, 3).cuda())  # few pixels: the small-tile variants of the deformable products
    torch.cuda.synchronize()
    launched = set(backend.gemm_route_counts(dev))
    assert launched, "ALIKED launched no shared GEMM"
    missing = launched - gv.covered_routes()
    print(f"precision {precision}: routes launched {sorted(backend.gemm_route_name(r) for r in launched)}")
    assert not missing, f"routes without a float64 case: {sorted(backend.gemm_route_name(r) for r in missing)}"
