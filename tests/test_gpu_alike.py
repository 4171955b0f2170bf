"""ALIKE on the MI355X (imcui/hloc/extractors/alike.py -> Shiaoming/ALIKE) against the CPU restatement (tests/alike_reference.py), in
both arithmetic modes: the dense score map and branch maps, the sparse descriptor head against the dense descriptor map at every
pixel, ALIKE's selection rule on the HIP score map (exact key-points in the exact order, the truncated descriptor pixel of upstream's
float32 round trip), the end-to-end key-point sets (equal, or every difference an audited round-off tie, at most 1 %), descriptors
and scores at the common key-points, ties on a flat map, the per-image mean fallback, zero key-points, the capacity retry, batch
independence, graph replay, the plugin's output contract and the routes of the shared GEMM.

Sizes: 32x40 (padded to 32x64: the 1/32 map is 1x2, the align_corners taps degenerate), 64x64, 100x150 (padding on both axes and the
crop), 160x224 (more than one GEMM tile at 1/8).  alike-t and alike-n everywhere, alike-s in the dense and end-to-end cases at 100x150.

Measured on one MI355X, both arithmetic modes, synthetic weights seed 0 (every line: profiles/alike_parity.txt): dense maps (score map, x4,
f2..f4) within 2.5e-06 of the restatement relative to the map's largest magnitude (bar 1e-4; the restatement's own spread over 1 / 8
threads is at most 9.7e-07); the probe's descriptors within 9.3e-07 of the dense descriptor map at every pixel; the rule on the HIP
score map: positions bitwise equal without sub_pixel (error 0.0e+00 px), within 1.5e-05 px with it, scores within 9.5e-07; 3 to
277 key-points per case read the neighbouring (truncated) pixel; end to end 0 key-points differ from the restatement's in any
case, descriptors within 6.5e-07 and scores within 1.5e-06 at the common key-points.
"""
from __future__ import annotations

import functools

import pytest
import torch

from alike_reference import ALIKEReference, banded_nms, describe, keypoints_from, select
from parity_utils import oracle_spread
from test_aliked_cpu import image

pytestmark = pytest.mark.gpu

SIZES = {"32x40": (32, 40, 11), "64x64": (64, 64, 1), "100x150": (100, 150, 2), "160x224": (160, 224, 3)}
BASE = dict(top_k=-1, detection_threshold=0.5, max_keypoints=5000, sub_pixel=False)
CONFS = {
    "default": BASE,
    "top50": {**BASE, "top_k": 50},
    "n50": {**BASE, "max_keypoints": 50},
    "mean": {**BASE, "detection_threshold": -1.0},
    "fallback": BASE,  # with the fallback weights
    "subpixel": {**BASE, "sub_pixel": True},
}
VARIANTS = ("alike-t", "alike-n")
DIMS = {"alike-t": (64, 64), "alike-s": (96, 96), "alike-n": (128, 128)}  # (c4, dim)


@functools.lru_cache(maxsize=None)
def _sd(variant: str, fallback: bool = False):
    from imcui_hip.synth_weights import alike_state_dict

    return alike_state_dict(variant, 0, fallback=fallback)


@functools.lru_cache(maxsize=None)
def _ref(variant: str, fallback: bool = False):
    return ALIKEReference(_sd(variant, fallback), variant)


@functools.lru_cache(maxsize=None)
def _oracle(variant: str, size: str, fallback: bool = False):
    """(image, the restatement's dense outputs, fp32 spread of those): computed once per (variant, size) and shared."""
    h, w, seed = SIZES[size]
    img = image(h, w, seed)
    spread, d = oracle_spread(lambda: _ref(variant, fallback).dense(img), threads=(1, 8))  # measured at every size the bar is used at
    return img, d, spread


def _bar(variant, size, fallback=False):
    return max(1e-4, 3 * _oracle(variant, size, fallback)[2])


@functools.lru_cache(maxsize=None)
def _plugin(variant: str, fallback: bool = False):
    from imcui_hip.hloc.extractors.alike import Alike

    return Alike({"model_name": variant, "state_dict": _sd(variant, fallback)}).eval().to("cuda:0")


@functools.lru_cache(maxsize=None)
def _hip(variant: str, size: str, conf: str, precision: int):
    """One HIP run with the debug maps, on the CPU: per-image slices of image 0."""
    fb = conf == "fallback"
    m = _plugin(variant, fb)
    m.conf.update(CONFS[conf])
    out = m.forward_batched(_oracle(variant, size, fb)[0].cuda(), want_maps=True)
    torch.cuda.synchronize()
    assert int(out["status"]) == 0
    n = int(out["num_keypoints"][0])
    o = {k: v[0].cpu() for k, v in out.items() if k not in ("status", "num_keypoints")}
    for k in ("keypoints", "scores", "descriptors"):
        assert not o[k][n:].any(), k  # entries past the count are zero
        o[k] = o[k][:n]
    o["n"] = n
    return o


# ------------------------------------------------------------------ dense maps
@pytest.mark.parametrize("variant,size", [(v, s) for v in VARIANTS for s in SIZES] + [("alike-s", "100x150")])
def test_dense_maps_match_the_restatement(variant, size, precision):
    d, bar = _oracle(variant, size)[1], _bar(variant, size)
    hip = _hip(variant, size, "default", precision)
    c4, dim = DIMS[variant]
    assert not hip["x4"][..., c4:].any()  # the channel padding of the stored maps stays zero
    maps = {"score_map": (hip["score_map"], d["score_map"][0, 0]), "x4": (hip["x4"][..., :c4].permute(2, 0, 1), d["x4"][0])}
    for k in ("f2", "f3", "f4"):
        maps[k] = (hip[k].permute(2, 0, 1), d[k][0])
    for name, (got, want) in maps.items():
        scale = max(want.abs().max().item(), 1e-30)
        err = (got - want).abs().max().item() / scale
        print(f"[alike] p{precision} {variant} {size} {name}: relative error {err:.2e} at scale {scale:.2f} (bar {bar:.1e}, oracle spread {_oracle(variant, size)[2]:.1e})")
        assert got.shape == want.shape and err <= bar, name


# ------------------------------------------------------------------ the sparse head is the dense head
@pytest.mark.parametrize("size", ["32x40", "100x150"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_sparse_descriptor_head_equals_the_dense_map_at_every_pixel(variant, size, precision):
    img, d, _ = _oracle(variant, size)
    h, w, _ = SIZES[size]
    m = _plugin(variant)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    xy = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)
    got = m._impl.desc_probe(m.packed, img.cuda(), xy).cpu()
    want = d["descriptor_map"][0].reshape(-1, h * w).t()
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"[alike] p{precision} {variant} {size} probe at {h * w} pixels: descriptor error {err:.2e} (bar {_bar(variant, size):.1e})")
    assert got.shape == want.shape and err <= _bar(variant, size)


# ------------------------------------------------------------------ selection
@pytest.mark.parametrize("conf", list(CONFS))
@pytest.mark.parametrize("size", ["100x150", "160x224"])  # (at 64x64 alike-n has fewer than 50 key-points: no cut to take)
@pytest.mark.parametrize("variant", VARIANTS)
def test_selection_is_the_rule_on_the_hip_score_map(variant, size, conf, precision):
    """The restated rule applied to the HIP score map returns exactly the HIP key-points in the HIP order (row-major, or descending
    score with ties at the lower index); without sub_pixel the positions are bitwise those of upstream's float32 round trip, so the
    truncated descriptor pixel is the restatement's at every key-point and the descriptor IS the head at that pixel (the probe
    entry); scores agree within 1e-6 (sampled from the same map), sub_pixel positions within 2e-3 px."""
    c = CONFS[conf]
    hip = _hip(variant, size, conf, precision)
    sm = hip["score_map"]
    h, w = sm.shape
    idx, branch, cut = select(sm, c)
    _, kp, ks, pix = keypoints_from(sm, idx, c["sub_pixel"])
    assert hip["n"] == idx.numel() and hip["n"] > 0, (hip["n"], idx.numel())
    assert branch == {"top50": "topk", "mean": "mean", "fallback": "mean"}.get(conf, "threshold")
    if conf in ("top50", "n50"):
        assert cut and hip["n"] == 50 and (hip["scores"][:-1] >= hip["scores"][1:] - 1e-6).all()  # the cut is taken: descending order
    perr = (hip["keypoints"] - kp).abs().max().item()
    serr = (hip["scores"] - ks).abs().max().item()
    ntr = int((pix != torch.stack([idx % w, idx // w], 1)).any(dim=1).sum())
    print(f"[alike] p{precision} {variant} {size} {conf}: {hip['n']} key-points ({branch}), position error {perr:.2e} px, score error {serr:.2e}, {ntr} truncated pixels")
    assert serr <= 1e-6
    if c["sub_pixel"]:
        assert perr <= 2e-3  # a differing candidate would sit at least a pixel away from the rule's
        return
    assert torch.equal(hip["keypoints"], kp)  # the same float32 operations in the same order
    assert torch.equal(hip["keypoints"].long(), pix)
    m = _plugin(variant, conf == "fallback")
    at_pix = m._impl.desc_probe(m.packed, _oracle(variant, size, conf == "fallback")[0].cuda(), pix).cpu()
    assert torch.equal(hip["descriptors"], at_pix)  # read at the truncated pixel, not at the candidate


def _audit(diff, sm_hip, sm_ref, thrs, cuts, r=2):
    """As tests/test_gpu_aliked.py::_audit: every key-point in one set but not the other must be a round-off tie, i.e. the margin
    that decides it -- against the threshold (0.5 or the mean of either map), against the cut of either map, or against a pixel of
    its own NMS window -- lies below twice the MEASURED difference of the two score maps.  simple_nms iterates, so a flipped maximum
    can free or suppress a second one up to 2r away: such a key-point passes only next to one that passed on its own margin.  (The
    band is geometry: no margin.)"""
    h, w = sm_ref.shape
    tol = 2 * (sm_hip - sm_ref).abs().max().item()
    own, margin = set(), {}
    for i in diff:
        y, x = divmod(i, w)
        v = sm_ref[y, x].item()
        y0, x0 = max(0, y - r), max(0, x - r)
        win = sm_ref[y0 : y + r + 1, x0 : x + r + 1].clone()
        win[y - y0, x - x0] = float("inf")  # the pixel itself
        margin[i] = min([(win - v).abs().min().item()] + [abs(v - t) for t in list(thrs) + list(cuts)])
        if margin[i] < tol:
            own.add(i)
    for i in diff:
        if i not in own:
            y, x = divmod(i, w)
            assert any(abs(y - j // w) <= 2 * r and abs(x - j % w) <= 2 * r for j in own), \
                f"key-point {i} differs with margin {margin[i]:.3e} >= 2 x score-map difference {tol:.3e}"


E2E = [(v, s, "default") for v in VARIANTS for s in SIZES] + [(v, "100x150", c) for v in VARIANTS for c in ("top50", "n50", "mean", "fallback", "subpixel")]
E2E += [("alike-s", "100x150", "default")]


@pytest.mark.parametrize("variant,size,conf", E2E)
def test_end_to_end_keypoints_descriptors_and_scores(variant, size, conf, precision):
    c, fb = CONFS[conf], conf == "fallback"
    img, d, _ = _oracle(variant, size, fb)
    bar = _bar(variant, size, fb)
    hip = _hip(variant, size, conf, precision)
    sm_ref, sm_hip = d["score_map"][0, 0], hip["score_map"]
    h, w = sm_ref.shape
    idx_ref, branch, _ = select(sm_ref, c)
    idx_hip, _, _ = select(sm_hip, c)  # (IS the HIP set: the test above)
    diff = sorted(set(idx_ref.tolist()) ^ set(idx_hip.tolist()))
    print(f"[alike] p{precision} {variant} {size} {conf}: {idx_hip.numel()} key-points, {len(diff)} differ from the restatement's")
    assert len(diff) <= 0.01 * idx_ref.numel()
    thrs = [0.5] if branch == "threshold" else ([sm_ref.mean().item(), sm_hip.mean().item()] if branch == "mean" else [0.0])
    limit = min(x for x in (c["top_k"], c["max_keypoints"]) if x > 0)
    cuts = [s.reshape(-1)[i].min().item() for s, i in ((sm_ref, idx_ref), (sm_hip, idx_hip)) if i.numel() == limit]
    _audit(diff, sm_hip, sm_ref, thrs, cuts)
    # descriptors and scores at the common key-points: the restatement on ITS maps
    _, kp_ref, ks_ref, _ = keypoints_from(sm_ref, idx_ref, c["sub_pixel"])
    de_ref = describe(d["descriptor_map"][0], kp_ref, c["sub_pixel"])
    pos_ref = {int(i): j for j, i in enumerate(idx_ref.tolist())}
    common = [(j, pos_ref[int(i)]) for j, i in enumerate(idx_hip.tolist()) if int(i) in pos_ref]
    jh, jr = torch.tensor([a for a, _ in common]), torch.tensor([b for _, b in common])
    derr = (hip["descriptors"][jh] - de_ref[jr]).abs().max().item()
    serr = (hip["scores"][jh] - ks_ref[jr]).abs().max().item()
    print(f"[alike] p{precision} {variant} {size} {conf}: descriptor error {derr:.2e}, score error {serr:.2e} (bar {bar:.1e})")
    assert (hip["descriptors"].norm(dim=1) - 1).abs().max().item() < 1e-5
    assert derr <= bar and serr <= bar
    if c["sub_pixel"]:  # refined on two maps that differ by the bar: the soft-argmax (temperature 0.1) moves by at most 2 r |d score| / 0.1
        assert (hip["keypoints"][jh] - kp_ref[jr]).abs().max().item() <= 40 * (sm_hip - sm_ref).abs().max().item() + 2e-3


# ------------------------------------------------------------------ other cases
@functools.lru_cache(maxsize=None)
def _flat_plugin():
    from imcui_hip.hloc.extractors.alike import Alike

    sd = {k: v.clone() for k, v in _sd("alike-t").items()}
    sd["convhead2.weight"][64].zero_()  # the score row: logit 0, score 0.5 at every pixel
    return Alike({"model_name": "alike-t", "state_dict": sd}).eval().to("cuda:0")


@pytest.mark.parametrize("limit", [300, 1500])
def test_device_ties_at_the_cut_on_a_flat_score_map(precision, limit):
    """The score map is 0.5 everywhere, so every pixel is an NMS maximum and the (72 - 5) x (88 - 5) = 5561 pixels of ALIKE's band all
    tie above the 0.2 threshold.  Every candidate EQUALS the limit-th largest score: the first `limit` in row-major order stay (at 1500 the
    count of equal candidates is carried across a 1024-candidate batch of the cut kernel), and the descending order of equal scores is
    the row-major one.  72 x 88 = 6336 pixels are two compaction chunks, the second one partial."""
    H, W = 72, 88
    m = _flat_plugin()
    c = {**BASE, "detection_threshold": 0.2, "max_keypoints": limit}
    m.conf.update(c)
    out = m.forward_batched(image(H, W, 5).cuda(), want_maps=True, kcap=H * W)
    sm = out["score_map"][0].cpu()
    assert torch.equal(sm, torch.full((H, W), 0.5))
    ys, xs = torch.meshgrid(torch.arange(3, H - 2), torch.arange(3, W - 2), indexing="ij")
    want = (ys * W + xs).reshape(-1)[:limit]
    idx, branch, cut = select(sm, c)
    assert branch == "threshold" and cut and torch.equal(idx, want)
    n = int(out["num_keypoints"][0])
    assert n == limit and int(out["status"]) == 0
    _, kp, ks, _ = keypoints_from(sm, idx, False)
    assert torch.equal(out["keypoints"][0, :n].cpu(), kp)
    assert (out["scores"][0, :n].cpu() - ks).abs().max().item() <= 1e-6  # (a bilinear sample of a constant map)
    for k in ("keypoints", "scores", "descriptors"):
        assert not out[k][0, n:].any(), k  # entries past the count are zero


def test_zero_keypoints_and_the_capacity_retry(precision):
    """The flat map again.  At the default threshold nothing is above 0.5 and nothing is above the mean (0.5, summed in double): zero
    key-points is a valid result.  At threshold 0.2 without a limit all 5561 band pixels are key-points, more than the NMS bound the
    default capacity is sized by: status bit 1 and the first kcap in row-major order; the plugin retries with room for every pixel."""
    H, W = 72, 88
    m = _flat_plugin()
    img = image(H, W, 5).cuda()
    m.conf.update(BASE)
    out, counts = m.forward_checked(img)
    assert counts == [0] and not out["keypoints"].any() and not out["descriptors"].any()
    pred = m({"image": img})
    assert pred["keypoints"].shape == (1, 0, 2) and pred["scores"].shape == (1, 0) and pred["descriptors"].shape == (1, 64, 0)
    m.conf.update({**BASE, "detection_threshold": 0.2, "max_keypoints": -1})
    small = m.forward_batched(img)
    kcap = small["keypoints"].shape[1]
    assert kcap == 24 * 30 and int(small["status"]) & 2 and small["num_keypoints"].tolist() == [kcap]
    out, counts = m.forward_checked(img)
    assert counts == [(H - 5) * (W - 5)] and int(out["status"]) == 0
    assert torch.equal(small["keypoints"][0], out["keypoints"][0, :kcap]) and torch.equal(small["descriptors"][0], out["descriptors"][0, :kcap])


def test_mean_fallback_is_taken_per_image_inside_a_batch(precision):
    """Two images, one network: the logit shift is placed between the highest logits of the two (from the restatement in float64), so
    image A has nothing above 0.5 and takes the mean of ITS score map while image B keeps the threshold.  Each image of the batch equals
    the rule on its own HIP score map."""
    from imcui_hip.hloc.extractors.alike import Alike

    variant, (h, w) = "alike-t", (64, 96)
    imgs = torch.cat([image(h, w, 21), image(h, w, 22)])
    sd = {k: v.clone() for k, v in _sd(variant).items()}
    logit = torch.logit(ALIKEReference(sd, variant).double().dense(imgs.double())["score_map"][:, 0])
    top = sorted(logit[b][banded_nms(torch.sigmoid(logit[b])) > 0].max().item() for b in range(2))  # highest candidate logit per image
    assert top[1] - top[0] > 0.1, top
    sd["convhead2.weight"][64, 15, 0, 0] -= (top[0] + top[1]) / 2  # the constant channel: dq - 1 = 15
    m = Alike({"model_name": variant, "state_dict": sd}).eval().to("cuda:0")
    m.conf.update(BASE)
    out = m.forward_batched(imgs.cuda(), want_maps=True)
    branches = []
    for b in range(2):
        sm = out["score_map"][b].cpu()
        idx, branch, _ = select(sm, BASE)
        branches.append(branch)
        n = int(out["num_keypoints"][b])
        got = out["keypoints"][b, :n].cpu()
        assert n > 0
        if branch == "threshold":  # decided against the constant 0.5 on the same map: exact
            assert torch.equal(got, keypoints_from(sm, idx, False)[1])
            continue
        # the mean route: the device mean is a double sum in another order, so a candidate within 1e-6 of the mean may fall either way;
        # every other candidate of the rule is a device key-point, bit for bit and in order, and the device adds nothing but such near-ties
        mean = sm.double().mean().float()
        nms = banded_nms(sm).reshape(-1)
        sure = idx[(nms[idx] - mean).abs() > 1e-6]
        allowed = set(torch.nonzero(nms > mean - 1e-6)[:, 0].tolist())
        flat = got.round().long()
        flat = flat[:, 1] * sm.shape[1] + flat[:, 0]
        assert set(flat.tolist()) <= allowed and set(sure.tolist()) <= set(flat.tolist())
        keep = torch.isin(flat, sure)
        assert torch.equal(got[keep], keypoints_from(sm, sure, False)[1])
    assert sorted(branches) == ["mean", "threshold"], branches


# ------------------------------------------------------------------ determinism
@pytest.mark.parametrize("variant", VARIANTS)
def test_batch_independence_and_graph_replay_are_bitwise(variant, precision):
    m = _plugin(variant)
    m.conf.update(BASE)
    a, b, c = (image(100, 150, s).cuda() for s in (2, 7, 8))
    keys = ("keypoints", "scores", "descriptors", "num_keypoints")
    solo = m.forward_batched(a, kcap=600)
    trio = m.forward_batched(torch.cat([b, a, c]), kcap=600)
    assert int(solo["num_keypoints"][0]) > 20
    for k in keys:
        assert torch.equal(solo[k][0], trio[k][1]), k
    from imcui_hip import backend

    batch = torch.cat([a, b])
    eager = m.forward_batched(batch, kcap=600)
    table = {}
    with backend.workspace_owner(table):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.forward_batched(batch, kcap=600)  # warm-up: allocates the graph-owned workspace
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = m.forward_batched(batch, kcap=600)
    for _ in range(2):
        for v in cap.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(eager[k], cap[k]), k


# ------------------------------------------------------------------ plugin
@pytest.mark.parametrize("variant", VARIANTS)
def test_plugin_output_contract(variant, precision):
    m = _plugin(variant)
    m.conf.update(BASE)
    img = image(100, 150, 2).cuda()
    with torch.no_grad():
        pred = m({"image": img})
    dim = DIMS[variant][1]
    n = pred["keypoints"].shape[1]
    assert set(pred) == {"keypoints", "scores", "descriptors"}
    assert n > 20 and pred["keypoints"].shape == (1, n, 2) and pred["scores"].shape == (1, n) and pred["descriptors"].shape == (1, dim, n)
    assert all(v.dtype == torch.float32 and v.is_cuda for v in pred.values())
    kp = pred["keypoints"][0]
    assert kp[:, 0].min() >= 3 - 1e-3 and kp[:, 0].max() <= 147 + 1e-3 and kp[:, 1].min() >= 3 - 1e-3 and kp[:, 1].max() <= 97 + 1e-3  # the band
    ref = _ref(variant).forward(img.cpu(), BASE)
    assert abs(n - ref["keypoints"][0].shape[0]) <= max(1, n // 100)
    with pytest.raises(ValueError, match="RGB"):
        m({"image": img[:, :1]})


# ------------------------------------------------------------------ shared-GEMM routes
def test_every_gemm_route_alike_launches_is_covered(precision):
    """Reset the route counters, run ALIKE, and require every route launched to be one the float64 variants suite
    (tests/test_gpu_gemm_variants.py: covered_routes()) enters."""
    import test_gpu_gemm_variants as gv
    from imcui_hip import backend

    dev = torch.device("cuda:0")
    backend.gemm_route_reset(dev)
    for variant in VARIANTS + ("alike-s",):
        m = _plugin(variant)
        m.conf.update(BASE)
        m.forward_batched(torch.cat([image(160, 224, 3), image(160, 224, 7)]).cuda())
        m.forward_batched(image(32, 40, 11).cuda())  # two rows at 1/32: the small end of the tiles
    torch.cuda.synchronize()
    launched = set(backend.gemm_route_counts(dev))
    assert launched, "ALIKE launched no shared GEMM"
    missing = launched - gv.covered_routes()
    print(f"[alike] p{precision} routes launched {sorted(backend.gemm_route_name(r) for r in launched)}")
    assert not missing, f"routes without a float64 case: {sorted(backend.gemm_route_name(r) for r in missing)}"
