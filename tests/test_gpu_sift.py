"""SIFT on the HIP backend against the float64 restatement (tests/sift_reference.py), stage by stage.

OpenCV is not installed where these tests run, so the detector is parity-unpinned like DISK and ALIKED: the binding requirement is
device == restatement.  Bars: a relative bar is max(1e-4, 3 x spread) with spread = the float32 restatement's own deviation from the
float64 one for that quantity at that size (measured here, printed); the pyramid's floor is 64 x 2^-24 (one rounding per pass on the
longest chain of about 30 blurs x 2 passes).  Discrete decisions are audited as in tests/test_gpu_aliked.py: a differing decision passes
only if its traced margin is below 2 x the largest device-vs-float64 difference of that quantity on the common key-points.
Angles are compared in degrees against bar x 360 (a bar relative to the angle itself would be meaningless at the 0 / 360 wrap).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import sift_reference as R

pytestmark = pytest.mark.gpu

SIZES = {"97x131": (97, 131, 0), "240x320": (240, 320, 1)}
LAYERS, CONTRAST, EDGE = 4, 0.0066667, 10.0
FLOOR = 64 * 2.0**-24


def _img(size: str) -> np.ndarray:
    h, w, seed = SIZES[size]
    return R.seeded_image(h, w, seed)[None]


@functools.lru_cache(maxsize=None)
def _plugin(**conf):
    from imcui_hip.hloc.extractors.sift import SIFT

    return SIFT(dict(conf)).eval().to("cuda:0")


@functools.lru_cache(maxsize=None)
def _hip(size: str, rootsift: bool = False, **conf):
    """One debug run of image `size`, on the CPU as numpy; the pyramid as a list of [L,h,w]."""
    m = _plugin(rootsift=rootsift, **conf)
    out = m.forward_batched(torch.from_numpy(_img(size))[None].cuda(), debug=True)
    torch.cuda.synchronize()
    assert int(out["status"]) == 0
    o = {k: (v[0].cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items() if k not in ("status", "pyramid")}
    o["pyramid"] = [p[0].cpu().numpy() for p in out["pyramid"]]
    o["ncand"], o["ntab"], o["n"] = (int(v) for v in o["counts"])
    assert o["n"] == int(out["num_keypoints"][0])
    return o


@functools.lru_cache(maxsize=None)
def _ref_pyramids(size: str):
    u8 = R.to_u8(_img(size))
    p64, p32 = R.pyramid(u8, LAYERS, np.float64), R.pyramid(u8, LAYERS, np.float32)
    spread = max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(p32, p64)) / 255.0
    return p64, spread


@functools.lru_cache(maxsize=None)
def _detect_on_hip_pyramid(size: str):
    """`detect` in float64 and float32 on the pyramid read back from the device."""
    pyr = _hip(size)["pyramid"]
    return R.detect(pyr, LAYERS, CONTRAST, EDGE, np.float64), R.detect(pyr, LAYERS, CONTRAST, EDGE, np.float32)


def _decode(size: str, idx: np.ndarray) -> np.ndarray:
    """Search-space index of the device -> (o, l, r, c)."""
    out, off = [], 0
    shapes = [p.shape[1:] for p in _hip(size)["pyramid"]]
    offs = np.cumsum([0] + [LAYERS * h * w for h, w in shapes])
    for i in idx.astype(np.int64):
        o = int(np.searchsorted(offs, i, side="right") - 1)
        h, w = shapes[o]
        q = i - offs[o]
        out.append((o, 1 + q // (h * w), (q % (h * w)) // w, q % w))
    return np.array(out, dtype=int).reshape(-1, 4)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30))) if len(a) else 0.0


# ------------------------------------------------------------------ a. pyramid
@pytest.mark.parametrize("size", list(SIZES))
def test_pyramid_matches_the_restatement(size):
    p64, spread = _ref_pyramids(size)
    got = _hip(size)["pyramid"]
    assert len(got) == len(p64) == R.num_octaves(*SIZES[size][:2])
    bar = max(FLOOR, 3 * spread)
    worst = 0.0
    for o, (g, r) in enumerate(zip(got, p64)):
        assert g.shape == r.shape, (o, g.shape, r.shape)
        worst = max(worst, float(np.abs(g - r).max()) / 255.0)
    print(f"{size} pyramid: {len(got)} octaves down to {got[-1].shape[1:]}, max error / 255 = {worst:.2e} (bar {bar:.2e}, float32 restatement spread {spread:.2e})")
    assert worst <= bar


# ------------------------------------------------------------------ b. detection is the rule on the HIP pyramid
@pytest.mark.parametrize("size", list(SIZES))
def test_detection_is_the_rule_on_the_hip_pyramid(size):
    hip = _hip(size)
    d64, d32 = _detect_on_hip_pyramid(size)
    n = hip["ncand"]
    assert n == len(d64["extrema"]) and np.array_equal(_decode(size, hip["extrema"][:n]), d64["extrema"])  # identical fp32 comparisons
    rec = hip["refined"][:n]
    v_hip = rec[:, 0] > 0
    v_ref = np.array([q["valid"] for q in d64["refined"]], bool)
    v_32 = np.array([q["valid"] for q in d32["refined"]], bool)
    common = np.nonzero(v_hip & v_ref)[0]
    assert len(common) > 100
    f = lambda key, idx, recs=d64["refined"]: np.array([float(recs[i][key]) for i in idx])  # noqa: E731
    # same final pixel on the common key-points, then the continuous quantities
    for col, key in ((2, "l"), (3, "r"), (4, "c")):
        assert np.array_equal(rec[common, col], f(key, common)), key
    d_off = max(np.abs(rec[common, col] - f(key, common)).max() for col, key in ((5, "xc"), (6, "xr"), (7, "xi")))
    d_contr = np.abs(np.abs(rec[common, 8]) - np.abs(f("contr", common))).max() * LAYERS
    d_edge = max(np.abs(rec[common, 12] - f("edge_q", common)).max(), np.abs(rec[common, 13] - f("det", common)).max() * (EDGE + 1) ** 2)
    diff = np.nonzero(v_hip != v_ref)[0]
    for i in diff:  # a differing key-point: one of its decisions lies within twice the measured arithmetic difference of that quantity
        m = d64["refined"][i]["margins"]
        assert m["offset"] < 2 * d_off or m["contrast"] < 2 * d_contr or m["edge"] < 2 * d_edge, (i, m, d_off, d_contr, d_edge)
    assert len(diff) <= 0.01 * max(v_ref.sum(), 1)
    c32 = np.nonzero(v_32 & v_ref)[0]
    s_resp = _rel(np.abs(f("contr", c32, d32["refined"])), np.abs(f("contr", c32)))
    s_size = _rel(f("size", c32, d32["refined"]), f("size", c32))
    e_pos = max(np.abs(rec[common, 10] - f("x", common)).max(), np.abs(rec[common, 11] - f("y", common)).max()) * 0.5  # image pixels
    e_resp, e_size = _rel(np.abs(rec[common, 8]), np.abs(f("contr", common))), _rel(rec[common, 9], f("size", common))
    print(f"{size} detection: {n} extrema exact, {int(v_hip.sum())} / {int(v_ref.sum())} refined (device / float64), {len(diff)} differ (all audited; "
          f"float32 restatement differs on {int((v_32 != v_ref).sum())}); position {e_pos:.2e} px, response {e_resp:.2e} (spread {s_resp:.2e}), "
          f"size {e_size:.2e} (spread {s_size:.2e}); offsets differ by {d_off:.2e}")  # fmt: skip
    assert e_pos <= 2e-3
    assert e_resp <= max(1e-4, 3 * s_resp) and e_size <= max(1e-4, 3 * s_size)


# ------------------------------------------------------------------ c. orientations at the device's key-points
def _ang_diff(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.minimum(d, 360.0 - d)


@pytest.mark.parametrize("size", list(SIZES))
def test_orientations_at_the_device_keypoints(size):
    hip = _hip(size)
    pyr, rec, table = hip["pyramid"], hip["refined"][: hip["ncand"]], hip["table"][: hip["ntab"]]
    ptr, worst_hist, worst_ang, spread_ang, audited, peaks_total = 0, 0.0, 0.0, 0.0, 0, 0
    pending = []
    for j in np.nonzero(rec[:, 0] > 0)[0]:
        o, l, r, c = (int(v) for v in rec[j, 1:5])
        scl = np.float32(rec[j, 9]) * np.float32(0.5) / np.float32(1 << o)
        h64 = R.orientation_hist(pyr[o][l], r, c, scl, np.float64)
        h32 = R.orientation_hist(pyr[o][l], r, c, scl, np.float32)
        hd = hip["hist"][j]
        scale = max(float(h64.max()), 1e-30)
        bins_d, ang_d, _ = R.hist_peaks(hd, np.float32)  # the device's own decisions on its own histogram ...
        rows = table[ptr : ptr + len(bins_d)]  # ... are the rows it wrote, in bin order
        assert len(rows) == len(bins_d) and np.array_equal(rows[:, :4], np.tile(rec[j, 1:5], (len(rows), 1))), j
        assert np.array_equal(rows[:, 4:7], np.tile(rec[j, 5:8], (len(rows), 1))) and (_ang_diff(rows[:, 9], ang_d) < 1e-3).all(), j
        ptr += len(bins_d)
        bins_r, ang_r, margins = R.hist_peaks(h64, np.float64)
        bins_s, ang_s, _ = R.hist_peaks(h32, np.float32)
        peaks_total += len(bins_r)
        if np.array_equal(bins_s, bins_r) and len(bins_r):
            spread_ang = max(spread_ang, float(_ang_diff(ang_s, ang_r).max()))
        if np.array_equal(bins_d, bins_r):  # the audit's yardstick comes from the key-points whose peaks agree
            worst_hist = max(worst_hist, float(np.abs(hd - h64).max()) / scale)
            if len(bins_r):
                worst_ang = max(worst_ang, float(_ang_diff(rows[:, 9], ang_r).max()))
        else:
            pending.append((j, sorted(set(bins_d.tolist()) ^ set(bins_r.tolist())), margins / scale))
    assert ptr == hip["ntab"]
    for j, bins, margins in pending:  # peak against 0.8 max and the two neighbour comparisons, relative to the histogram's maximum
        for b in bins:
            assert margins[b] < 2 * worst_hist, (j, b, margins[b], worst_hist)
            audited += 1
    bar = max(1e-4, 3 * spread_ang / 360.0) * 360.0
    print(f"{size} orientations: {peaks_total} peaks, smoothed histograms within {worst_hist:.2e} of their maximum, {audited} differing peaks (audited), "
          f"angles within {worst_ang:.2e} deg (bar {bar:.2e}, float32 restatement spread {spread_ang:.2e} deg)")  # fmt: skip
    assert audited <= 0.01 * peaks_total
    assert worst_ang <= bar


# ------------------------------------------------------------------ d. descriptors at the device's key-points and angles
@pytest.mark.parametrize("size", list(SIZES))
def test_descriptors_at_the_device_keypoints(size):
    hip = _hip(size)
    table = hip["table"][: hip["ntab"]]
    sel = R.wrapper_stages(table, SIZES[size][:2], 4096, 0, 4096)
    n = hip["n"]
    assert n == len(sel["keep"]) and n > 100
    raw_d, q_d = hip["desc_raw"][:n], hip["descriptors"][:n]
    worst, spread, skipped, pending = 0.0, 0.0, 0, []
    for k, row in enumerate(table[sel["keep"]]):
        o, l = int(row[0]), int(row[1])
        ref = R.describe(hip["pyramid"][o][l], o, row[10], row[11], row[8], row[9], np.float64)
        if ref["round_margin"] < 1e-4:
            skipped += 1
            continue
        r32 = R.describe(hip["pyramid"][o][l], o, row[10], row[11], row[8], row[9], np.float32)
        spread = max(spread, float(np.abs(r32["raw"] - ref["raw"]).max()) / 512.0)
        worst = max(worst, float(np.abs(raw_d[k] - ref["raw"]).max()))
        pending.append((k, ref))
    bar = 512 * max(1e-4, 3 * spread)
    flips = 0
    for k, ref in pending:
        bad = np.nonzero(q_d[k] != ref["quant"])[0]
        for e in bad:  # only an element whose float64 value sits on a rounding boundary may round the other way
            assert abs(abs(ref["raw"][e] - np.floor(ref["raw"][e])) - 0.5) < 2 * worst and abs(q_d[k][e] - ref["quant"][e]) == 1, (k, e, ref["raw"][e], q_d[k][e])
            flips += 1
    print(f"{size} descriptors: {n} key-points ({skipped} skipped: a cvRound argument within 1e-4 of a half-integer), unquantised within {worst:.2e} "
          f"(bar {bar:.2e}, float32 restatement spread {spread * 512:.2e}), {flips} of {128 * len(pending)} integers on a rounding boundary")  # fmt: skip
    assert skipped <= 0.01 * n
    assert worst <= bar
    rs = _hip(size, rootsift=True)
    assert rs["n"] == n
    rows = rs["descriptors"][:n]
    assert np.abs(np.linalg.norm(rows.astype(np.float64), axis=1) - 1.0).max() < 1e-5
    assert np.abs(rows - R.rootsift(q_d.astype(np.float64))).max() < 1e-6
    assert np.array_equal(rs["keypoints"][:n], hip["keypoints"][:n])


# ------------------------------------------------------------------ e. wrapper stages on the device
@pytest.mark.parametrize("size,conf", [("240x320", (("max_keypoints", 300),)), ("240x320", (("nms_radius", 3),)), ("240x320", (("nms_radius", None),)),
                                       ("97x131", (("nms_radius", 3), ("max_keypoints", 50)))])  # fmt: skip
def test_wrapper_stages_on_the_device(size, conf):
    hip = _hip(size, **dict(conf))
    c = {"nms_radius": 0, "max_keypoints": 4096, **dict(conf)}
    table = hip["table"][: hip["ntab"]]
    sel = R.wrapper_stages(table, SIZES[size][:2], c["max_keypoints"], c["nms_radius"], c["max_keypoints"])
    n = hip["n"]
    print(f"{size} {dict(conf)}: {hip['ntab']} table rows -> {n} key-points (restatement {len(sel['keep'])}, tie at the cut: {sel['tie_at_cut']})")
    assert n == len(sel["keep"]) and n > 20
    if "max_keypoints" in c and c["max_keypoints"] < 4096:
        assert n <= c["max_keypoints"] < hip["ntab"]  # retainBest cuts the table first; the per-pixel filter may then leave fewer
    same = np.ones(n, bool)
    for k in ("keypoints", "scores", "scales", "oris"):
        same &= (hip[k][:n] == sel[k]).reshape(n, -1).all(1)
    if sel["tie_at_cut"]:  # equal scores exactly at the cut may resolve either way
        cut = np.sort(sel["scores"])[0]
        assert (same | (hip["scores"][:n] == cut)).all()
    else:
        assert same.all()


# ------------------------------------------------------------------ f. ground truth without the restatement
@functools.lru_cache(maxsize=None)
def _shift_reference():
    a, b = R.shift_pair(240, 320)
    ra, rb = R.extract(a), R.extract(b)
    return R.shift_consistency(ra, rb, (240, 320), R.mutual_nn(ra["descriptors"], rb["descriptors"]))


def test_shifted_crops_give_the_same_keypoints():
    from imcui_hip.hloc.matchers.nearest_neighbor import NearestNeighbor

    a, b = R.shift_pair(240, 320)
    m = _plugin()
    out, counts = m.forward_checked(torch.from_numpy(np.stack([a, b])).cuda())
    res = [{k: out[k][i, :n].cpu().numpy() for k in ("keypoints", "scales", "oris", "descriptors")} for i, n in enumerate(counts)]
    nn = NearestNeighbor({}).eval().to("cuda:0")
    m01 = nn({"descriptors0": out["descriptors"][0:1, : counts[0]].permute(0, 2, 1).contiguous(), "descriptors1": out["descriptors"][1:2, : counts[1]].permute(0, 2, 1).contiguous()})
    got = R.shift_consistency(res[0], res[1], (240, 320), m01["matches0"][0].cpu().numpy())
    ref = _shift_reference()
    print(f"shifted crops: device {got}, restatement {ref}")
    assert got["interior"] > 100 and got["share"] >= ref["share"] - 0.01
    assert got["share"] > 0.9 and got["matched_share"] > 0.9 and got["matched_share"] >= ref["matched_share"] - 0.01


# ------------------------------------------------------------------ g. bitwise checks
def test_batch_independence_and_graph_replay_are_bitwise():
    from imcui_hip import backend

    m = _plugin()
    a, b, c = (torch.from_numpy(R.seeded_image(240, 320, s)[None, None]).cuda() for s in (1, 7, 8))
    keys = ("keypoints", "scores", "scales", "oris", "descriptors")
    solo = m.forward_batched(a)
    trio = m.forward_batched(torch.cat([b, a, c]))
    n = int(solo["num_keypoints"][0])
    assert n > 500 and n == int(trio["num_keypoints"][1]) and int(solo["status"]) == 0 and int(trio["status"]) == 0
    for k in keys:
        assert torch.equal(solo[k][0, :n], trio[k][1, :n]), k
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
    counts = eager["num_keypoints"].tolist()
    for _ in range(2):
        for v in cap.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert cap["num_keypoints"].tolist() == counts and int(cap["status"]) == 0
        for k in keys:
            for i, cnt in enumerate(counts):
                assert torch.equal(eager[k][i, :cnt], cap[k][i, :cnt]), k


# ------------------------------------------------------------------ h. plugin contract
def test_plugin_output_contract():
    m = _plugin()
    img = torch.from_numpy(_img("240x320"))[None].cuda()
    with torch.no_grad():
        pred = m({"image": img})
    n = pred["keypoints"].shape[1]
    assert set(pred) == {"keypoints", "scales", "oris", "scores", "keypoint_scores", "descriptors"} and n > 500
    assert pred["keypoints"].shape == (1, n, 2) and pred["descriptors"].shape == (1, 128, n)
    assert all(pred[k].shape == (1, n) for k in ("scales", "oris", "scores", "keypoint_scores"))
    assert all(v.dtype == torch.float32 and v.is_cuda for v in pred.values())
    kp = pred["keypoints"][0]
    assert kp[:, 0].min() > 0 and kp[:, 0].max() < 320 and kp[:, 1].min() > 0 and kp[:, 1].max() < 240
    assert (pred["oris"] >= 0).all() and (pred["oris"] < 2 * np.pi + 1e-6).all() and (pred["scales"] > 1.6).all() and (pred["scores"] > 0).all()
    assert ((pred["descriptors"][0].norm(dim=0) - 1).abs() < 1e-5).all()
    # a 3-channel image goes through kornia's rgb_to_grayscale in float32: the same result as that gray fed directly
    rgb = torch.from_numpy(np.stack([R.seeded_image(240, 320, s) for s in (1, 2, 3)])[None])
    gray = (0.299 * rgb[:, 0:1] + 0.587 * rgb[:, 1:2] + 0.114 * rgb[:, 2:3]).float()
    with torch.no_grad():
        p3, p1 = m({"image": rgb.cuda()}), m({"image": gray.cuda()})
    assert all(torch.equal(p3[k], p1[k]) for k in p3)
    p3 = m({"image": img.expand(-1, 3, -1, -1).contiguous()})  # a 3-channel copy of gray
    g1 = m({"image": (0.299 * img.cpu() + 0.587 * img.cpu() + 0.114 * img.cpu()).cuda()})
    assert all(torch.equal(p3[k], g1[k]) for k in p3)


def test_capacity_retry_unequal_counts_refusals_and_blank_image():
    from imcui_hip import ImcuiHipError

    m = _plugin()
    img = torch.from_numpy(_img("240x320"))[None].cuda()
    full, counts = m.forward_checked(img)
    n = counts[0]
    small = m.forward_batched(img, kcap=100)
    assert int(small["status"]) == 1 and int(small["num_keypoints"][0]) == 100 and int(small["counts"][0, 2]) == n
    tiny = m.forward_batched(img, ccap=200)
    assert int(tiny["status"]) & 2 and int(tiny["counts"][0, 0]) == int(full["counts"][0, 0]) > 200
    out, c2 = m.forward_checked(img, kcap=100, ccap=200)  # both bits, retried with the capacities the counts ask for
    assert c2 == counts and int(out["status"]) == 0
    for k in ("keypoints", "scores", "scales", "oris", "descriptors"):
        assert torch.equal(out[k][0, :n], full[k][0, :n]), k
    two = torch.cat([img, torch.from_numpy(R.seeded_image(240, 320, 5)[None, None]).cuda()])
    with pytest.raises(ValueError, match="unequal counts"):
        m({"image": two})
    with pytest.raises(ImcuiHipError, match="image_size"):
        m({"image": img, "image_size": torch.tensor([[320, 240]])})
    blank = m({"image": torch.full((1, 1, 97, 131), 0.5).cuda()})
    assert blank["keypoints"].shape == (1, 0, 2) and blank["descriptors"].shape == (1, 128, 0) and blank["scores"].shape == (1, 0)
    from imcui_hip.hloc.extractors.sift import SIFT

    for bad in ({"backend": "pycolmap"}, {"backend": "pycolmap_cuda"}, {"first_octave": 0}, {"num_octaves": 2}, {"num_octaves": 6}):
        with pytest.raises(ImcuiHipError):
            SIFT(bad)
    with pytest.raises(ValueError):
        SIFT({"backend": "vlfeat"})
    with pytest.raises(ValueError):
        m({"image": torch.zeros(1, 2, 64, 64).cuda()})
