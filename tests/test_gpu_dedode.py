"""DeDoDe on the GPU against tests/dedode_reference.py (synthetic weights seed 0, both arithmetic modes): the detector's dense logits at
every scale, log p and the score map; the restated filter, score arithmetic and cut applied to the DEVICE's own log p / score map (bit
for bit); the end-to-end key-point sets; the sparse description head against the dense grid it never forms; rows past the count, batch
independence, graph replay, the file-based driver and DeDoDe followed by the Dual-Softmax plugin.

Sizes: 32 x 48 (1/8 map 4 x 6: smaller than the 5 x 5 filter's tile, narrower than the 51 taps at every scale), 40 x 56 (1/8 map 5 x 7,
odd maps below full resolution), 96 x 128 (several tiles and workgroups); batches of 3.

Bars.  delta = max(1e-4, 3 x the restatement's own fp32 spread over 1 / 8 threads) relative to a map's largest magnitude, D = delta x
the largest |logit| at full resolution.  log p = l - lse is held to 2 D.  The density is a positive-weighted sum of p + 1e-6, so
log score = log p - log(density + 1e-8) / 2 is held to 3 D plus the measured float32 round-off of the restated score arithmetic (the
explicit float32 form against its float64 evaluation on the same log p).  A key-point present in one set only must have a restated
log score within 6 D of the restatement's k-th, and at most 2 % of k may be such points.

Measured on one MI355X, both arithmetic modes: logits per scale within 3.9e-06 of the restatement (delta is its floor of 1e-4 at every
size: three times the restatement's own spread stays below it), log p within 4.5e-05 (bars 1.7e-03 .. 3.5e-03), log score within 4.4e-05, the 1/2-resolution description grid
within 1.5e-06; the rule on the device's maps exact in all 12 cases; end to end 0 of 64 key-points differ, log confidences within
9.5e-06, descriptors within 9.8e-07 of the grid's magnitude; the sparse head within 9.0e-08 .. 2.2e-07 of the dense grid's magnitude
(bars 2e-6 / 4e-6); 113 mutual matches of 300 between the two crops at threshold 0, the same in both directions."""
from __future__ import annotations

import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dedode_reference as R
from parity_utils import oracle_spread
from test_dedode_cpu import CAP, K, SIZES, image, sds

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
IDS = [f"{h}x{w}" for h, w in SIZES]
B = 3


@functools.lru_cache(maxsize=None)
def _plugin():
    from imcui_hip.hloc.extractors.dedode import DeDoDe

    det, desc = sds()
    return DeDoDe({"state_dict_detector": det, "state_dict_descriptor": desc}).eval().to(DEV)


def _batch(hw):
    return torch.cat([image(*hw, seed=s) for s in (3, 0, 4)])  # the reference image is image 1 of the batch


def _run(hw, k=K, img=None, **kw):
    m = _plugin()
    m.conf.update(max_keypoints=k)
    out = m.forward_batched((_batch(hw) if img is None else img).to(DEV), **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _reference(hw):
    """(fp32 spread of the logits over thread counts, of the description grid, the float32 restatement at k = K); once per size."""
    run = lambda: R.extract(*sds(), image(*hw), {"max_keypoints": K})  # noqa: E731
    s_logits, ref = oracle_spread(run, threads=(1, 8), keys=("logits",))
    s_dense, _ = oracle_spread(run, threads=(1, 8), keys=("dense", "desc2"))
    return s_logits, s_dense, ref


def _bars(hw):
    s_logits, s_dense, ref = _reference(hw)
    delta = max(1e-4, 3 * s_logits)
    D = delta * ref["logits"][-1].abs().max().item()
    logp = ref["logp"]
    roundoff = (torch.log(R.score_from_logp_explicit(logp)).double() - torch.log(R.score_from_logp_explicit(logp.double()))).abs().max().item()
    return delta, D, roundoff, max(1e-4, 3 * s_dense), ref


def _rel(a, b):
    return (a.double().cpu() - b.double()).abs().max().item() / max(b.abs().max().item(), 1e-30)


# ------------------------------------------------------------------ dense maps
@pytest.mark.parametrize("hw", SIZES, ids=IDS)
def test_dense_maps_against_the_restatement(hw, precision):
    delta, D, roundoff, delta_desc, ref = _bars(hw)
    out = _run(hw, want_maps=True)
    assert int(out["status"][0]) == 0
    errs = [_rel(a[1], b) for a, b in zip(out["logits"], ref["logits"])]
    e_logp = (out["logp"][1].double().cpu() - ref["logp"].double()).abs().max().item()
    e_score = (torch.log(out["score"][1]).double().cpu() - torch.log(ref["score"]).double()).abs().max().item()
    e_desc2 = _rel(out["desc2"][1], ref["desc2"])
    print(f"[dedode] {hw} mode {precision}: delta {delta:.1e} (D {D:.1e}), score round-off {roundoff:.1e}; logits per scale " + ", ".join(f"{e:.2e}" for e in errs)
          + f"; log p {e_logp:.2e} (bar {2 * D:.1e}); log score {e_score:.2e} (bar {3 * D + roundoff:.1e}); 1/2-resolution description grid {e_desc2:.2e} (bar {delta_desc:.1e})")  # fmt: skip
    assert [tuple(a.shape[1:]) for a in out["logits"]] == [tuple(b.shape) for b in ref["logits"]]
    for e in errs:
        assert e < delta, errs
    assert e_logp < 2 * D and e_score < 3 * D + roundoff and e_desc2 < delta_desc
    assert abs(torch.exp(out["logp"][1].double()).sum().item() - 1) < 1e-4


# ------------------------------------------------------------------ the rule on the device's own maps
def _assert_rule(out, b, k, kout=None):
    """The restated explicit-order filter and score on image b's DEVICE log p, then the restated cut: bit for bit."""
    logp, score = out["logp"][b].cpu(), out["score"][b].cpu()
    assert torch.equal(R.score_from_logp_explicit(logp), score), "score map: the written-out float32 order, bit for bit"
    want = R.select(score, k)
    assert int(out["num_keypoints"][b]) == k == want["idx"].numel()
    assert torch.equal(out["keypoints"][b, :k].cpu(), want["keypoints"]), "coordinates, in the rule's order"
    assert torch.equal(out["scores"][b, :k].cpu(), want["scores"]), "confidences are the scores"
    return want


@pytest.mark.parametrize("every", [False, True], ids=["k64", "kHW"])
@pytest.mark.parametrize("hw", SIZES, ids=IDS)
def test_rule_on_the_device_maps_is_bitwise(hw, every, precision):
    k = hw[0] * hw[1] if every else K
    out = _run(hw, k=k, want_maps=True)
    for b in (0, 1, 2):
        want = _assert_rule(out, b, k)
    s = out["scores"][1]
    assert torch.all(s[:-1] >= s[1:])
    if every:
        assert sorted(want["idx"].tolist()) == list(range(k))
    print(f"[dedode] {hw} k={k} mode {precision}: score map, count, order, coordinates and confidences equal the restated rule on the device's log p")


def test_crafted_equal_scores_follow_the_index_rule():
    from imcui_hip import backend

    impl = backend.DeDoDeHIP()
    H, W = 24, 40
    flat = torch.full((2, H, W), 0.125)
    out = impl.select_probe(flat.to(DEV), 37, mode="score")
    torch.cuda.synchronize()
    for b in range(2):
        want = R.select(flat[b], 37)
        assert want["idx"].tolist() == list(range(37)), "a flat map: the first k pixels"
        assert torch.equal(out["keypoints"][b].cpu(), want["keypoints"]) and torch.equal(out["scores"][b].cpu(), want["scores"])
    # three plateaus: 5 pixels at 0.9, 11 at 0.5 scattered over rows, the rest 0.1 with a -0.0 / +0.0 pair below; k cuts the 0.5 plateau
    g = torch.Generator().manual_seed(5)
    m = torch.full((H * W,), 0.1)
    perm = torch.randperm(H * W, generator=g)
    m[perm[:5]], m[perm[5:16]] = 0.9, 0.5
    m[perm[16]], m[perm[17]] = -0.0, 0.0
    m = m.view(1, H, W)
    for k in (3, 9, 16, 20, H * W):
        out = impl.select_probe(m.to(DEV), k, mode="score", kout=k + 3)
        torch.cuda.synchronize()
        want = R.select(m[0], k)
        assert torch.equal(out["keypoints"][0, :k].cpu(), want["keypoints"]) and torch.equal(out["scores"][0, :k].cpu(), want["scores"]), k
        assert not out["keypoints"][0, k:].any() and not out["scores"][0, k:].any() and int(out["num_keypoints"][0]) == k
    assert sorted(R.select(m[0], 9)["idx"][5:].tolist()) == sorted(perm[5:16].tolist())[:4], "the cut keeps the lowest indices of the plateau"
    # a flat log p through filter and score: zero padding makes the density smallest in the corners
    lp = torch.full((1, H, W), -float(np.log(H * W)))
    out = impl.select_probe(lp.to(DEV), 4, mode="logp")
    torch.cuda.synchronize()
    assert torch.equal(out["score"][0].cpu(), R.score_from_logp_explicit(lp[0]))
    corners = sorted(map(tuple, ((out["keypoints"][0].cpu() * 2).round() / 2).tolist()))
    assert corners == sorted([(0.5, 0.5), (W - 0.5, 0.5), (0.5, H - 0.5), (W - 0.5, H - 0.5)])


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("hw", SIZES, ids=IDS)
def test_end_to_end_against_the_restatement(hw, precision):
    delta, D, roundoff, delta_desc, ref = _bars(hw)
    out = _run(hw, want_maps=True)
    H, W = hw
    kp = out["keypoints"][1].cpu()
    idx = (torch.floor(kp[:, 1]).long() * W + torch.floor(kp[:, 0]).long()).tolist()
    ridx = ref["idx"].tolist()
    one = set(idx) ^ set(ridx)
    ls = torch.log(ref["score"].double()).reshape(-1)
    kth = ls[ridx[-1]].item()
    for i in one:
        assert abs(ls[i].item() - kth) < 6 * D, f"pixel {i} is in one set only and its restated log score is {ls[i].item() - kth:+.2e} from the k-th (6 D = {6 * D:.1e})"
    assert len(one) // 2 <= CAP * K
    common = [i for i in idx if i in set(ridx)]
    rows, rrows = [idx.index(i) for i in common], [ridx.index(i) for i in common]
    assert torch.equal(kp[rows], ref["keypoints"][rrows]), "positions of the common key-points are equal"
    e_conf = (torch.log(out["scores"][1].cpu()[rows]).double() - torch.log(ref["scores"][rrows]).double()).abs().max().item()
    M = ref["dense"].abs().max().item()
    e_desc = (out["descriptors"][1].cpu()[rows].double() - ref["descriptors"][rrows].double()).abs().max().item() / M
    print(f"[dedode] {hw} mode {precision}: {len(one) // 2} of {K} key-points in one set only, {len(common)} common: log confidence {e_conf:.2e} "
          f"(bar {3 * D + roundoff:.1e}), descriptors {e_desc:.2e} of the grid's magnitude (bar {delta_desc:.1e})")  # fmt: skip
    assert len(common) >= K - 1 and e_conf < 3 * D + roundoff and e_desc < delta_desc


@pytest.mark.parametrize("hw", SIZES, ids=IDS)
def test_sparse_head_equals_the_dense_grid(hw, precision):
    """The descriptors of the sparse head against grid_sample of the full-resolution grid written for this test only, which out_conv
    forms on the shared GEMM; the bar is that GEMM's own against float64 (tests/test_gpu_gemm_variants.py: 2e-6 exact, 4e-6 split),
    relative to the grid's largest magnitude."""
    k = 200
    out = _run(hw, k=k, want_maps=True, want_dense=True)
    bar = 2e-6 if precision == 0 else 4e-6
    worst = 0.0
    for b in range(B):
        want = R.select(out["score"][b].cpu(), k)
        dense = out["dense"][b].cpu()
        got = R.describe(dense.permute(2, 0, 1).contiguous(), want["grid"])
        at_pixel = dense.reshape(-1, 256)[want["idx"]]
        assert (got - at_pixel).abs().max().item() <= 1e-5 * dense.abs().max().item()  # the round trip's weights at a pixel centre
        worst = max(worst, (out["descriptors"][b].cpu() - got).abs().max().item() / dense.abs().max().item())
    ref_e = _rel(out["dense"][1], _bars(hw)[4]["dense"])
    print(f"[dedode] {hw} mode {precision}: sparse head against the dense grid {worst:.2e} of its magnitude (bar {bar:.0e}); dense grid against the restatement {ref_e:.2e}")
    assert worst < bar and ref_e < _bars(hw)[3]


# ------------------------------------------------------------------ batches, graphs, the plugin
def test_rows_past_the_count_batch_independence_and_graph_replay(precision):
    from imcui_hip import backend

    hw = (40, 56)
    m = _plugin()
    m.conf.update(max_keypoints=50)
    keys = ("keypoints", "scores", "descriptors", "num_keypoints")
    batch = _batch(hw).to(DEV)
    padded = m.forward_batched(batch, kout=70)
    assert padded["keypoints"].shape == (B, 70, 2) and padded["num_keypoints"].tolist() == [50] * B
    assert not padded["keypoints"][:, 50:].any() and not padded["scores"][:, 50:].any() and not padded["descriptors"][:, 50:].any()
    assert padded["descriptors"][:, :50].abs().amax(dim=2).min().item() > 0
    solo = m.forward_batched(batch[1:2])
    trio = m.forward_batched(batch)
    for k in keys:
        assert torch.equal(solo[k][0], trio[k][1]), k
        assert torch.equal(padded[k][:, :50] if k != "num_keypoints" else padded[k], trio[k]), k
    eager = trio
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
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.utils.base_model import dynamic_load

    hw = (96, 128)
    det, desc = sds()
    m = dynamic_load(extractors, "dedode")({"state_dict_detector": det, "state_dict_descriptor": desc, "max_keypoints": 40}).eval().to(DEV)
    pred = m({"image": image(*hw).to(DEV)})
    kp, de, sc = pred["keypoints"], pred["descriptors"], pred["scores"]
    assert kp.shape == (1, 40, 2) and de.shape == (1, 256, 40) and sc.shape == (1, 40)
    assert kp.dtype == de.dtype == sc.dtype == torch.float32 and kp.is_cuda and de.is_contiguous()
    assert torch.all(sc[0, :-1] >= sc[0, 1:])
    assert kp[..., 0].min() > 0 and kp[..., 0].max() < hw[1] and kp[..., 1].min() > 0 and kp[..., 1].max() < hw[0]
    assert (kp - torch.floor(kp) - 0.5).abs().max().item() < 1e-4, "pixel centres (the float32 round trip through the normalised grid)"
    assert (de[0].norm(dim=0) - 1).abs().max().item() > 1e-2, "descriptors are not normalised: the matcher does that"


def test_dedode_extract_from_files(tmp_path, golden_dir):
    """The `dedode` conf (imcui/hloc/configs/extractors.py:317-331, recorded in tests/golden/dedode_confs.json) through the file-based
    batch extractor on 96 x 128 images; resize_max is lowered from 1600 to 128 so that `force_resize` keeps the small image as it is."""
    from PIL import Image

    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc import extractors
    from imcui_hip.hloc.utils.base_model import dynamic_load
    from imcui_hip.hloc.utils.h5lite import open_h5
    from test_gpu_disk_files import _host_rgb, _rgb_u8

    with open(os.path.join(golden_dir, "dedode_confs.json")) as f:
        conf = json.load(f)["extractor_confs"]["dedode"]
    conf = {**conf, "preprocessing": {**conf["preprocessing"], "resize_max": 128}}
    root = tmp_path / "images"
    root.mkdir()
    images = {"a.png": _rgb_u8(96, 128, 400), "b.png": _rgb_u8(96, 128, 401)}
    for fname, arr in images.items():
        Image.fromarray(np.ascontiguousarray(arr)).save(root / fname)
    det, desc = sds()
    model = dynamic_load(extractors, conf["model"]["name"])({**conf["model"], "state_dict_detector": det, "state_dict_descriptor": desc}).eval().to(DEV)
    feature_path = ef.main(conf, root, tmp_path / "out", model=model, batch_size=2)
    assert feature_path == tmp_path / "out" / (conf["output"] + ".h5")
    assert sorted(ef.list_h5_names(feature_path)) == sorted(images)
    pconf = SimpleNamespace(**{**ef.DEFAULT_PREPROCESSING, **conf["preprocessing"]})
    with open_h5(feature_path, "r") as fd:
        for f in images:
            raw = ef.read_image_u8(root / f)
            img = _host_rgb(raw, pconf).cuda()
            with torch.no_grad():
                pred = model({"image": img})
            grp = fd[f]
            assert set(grp.keys()) == {"keypoints", "scores", "descriptors", "image_size"}
            n = pred["keypoints"].shape[1]
            assert n == 5000
            kp = ((pred["keypoints"][0].cpu().numpy() + 0.5) * np.ones(2, np.float32)[None] - 0.5).astype(np.float16)
            assert grp["keypoints"].__array__().shape == (n, 2) and np.array_equal(grp["keypoints"].__array__(), kp), f
            assert grp["descriptors"].__array__().shape == (256, n) and grp["descriptors"].__array__().dtype == np.float16
            assert np.array_equal(grp["scores"].__array__(), pred["scores"][0].cpu().numpy().astype(np.float16))
            assert np.array_equal(grp["descriptors"].__array__(), pred["descriptors"][0].cpu().numpy().astype(np.float16))
            assert tuple(grp["image_size"].__array__()) == (128, 96)


def test_dedode_then_dual_softmax_on_two_crops():
    """The zoo entry `dedode` = this extractor + the Dual-Softmax matcher (which normalises the 256-d descriptors): two crops of one
    canvas, matched in both directions, agree with each other, and every match is a mutual pair of rows."""
    from imcui_hip.hloc.matchers.dual_softmax import DualSoftMax

    m = _plugin()
    m.conf.update(max_keypoints=300)
    canvas = image(96, 160, seed=7)
    crops = [canvas[..., :128].contiguous(), canvas[..., 32:].contiguous()]
    preds = [m({"image": c.to(DEV)}) for c in crops]
    shifted = lambda rows, cols: ((preds[0]["keypoints"][0].cpu()[rows] - preds[1]["keypoints"][0].cpu()[cols] - torch.tensor([32.0, 0.0])).abs().amax(dim=1) < 0.5).sum().item()  # noqa: E731
    for thr in (0.0, 0.2):  # every mutual nearest neighbour, then the plugin's default threshold
        matcher = DualSoftMax({"match_threshold": thr}).eval().to(DEV)
        fwd = matcher({"descriptors0": preds[0]["descriptors"], "descriptors1": preds[1]["descriptors"]})
        bwd = matcher({"descriptors0": preds[1]["descriptors"], "descriptors1": preds[0]["descriptors"]})
        m0, m1 = fwd["matches0"][0].cpu(), bwd["matches0"][0].cpu()
        assert m0.shape == (300,) and m0.dtype == torch.int64 and m0.max().item() < 300
        rows = torch.nonzero(m0 >= 0)[:, 0]
        assert torch.equal(m1[m0[rows]], rows), "a match of crop 0 -> 1 is the match of 1 -> 0"
        assert torch.nonzero(m1 >= 0).numel() == rows.numel() and m0[rows].unique().numel() == rows.numel()
        print(f"[dedode] two crops shifted by 32 px, match_threshold {thr}: {rows.numel()} mutual matches of 300, {shifted(rows, m0[rows])} of them on the same "
              "canvas pixel (synthetic weights)")  # fmt: skip
        if thr == 0.0:
            assert rows.numel() >= 10, rows.numel()
