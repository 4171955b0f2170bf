"""AdaLAM (`adalam`) on the GPU against the numpy restatement tests/adalam_reference.py.

Stage A (putative matches on the matrix cores) is compared by equality on integer descriptors, where every arithmetic is exact; the
filter (stages B .. G, imcui_hip_adalam_filter) by equality against the float32 restatement, which follows the kernel's operation
order, and within 1 % of a scene's key-points against float64.
"""
import functools
import io
import os

import numpy as np
import pytest
import torch

import adalam_reference as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
EPS32 = 2.0**-23


def _impl():
    from imcui_hip import backend

    return backend.AdaLAMHIP()


def _conf(**over):
    return {**R.DEFAULT_CONF, **over}


@functools.lru_cache(maxsize=None)
def _scene(seed, N=None, filters=None, dup=False):
    sc = R.make_scene(seed, N=N, filters=filters)
    if dup:  # SIFT's multi-orientation case: 20 % of the key-points once more at the same position, orientation turned by 90 degrees
        rng = np.random.default_rng(1000 + seed)
        pick = rng.choice(len(sc["k0"]), len(sc["k0"]) // 5, replace=False)
        for k in ("k0", "k1", "d0", "d1", "o0", "o1", "s0", "s1", "outlier"):
            sc[k] = np.concatenate([sc[k], sc[k][pick]])
        sc["o0"][-len(pick):] += 90
        sc["o1"][-len(pick):] += 90
    return sc


@functools.lru_cache(maxsize=None)
def _stage_a32(seed, N=None, filters=None, dup=False):
    sc = _scene(seed, N, filters, dup)
    return R.stage_a(sc["d0"], sc["d1"], np.float32)


def _ref(sc, a, conf, dtype):
    return R.filter_matches(sc["k0"], sc["k1"], sc["o0"], sc["o1"], sc["s0"], sc["s1"], a["nn"], a["score"], a["mnn"], sc["size"], sc["size"],
                            {**sc["conf"], **conf}, dtype)  # fmt: skip


def _pad(arrs, ncap, dtype, tail=()):
    out = torch.zeros((len(arrs), ncap, *tail), dtype=dtype)
    for b, a in enumerate(arrs):
        out[b, : len(a)] = torch.as_tensor(np.asarray(a)).to(dtype)
    return out.to(DEV)


def _geom(scs, ncap=None):
    ncap = ncap or max(max(len(s["k0"]), len(s["k1"]), 1) for s in scs)
    k0, k1 = _pad([s["k0"] for s in scs], ncap, torch.float32, (2,)), _pad([s["k1"] for s in scs], ncap, torch.float32, (2,))
    so = tuple(_pad([s[k] for s in scs], ncap, torch.float32) for k in ("s0", "o0", "s1", "o1"))
    n0 = torch.tensor([len(s["k0"]) for s in scs], dtype=torch.int32, device=DEV)
    n1 = torch.tensor([len(s["k1"]) for s in scs], dtype=torch.int32, device=DEV)
    return ncap, k0, k1, so, n0, n1


def _gpu_filter(scs, As, conf, members=True, impl=None, ncap=None):
    """imcui_hip_adalam_filter on a batch of scenes with given putative matches; everything back on the host."""
    ncap, k0, k1, so, n0, n1 = _geom(scs, ncap)
    nn = _pad([a["nn"] for a in As], ncap, torch.int32)
    score = _pad([a["score"] for a in As], ncap, torch.float32)
    mnn = _pad([a["mnn"] for a in As], ncap, torch.int32)
    H, W = scs[0]["size"]
    out = (impl or _impl()).filter(k0, k1, nn, score, mnn, n0, n1, (W, H), (W, H), conf, scales_oris=so, members=members)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_filter(out, b, sc, a, conf, tag, members=True):
    """Pair b of a GPU result against both restatements."""
    n = len(sc["k0"])
    r32, r64 = _ref(sc, a, conf, np.float32), _ref(sc, a, conf, np.float64)
    assert np.array_equal(out["seed"][b, :n].astype(bool), r32["seed"]), tag
    assert np.array_equal(r32["seed"], r64["seed"]), tag
    info = out["seed_info"][b, :n]
    assert np.array_equal(info[:, 0], r32["n_members"]), tag
    if members:
        for s, mem in r32["members"].items():
            assert np.array_equal(out["seed_members"][b, s, : len(mem)], mem), (tag, s)
            assert np.array_equal(mem, r64["members"][s]), (tag, s)
    assert np.array_equal(info[:, 1], r32["best_iter"]), (tag, np.flatnonzero(info[:, 1] != r32["best_iter"])[:5])
    assert np.array_equal(info[:, 2], r32["count"]), tag
    assert np.array_equal(info[:, 3].astype(bool), r32["passed"]), tag
    assert np.array_equal(out["matches0"][b, :n], r32["matches0"]), tag
    assert (out["matches0"][b, n:] == -1).all() and (out["matching_scores0"][b] == 0).all(), tag
    diff = int((out["matches0"][b, :n] != r64["matches0"]).sum())
    same = (info[:, 2] == r64["count"]) & (r64["count"] > 0) & (r32["count"] == r64["count"])
    c64 = r64["conf"][same]
    e32 = float((np.abs(r32["conf"][same].astype(np.float64) - c64) / c64).max()) if same.any() else 0.0
    eg = float((np.abs(out["seed_conf"][b, :n][same].astype(np.float64) - c64) / c64).max()) if same.any() else 0.0
    print(f"{tag}: {int(r32['seed'].sum())} seeds, {int(r32['passed'].sum())} passed, {int((r32['matches0'] > -1).sum())} matches, widest "
          f"neighbourhood {int(r32['n_members'].max()) if n else 0}; vs float64 {diff} of {n} key-points differ (cap {n // 100}); conf error {eg:.3g} "
          f"(float32 restatement {e32:.3g}, bar {3 * max(e32, EPS32):.3g})")  # fmt: skip
    assert diff <= n // 100, tag
    assert eg <= 3 * max(e32, EPS32), tag
    return r32


# ------------------------------------------------------------------ stage A
def _int_desc(rng, n, D, hi=16):
    return rng.integers(0, hi, (n, D)).astype(np.float64)


def _run_stage_a(d0, d1):
    n0, n1 = len(d0), len(d1)
    ncap = max(n0, n1)
    rng = np.random.default_rng(7)
    k0 = _pad([rng.uniform(0, 300, (n0, 2))], ncap, torch.float32, (2,))
    k1 = _pad([rng.uniform(0, 300, (n1, 2))], ncap, torch.float32, (2,))
    t0, t1 = _pad([d0], ncap, torch.float32, (d0.shape[1],)), _pad([d1], ncap, torch.float32, (d1.shape[1],))
    c0 = torch.tensor([n0], dtype=torch.int32, device=DEV)
    c1 = torch.tensor([n1], dtype=torch.int32, device=DEV)
    out = _impl().forward(k0, k1, t0, t1, c0, c1, (320, 240), (320, 240), _conf(**R.FILTERS_OFF), probe=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy()[0] for k, v in out.items()}


@pytest.mark.parametrize("n0,n1", [(2, 2), (5, 300), (63, 64), (64, 65), (129, 128), (257, 4096), (4096, 4096)])
def test_stage_a_integer_descriptors_exact(n0, n1, precision):
    """nn, mnn and the score bits against exact integer arithmetic (float32 holds every intermediate exactly)."""
    rng = np.random.default_rng(n0 * 10007 + n1)
    d0, d1 = _int_desc(rng, n0, 128), _int_desc(rng, n1, 128)
    m = min(n0, n1)
    d1[: m // 2] = d0[: m // 2]  # exact matches (distance 0) and ...
    d1[m // 2 : m] = d0[m // 2 : m] + (rng.random((m - m // 2, 128)) < 0.1)  # ... near ones
    if n1 > 4:
        d1[n1 - 1] = d1[1]  # equal minima: the lowest index wins
    ref = R.stage_a(d0, d1, np.float64)
    out = _run_stage_a(d0, d1)
    assert np.array_equal(out["nn"][:n0], ref["nn"])
    assert np.array_equal(out["mnn"][:n0].astype(bool), ref["mnn"])
    assert np.array_equal(out["score"][:n0].view(np.uint32), R.stage_a(d0, d1, np.float32)["score"].view(np.uint32))
    assert np.array_equal(out["score"][:n0], (ref["dist"].astype(np.float32) / np.maximum(ref["d2nd"].astype(np.float32), np.float32(1e-3))))


@pytest.mark.parametrize("D", [64, 128, 256])
def test_stage_a_other_widths_and_norm_ratio(D, precision):
    """Unnormalised descriptors whose norms differ by a factor of 4 between the images, at every width."""
    rng = np.random.default_rng(D)
    d0 = _int_desc(rng, 200, D)
    d1 = np.concatenate([4 * d0[:150] + (rng.random((150, D)) < 0.2), _int_desc(rng, 100, D, 64)])
    ref = R.stage_a(d0, d1, np.float64)
    out = _run_stage_a(d0, d1)
    assert np.array_equal(out["nn"][:200], ref["nn"]) and np.array_equal(out["mnn"][:200].astype(bool), ref["mnn"])
    assert np.array_equal(out["score"][:200], R.stage_a(d0, d1, np.float32)["score"])


def test_stage_a_rootsift_like_descriptors(precision):
    """Float descriptors: nn / mnn equal float64 wherever float64's margin between best and second exceeds 3 x the float32
    restatement's error on the distances."""
    rng = np.random.default_rng(5)
    n0, n1 = 700, 900
    x = rng.gamma(0.5, 1.0, (n1, 128))
    d1 = np.sqrt(x / x.sum(1, keepdims=True)).astype(np.float32).astype(np.float64)
    y = x[:n0] * rng.uniform(0.7, 1.3, (n0, 128))
    d0 = np.sqrt(y / y.sum(1, keepdims=True)).astype(np.float32).astype(np.float64)
    r64, r32 = R.stage_a(d0, d1, np.float64), R.stage_a(d0, d1, np.float32)
    bar = 3 * max(float(np.abs(r32["dist"] - r64["dist"]).max()), float(np.abs(r32["d2nd"] - r64["d2nd"]).max()))
    out = _run_stage_a(d0, d1)
    clear = (r64["d2nd"] - r64["dist"]) > bar
    dist = (R.sq_norms(d0, np.float64)[:, None] - 2 * (d0 @ d1.T)) + R.sq_norms(d1, np.float64)[None, :]
    col = np.partition(dist, 1, axis=0)
    col_clear = (col[1] - col[0]) > bar
    print(f"root-SIFT-like: bar {bar:.3g}, {int(clear.sum())} of {n0} rows clear, error of the score {np.abs(out['score'][:n0] - r64['score']).max():.3g}")
    assert clear.sum() > 0.9 * n0
    assert np.array_equal(out["nn"][:n0][clear], r64["nn"][clear])
    ok = clear & col_clear[r64["nn"]]
    assert np.array_equal(out["mnn"][:n0][ok].astype(bool), r64["mnn"][ok])


def test_refusals():
    from imcui_hip import backend

    impl = _impl()
    sc = _scene(3)
    ncap, k0, k1, so, n0, n1 = _geom([sc])
    d = torch.zeros((1, ncap, 96), device=DEV)
    with pytest.raises(backend.ImcuiHipError, match="width"):
        impl.forward(k0, k1, d, d, n0, n1, (320, 240), (320, 240), _conf(), scales_oris=so)
    d = torch.zeros((1, ncap, 128), device=DEV)
    with pytest.raises(backend.ImcuiHipError, match="oris"):
        impl.forward(k0, k1, d, d, n0, n1, (320, 240), (320, 240), _conf(), scales_oris=None)
    hd = backend.get_handle(torch.device(DEV))
    carr = backend.adalam_conf_array(_conf())
    z = torch.zeros(8, device=DEV)
    zi = torch.zeros(8, dtype=torch.int32, device=DEV)
    args = (backend._ptr(z), backend._ptr(z), None, None, None, None, backend._ptr(zi), backend._ptr(zi), 240, 320, 240, 320, carr, backend._ptr(zi), backend._ptr(z),
            None, None, None, None, None, None, None, backend._ptr(z), 32)  # fmt: skip
    assert hd.launch(hd.lib.imcui_hip_adalam_forward, 1, 4, 96, backend._ptr(z), backend._ptr(z), *args, check=False) == -4
    assert hd.launch(hd.lib.imcui_hip_adalam_forward, 1, 5000, 128, backend._ptr(z), backend._ptr(z), *args, check=False) == -4
    assert hd.launch(hd.lib.imcui_hip_adalam_forward, 1, 4, 128, backend._ptr(z), backend._ptr(z), *args, check=False) == -1  # thresholds on, no oris
    assert hd.lib.imcui_hip_adalam_workspace_bytes(hd.h, 1, 5000, 128) == 0


# ------------------------------------------------------------------ stages B .. G
@pytest.mark.parametrize("seed", sorted(R.SCENES))
def test_filter_scenes(seed):
    sc, a = _scene(seed), _stage_a32(seed)
    conf = _conf(**sc["conf"])
    out = _gpu_filter([sc], [a], conf)
    r32 = _check_filter(out, 0, sc, a, conf, f"scene {seed}")
    assert r32["passed"].sum() >= 10 and (r32["matches0"] > -1).sum() >= 0.3 * len(sc["k0"])


@pytest.mark.parametrize("N", [6, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096])
def test_filter_one_neighbourhood_of_every_width(N):
    """area_ratio = 1: every neighbourhood holds all N key-points, so N is the member count: exactly min_inliers, and one case on
    either side of every width at which the LDS sort (64, 128, ... 4096 keys) and the scan (one / several keys per thread, at 256) switch."""
    sc, a = _scene(11, N, False), _stage_a32(11, N, False)
    conf = _conf(**sc["conf"], area_ratio=1)
    out = _gpu_filter([sc], [a], conf, members=N <= 2049)
    r32 = _check_filter(out, 0, sc, a, conf, f"N = {N}", members=N <= 2049)
    assert r32["seed"].any() and (r32["n_members"][r32["seed"]] == N).all()


@pytest.mark.parametrize("over", [{"ransac_iters": 1}, {"ransac_iters": 5}, {"refit": False}, {"force_seed_mnn": False},
                                  {"orientation_difference_threshold": None}, {"scale_rate_threshold": None},
                                  {"detected_scale_rate_threshold": None}, {"min_inliers": 3, "min_confidence": 50}],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))  # fmt: skip
def test_filter_conf_variants(over):
    sc, a = _scene(0), _stage_a32(0)
    conf = _conf(**over)
    out = _gpu_filter([sc], [a], conf)
    _check_filter(out, 0, sc, a, conf, str(over))


def test_filter_duplicated_keypoints():
    """20 % of the key-points twice at one position with the orientation turned by 90 degrees: duplicates inside a neighbourhood carry
    weight 0, and with the orientation test off both copies are members."""
    for filters in (True, False):
        sc, a = _scene(0, None, filters, True), _stage_a32(0, None, filters, True)
        conf = _conf(**sc["conf"])
        out = _gpu_filter([sc], [a], conf)
        _check_filter(out, 0, sc, a, conf, f"duplicates, filters {filters}")


def test_filter_noise_free_scene_accepts_nothing():
    """Every residual of an exact similarity is too perfect: weight 0 everywhere, count 0, nothing accepted."""
    sc = dict(_scene(3))
    th = np.radians(90.0)
    Rm = 2.0 * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]).round()
    sc["k1"] = (sc["k0"] - 100) @ Rm.T + 300  # exact in float32
    a = R.stage_a(sc["d0"], sc["d0"], np.float32)
    conf = _conf(**R.FILTERS_OFF, detected_scale_rate_threshold=None)
    out = _gpu_filter([sc], [a], conf)
    r32 = _check_filter(out, 0, sc, a, conf, "noise-free")
    assert r32["seed"].any() and (r32["n_members"] >= 6).any() and not r32["passed"].any() and (out["matches0"] == -1).all()


@pytest.mark.parametrize("n", [0, 1, 2, 5, 6])
def test_filter_tiny_pairs(n):
    sc = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in _scene(3).items()}
    a = R.stage_a(sc["d0"], sc["d1"], np.float32)
    conf = _conf(**R.FILTERS_OFF, area_ratio=1, min_confidence=1)
    out = _gpu_filter([sc], [a], conf, ncap=8)
    _check_filter(out, 0, sc, a, conf, f"{n} key-points")
    if n < 2:
        assert (out["matches0"] == -1).all() and not out["seed"].any()


# ------------------------------------------------------------------ batching
def _ragged():
    seeds = [(0, None), (2, None), (3, 0), (4, None), (1, 700)]  # (scene, N): the third pair is empty
    scs = [_scene(s, N) if N != 0 else {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in _scene(s).items()} for s, N in seeds]
    return scs


def _batch_tensors(scs):
    ncap, k0, k1, so, n0, n1 = _geom(scs)
    d0, d1 = _pad([s["d0"] for s in scs], ncap, torch.float32, (128,)), _pad([s["d1"] for s in scs], ncap, torch.float32, (128,))
    H, W = scs[0]["size"]
    return (k0, k1, d0, d1, n0, n1, (W, H), (W, H)), so


def _forward_batch(impl, scs, conf, tensors=None):
    args, so = tensors or _batch_tensors(scs)
    return impl.forward(*args, conf, scales_oris=so, probe=True)


def test_ragged_batch_equals_single_pairs(precision):
    scs = _ragged()
    conf = _conf(**R.FILTERS_OFF)
    impl = _impl()
    out = {k: v.cpu().numpy() for k, v in _forward_batch(impl, scs, conf).items()}
    for b, sc in enumerate(scs):
        n = len(sc["k0"])
        one = {k: v.cpu().numpy() for k, v in _forward_batch(impl, [sc], conf).items()}
        for k in ("matches0", "matching_scores0", "nn", "score", "mnn", "seed", "seed_info", "seed_conf"):
            assert np.array_equal(out[k][b, :n].view(np.int32), one[k][0, :n].view(np.int32)), (b, k)
        assert (out["matches0"][b, n:] == -1).all()
        ref = R.run_scene(sc, np.float32, conf) if n else None
        if n:
            assert np.array_equal(out["matches0"][b, :n], ref["matches0"]), b
            assert np.array_equal(out["nn"][b, :n], ref["nn"]) and np.array_equal(out["score"][b, :n], ref["score"]), b
    assert (out["matches0"][2] == -1).all()


def test_graph_capture_and_replay_bit_equal():
    from imcui_hip import backend

    scs = _ragged()
    conf = _conf(**R.FILTERS_OFF)
    impl = _impl()
    tensors = _batch_tensors(scs)  # (made before the capture: a host-to-device copy cannot be captured)
    eager = {k: v.clone() for k, v in _forward_batch(impl, scs, conf, tensors).items()}
    assert (eager["matches0"] > -1).sum() >= 400
    table = {}
    with backend.workspace_owner(table):
        _forward_batch(impl, scs, conf, tensors)  # warm-up: the workspace
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = _forward_batch(impl, scs, conf, tensors)
    for _ in range(2):
        for v in out.values():
            v.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        for k, v in eager.items():
            assert torch.equal(v.view(torch.int32), out[k].view(torch.int32)), k


# ------------------------------------------------------------------ end to end
def _model(**conf):
    from imcui_hip.hloc.matchers.adalam import AdaLAM

    return AdaLAM(conf).eval().to(DEV)


def _data(sc):
    H, W = sc["size"]
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=DEV)[None]  # noqa: E731
    return {"image0": torch.zeros(1, 1, H, W, device=DEV), "image1": torch.zeros(1, 1, H, W, device=DEV), "keypoints0": t(sc["k0"]),
            "keypoints1": t(sc["k1"]), "descriptors0": t(sc["d0"].T), "descriptors1": t(sc["d1"].T), "scales0": t(sc["s0"]), "scales1": t(sc["s1"]),
            "oris0": t(sc["o0"]), "oris1": t(sc["o1"])}  # fmt: skip


def test_plugin_forward_and_forward_batched():
    sc = _scene(0)
    model = _model()
    ref = R.run_scene(sc, np.float32)
    pred = model(_data(sc))
    assert pred["matches0"].dtype == torch.long and pred["matches0"].shape == (1, 300) and pred["matching_scores0"].shape == (1, 300)
    assert np.array_equal(pred["matches0"][0].cpu().numpy(), ref["matches0"]) and (pred["matching_scores0"] == 0).all()
    assert (ref["matches0"] > -1).sum() > 150
    scs = [_scene(0), _scene(3)]
    ncap, k0, k1, so, n0, n1 = _geom(scs)
    d0, d1 = _pad([s["d0"] for s in scs], ncap, torch.float32, (128,)), _pad([s["d1"] for s in scs], ncap, torch.float32, (128,))
    out = model.forward_batched(k0, k1, d0, d1, n0, n1, (320, 240), (320, 240), scales_oris=so)
    for b, s in enumerate(scs):
        assert np.array_equal(out["matches0"][b, : len(s["k0"])].cpu().numpy(), R.run_scene(s, np.float32)["matches0"]), b
    with pytest.raises(AttributeError, match="oris"):
        model.forward_batched(k0, k1, d0, d1, n0, n1, (320, 240), (320, 240), scales_oris=None)
    one = model(_data({k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in sc.items()}))  # adalam.py:41-44
    assert one["matches0"].shape == (1, 1) and (one["matches0"] == -1).all()


def test_match_from_pairs_with_scales_and_oris():
    from imcui_hip.hloc import match_features as mf

    feats = {}
    scs = {"a": _scene(0), "b": _scene(3), "c": _scene(2)}
    for name, sc in scs.items():
        for side in (0, 1):
            feats[f"{name}{side}"] = {"keypoints": sc[f"k{side}"].astype(np.float32), "descriptors": sc[f"d{side}"].T.astype(np.float32),
                                      "scales": sc[f"s{side}"].astype(np.float32), "oris": sc[f"o{side}"].astype(np.float32),
                                      "image_size": np.array([320, 240])}  # fmt: skip
    store, sink = mf.DictFeatureStore(feats), mf.DictMatchSink()
    pairs = [(f"{n}0", f"{n}1") for n in scs]
    assert mf.match_from_pairs(_model(), pairs, store, store, sink, batch_size=2) == 3
    for name, sc in scs.items():
        rec = sink.matches[mf.names_to_pair(f"{name}0", f"{name}1")]
        assert np.array_equal(rec["matches0"], R.run_scene(sc, np.float32)["matches0"]), name
        assert (rec["matching_scores0"] == 0).all()


def test_sift_features_of_real_images_through_the_plugin():
    """Root-SIFT descriptors, scales and orientations of a real image pair: nn / score / mnn are taken from the GPU and fed to the
    restatement's filter, which must then agree with the GPU's filter."""
    from PIL import Image

    from imcui_hip.hloc.extractors.sift import SIFT

    z = np.load(os.path.join(HERE, "golden", "evd_pairs.npz"))
    imgs = [torch.from_numpy(np.asarray(Image.open(io.BytesIO(z[f"img{s}_0"].tobytes())).convert("L"), dtype=np.float32) / 255.0) for s in (0, 1)]
    sift = SIFT({"max_keypoints": 1024}).eval().to(DEV)
    f = [sift({"image": im[None, None].to(DEV)}) for im in imgs]
    data = {"image0": imgs[0][None, None].to(DEV), "image1": imgs[1][None, None].to(DEV)}
    for side in (0, 1):
        for k in ("keypoints", "descriptors", "scales", "oris"):
            data[f"{k}{side}"] = f[side][k]
    model = _model()
    pred = model(data)["matches0"][0].cpu().numpy()
    n0, n1 = data["keypoints0"].shape[1], data["keypoints1"].shape[1]
    c0 = torch.tensor([n0], dtype=torch.int32, device=DEV)
    c1 = torch.tensor([n1], dtype=torch.int32, device=DEV)
    so = (data["scales0"], data["oris0"], data["scales1"], data["oris1"])
    size = tuple(imgs[0].shape[::-1])
    out = model.forward_batched(data["keypoints0"], data["keypoints1"], data["descriptors0"].transpose(2, 1).contiguous(),
                                data["descriptors1"].transpose(2, 1).contiguous(), c0, c1, size, tuple(imgs[1].shape[::-1]), scales_oris=so, probe=True)  # fmt: skip
    o = {k: v.cpu().numpy()[0] for k, v in out.items()}
    assert np.array_equal(o["matches0"][:n0], pred)
    g = lambda k: data[k][0].cpu().numpy().astype(np.float64)  # noqa: E731
    ref = R.filter_matches(g("keypoints0"), g("keypoints1"), g("oris0"), g("oris1"), g("scales0"), g("scales1"), o["nn"][:n0], o["score"][:n0],
                           o["mnn"][:n0], imgs[0].shape, imgs[1].shape, None, np.float32)  # fmt: skip
    print(f"real pair: {n0} x {n1} key-points, {int(ref['seed'].sum())} seeds, {int(ref['passed'].sum())} passed, {int((ref['matches0'] > -1).sum())} matches")
    assert np.array_equal(o["seed"][:n0].astype(bool), ref["seed"])
    assert np.array_equal(o["seed_info"][:n0, 0], ref["n_members"])
    assert np.array_equal(pred, ref["matches0"])
