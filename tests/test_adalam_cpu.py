"""AdaLAM without a device: the numpy restatement's stages on hand-made cases, its float32 mode against float64 on the six scenes,
the plugin's conf / required inputs / refusals, and the new exports in the header."""
import numpy as np
import pytest
import torch

import adalam_reference as R

SIZE = (240, 320)
OFF = dict(R.FILTERS_OFF)


def _filter(k0, k1, nn=None, score=None, mnn=None, conf=None, o0=None, o1=None, s0=None, s1=None, dtype=np.float64):
    n = len(k0)
    nn = np.arange(n) if nn is None else nn
    score = np.full(n, 0.1) if score is None else score
    mnn = np.ones(n, dtype=bool) if mnn is None else mnn
    return R.filter_matches(np.asarray(k0, float), np.asarray(k1, float), o0, o1, s0, s1, nn, score, mnn, SIZE, SIZE, conf or OFF, dtype)


def test_stage_a_ties_second_best_and_small_sets():
    d0 = np.array([[1.0, 0], [0, 2], [3, 3]])
    d1 = np.array([[0.0, 2], [1, 0], [1, 0], [5, 5]])
    a = R.stage_a(d0, d1)
    assert a["nn"].tolist() == [1, 0, 3] and a["nn21"].tolist() == [1, 0, 0, 2]  # equal minima: the lowest index
    assert a["mnn"].tolist() == [True, True, True]
    assert a["dist"].tolist() == [0, 0, 8] and a["d2nd"].tolist() == [0, 5, 10]
    assert np.allclose(a["score"], [0, 0, 0.8])  # the second best of row 0 is the tied minimum; the denominator is floored at 1e-3
    for n0, n1 in ((1, 4), (3, 1), (0, 0)):
        a = R.stage_a(d0[:n0], d1[:n1])
        assert (a["nn"] == -1).all() and not a["mnn"].any() and len(a["nn"]) == n0
    a32 = R.stage_a(d0 * 1000, d1 * 1000, np.float32)
    assert a32["score"].dtype == np.float32 and a32["nn"].tolist() == [1, 0, 3]


def test_seed_rule_equal_scores_and_strict_radius():
    R0 = np.sqrt(240 * 320 / 100 / np.pi)  # 15.63...
    k0 = np.array([[50, 50], [55, 50], [50 + 15.5, 50], [50, 50 + 15.75], [200, 200], [202, 200]])
    score = np.array([0.2, 0.2, 0.3, 0.3, 0.5, 0.1])
    out = _filter(k0, k0, score=score)
    # 0 and 1 tie: both survive; 2 lies inside R0 of 0 and is beaten; 3 lies outside R0 of 0 (15.75 > R0) but inside R0 of nobody better
    assert 15.5 < R0 < 15.75
    assert out["seed"].tolist() == [True, True, False, True, False, True]
    # the ratio test is strict and the mutual flag counts for the seed itself and for whoever beats it
    out = _filter(k0, k0, score=np.array([0.64, 0.6399, 0.3, 0.3, 0.5, 0.1]), mnn=np.array([1, 1, 1, 1, 1, 0], bool))
    # 0 fails the ratio test and so beats nobody: 2 is a seed now and beats 1; 5 is not mutual: no seed, and it does not beat 4
    assert out["seed"].tolist() == [False, False, True, True, True, False]
    out = _filter(k0, k0, score=np.array([0.64, 0.6399, 0.3, 0.3, 0.5, 0.1]), mnn=np.array([1, 1, 1, 1, 1, 0], bool), conf={**OFF, "force_seed_mnn": False})
    assert out["seed"].tolist() == [False, False, True, True, False, True]


def test_neighbourhood_radius_and_threshold_strictness():
    rs = 4 * np.sqrt(240 * 320 / 100 / np.pi)  # 62.53...
    k0 = np.array([[100.0, 100], [162.5, 100], [162.75, 100], [100, 100 + 62.5], [110, 100]])
    score = np.array([0.1, 0.7, 0.7, 0.7, 0.7])  # only key-point 0 is a seed
    out = _filter(k0, k0, score=score)
    assert 62.5 < rs < 62.75 and out["members"][0].tolist() == [0, 1, 3, 4]  # (score, index) order, 162.75 is outside
    k1 = k0.copy()
    k1[4] = [100 + 62.75, 100]  # inside in image 0, outside in image 1
    assert _filter(k0, k1, score=score)["members"][0].tolist() == [0, 1, 3]
    # orientation: strict threshold, differences wrap at +-180; scale: strict on both sides
    o0 = np.zeros(5)
    o1 = np.array([170.0, -161, -160, 141, 140])  # relative to the seed: 0, 29, 30 (through the wrap), -29, -30
    conf = {"scale_rate_threshold": 10}
    out = _filter(k0, k0, score=score, conf=conf, o0=o0, o1=o1, s0=np.ones(5), s1=np.ones(5))
    assert out["members"][0].tolist() == [0, 1, 3]
    conf = {"orientation_difference_threshold": None, "scale_rate_threshold": 2}
    s1 = np.array([2.0, 4.0, 2.0, 1.0, 1.25])  # rels_s / rels_i = 1, 0.5 (= 1 / T: out), (outside), 2 (= T: out), 1.6
    assert _filter(k0, k0, score=score, conf=conf, s0=np.ones(5), s1=s1)["members"][0].tolist() == [0, 4]
    s1 = np.array([2.0, 3.9, 2.0, 1.1, 1.25])
    assert _filter(k0, k0, score=score, conf=conf, s0=np.ones(5), s1=s1)["members"][0].tolist() == [0, 1, 3, 4]
    assert R.wrap(np.array([180.0, -180, 179, 540, -181])).tolist() == [-180, -180, 179, -180, 179]
    assert R.wrap(np.array([180.0, 190.5], np.float32), np.float32).dtype == np.float32


def test_couple_enumeration_and_void_couples():
    c = R.couples(128)
    assert c[:6] == [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3)]
    assert set(c[:120]) == {(a, b) for b in range(16) for a in range(b)} and c[120:] == [(a, 16) for a in range(8)]
    assert R.couples(5) == [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3)]
    # n < 17: indices wrap, a couple that wraps onto itself is void, so is a degenerate one and one outside the scale-rate bounds
    xy = np.array([[0.1, 0, 0.1, 0], [0, 0.1, 0, 0.1], [0.2, 0, 0.2, 0], [0.1, 0.1, 0.7, 0.7]])
    n = len(xy)
    assert [(a % n, b % n) for a, b in c[6:10]] == [(0, 0), (1, 0), (2, 0), (3, 0)]
    assert R.hypothesis(0, 0, xy, R.DEFAULT_CONF, np.float64) is None
    assert R.hypothesis(0, 2, xy, R.DEFAULT_CONF, np.float64) is None  # collinear with the seed: det = 0
    assert np.allclose(R.hypothesis(0, 1, xy, R.DEFAULT_CONF, np.float64), (1, 0, 0, 1))
    assert R.hypothesis(0, 3, xy, R.DEFAULT_CONF, np.float64) is None  # det A = 7 > 5
    assert R.hypothesis(0, 3, xy, {**R.DEFAULT_CONF, "detected_scale_rate_threshold": None}, np.float64) is not None


def test_selection_duplicates_and_too_perfect():
    f = np.float64
    r2 = np.array([0.0, 1e-9, 0.0009, 0.0019, 0.0035, 0.0037, 0.02])
    w = np.ones(7, dtype=bool)
    acc, acc1, count, tot, mx = R.select(r2, w, f(200), f)
    # two too perfect members: accepted with weight 0; tot = 5; cum / tot = .2 .4 .6 .8 1 against r2 * 200 = .18 .38 .7 .74 4
    assert acc.tolist() == [True, True, True, True, False, True, False] and acc1.tolist() == [False, False, True, True, False, True, False]
    assert (count, tot, mx) == (3, 5, 0.0037)  # the test is per member, not prefix-closed: rank 3 fails, rank 4 passes
    w[3] = False  # a duplicate: weight 0; tot = 4, cum / tot = .25 .25 .5 .75 1
    acc, acc1, count, tot, mx = R.select(r2, w, f(200), f)
    assert acc.tolist() == [True, True, True, False, False, True, False] and (count, tot) == (2, 4)
    w[3], w[5] = True, False  # cum / tot = .25 .5 .75 .75 1: the duplicate passes its own test and is accepted, with weight 0
    acc, acc1, count, tot, mx = R.select(r2, w, f(200), f)
    assert acc.tolist() == [True] * 6 + [False] and acc1.tolist() == [False, False, True, True, True, False, False] and (count, tot, mx) == (3, 4, 0.0035)
    assert R.select(np.zeros(4), np.ones(4, bool), f(200), f)[2:4] == (0, 0)  # all too perfect: nothing counts
    # equal residuals are ranked by list position
    acc = R.select(np.array([0.003, 0.003, 0.003]), np.ones(3, bool), f(200), f)[0]
    assert acc.tolist() == [False, True, True]


def test_duplicate_members_carry_no_weight_and_noise_free_scene_is_rejected():
    sc = R.make_scene(0)
    a = R.stage_a(sc["d0"], sc["d1"])
    k0 = np.concatenate([sc["k0"], sc["k0"][:60]])
    k1 = np.concatenate([sc["k1"], sc["k1"][:60]])
    nn = np.concatenate([a["nn"], a["nn"][:60]])
    score = np.concatenate([a["score"], a["score"][:60]])
    mnn = np.concatenate([a["mnn"], np.zeros(60, bool)])
    base = R.filter_matches(sc["k0"], sc["k1"], None, None, None, None, a["nn"], a["score"], a["mnn"], SIZE, SIZE, OFF)
    dup = R.filter_matches(k0, k1, None, None, None, None, nn, score, mnn, SIZE, SIZE, OFF)
    assert np.array_equal(dup["seed"][:300], base["seed"]) and not dup["seed"][300:].any()
    assert np.array_equal(dup["count"][:300], base["count"]) and np.array_equal(dup["passed"][:300], base["passed"])  # weight 0: the counts do not move
    assert np.array_equal(dup["matches0"][:300], base["matches0"]) and np.array_equal(dup["matches0"][300:], base["matches0"][:60])
    # an exact similarity: every residual is too perfect, no weight is left and nothing is accepted
    k1 = (sc["k0"] - 100) * 2 + 300
    out = R.filter_matches(sc["k0"], k1, None, None, None, None, np.arange(300), np.full(300, 0.1), np.ones(300, bool), SIZE, SIZE,
                           {**OFF, "detected_scale_rate_threshold": None})  # fmt: skip
    assert out["seed"].any() and (out["n_members"] >= 6).any() and not out["passed"].any() and (out["matches0"] == -1).all()


def test_fewer_than_two_keypoints():
    sc = R.make_scene(3)
    for n0, n1 in ((1, 64), (64, 1), (0, 0)):
        out = R.match_and_filter(sc["k0"][:n0], sc["k1"][:n1], sc["d0"][:n0], sc["d1"][:n1], sc["o0"][:n0], sc["o1"][:n1], sc["s0"][:n0], sc["s1"][:n1],
                                 SIZE, SIZE)  # fmt: skip
        assert out["matches0"].shape == (n0,) and (out["matches0"] == -1).all() and not out["seed"].any()


@pytest.mark.parametrize("seed", sorted(R.SCENES))
def test_float32_against_float64_on_the_scenes(seed):
    """At most 1 % of a scene's key-points may differ between the two arithmetic modes (measured: 0 on all six)."""
    sc = R.make_scene(seed)
    a, b = R.run_scene(sc, np.float64), R.run_scene(sc, np.float32)
    N = len(sc["k0"])
    diff = int((a["matches0"] != b["matches0"]).sum())
    inl = ~sc["outlier"] & (a["nn"] == np.arange(N))
    kept = int(((a["matches0"] > -1) & sc["outlier"]).sum())
    print(f"scene {seed}: N {N}, {int(a['seed'].sum())} seeds, {int(a['passed'].sum())} neighbourhoods passed, {int((a['matches0'] > -1).sum())} matches; "
          f"{int((a['matches0'][inl] == np.arange(N)[inl]).sum())} of {int(inl.sum())} true NN matches accepted, {kept} of {int(sc['outlier'].sum())} planted outliers "
          f"kept; float32 differs on {diff} key-points")  # fmt: skip
    assert diff <= N // 100
    assert np.array_equal(a["seed"], b["seed"]) and np.array_equal(a["nn"], b["nn"])


def test_plugin_conf_required_inputs_and_refusals():
    import sys

    from imcui_hip import backend
    from imcui_hip.hloc.matchers import adalam
    from imcui_hip.hloc.utils.base_model import dynamic_load

    assert dynamic_load(sys.modules["imcui_hip.hloc.matchers"], "adalam") is adalam.AdaLAM
    assert adalam.AdaLAM.default_conf == R.DEFAULT_CONF
    assert adalam.AdaLAM.required_inputs == ["image0", "image1", "descriptors0", "descriptors1", "keypoints0", "keypoints1", "scales0", "scales1",
                                             "oris0", "oris1"]  # fmt: skip
    m = adalam.AdaLAM({"ransac_iters": 64})
    assert m.conf["ransac_iters"] == 64 and m.conf["area_ratio"] == 100 and m.add_scale_ori and len(list(m.buffers())) == 1
    assert list(backend.adalam_conf_array(m.conf)) == [100, 4, 64, 6, 200, 30, 1.5, 5, 1, 1]
    assert list(backend.adalam_conf_array({**m.conf, "scale_rate_threshold": None}))[6] == -1
    with pytest.raises(backend.ImcuiHipError, match="refit"):
        adalam.AdaLAM({"refit": None})
    k = torch.zeros(1, 8, 2)
    d = torch.zeros(1, 8, 128)
    n = torch.full((1,), 8, dtype=torch.int32)
    so = (torch.ones(1, 8),) * 4
    with pytest.raises(AttributeError, match="oris0"):
        m.forward_batched(k, k, d, d, n, n, (320, 240), (320, 240))
    with pytest.raises(AttributeError, match="scales0"):
        adalam.AdaLAM({"orientation_difference_threshold": None}).forward_batched(k, k, d, d, n, n, (320, 240), (320, 240), scales_oris=(None, so[1], None, so[3]))
    with pytest.raises(backend.ImcuiHipError, match="ROCm device"):  # no CPU fall-back
        m.forward_batched(k, k, d, d, n, n, (320, 240), (320, 240), scales_oris=so)
    with pytest.raises(AssertionError, match="oris1"):
        m({"image0": 0, "image1": 0, "descriptors0": 0, "descriptors1": 0, "keypoints0": 0, "keypoints1": 0, "scales0": 0, "scales1": 0, "oris0": 0})
    one = {"image0": torch.zeros(1, 1, 8, 8), "image1": torch.zeros(1, 1, 8, 8), "keypoints0": torch.zeros(1, 1, 2), "keypoints1": k,
           "descriptors0": torch.zeros(1, 128, 1), "descriptors1": d.transpose(2, 1), "scales0": torch.ones(1, 1), "scales1": so[0], "oris0": torch.ones(1, 1),
           "oris1": so[0]}  # fmt: skip
    out = m(one)  # adalam.py:41-44: fewer than two key-points, no launch
    assert out["matches0"].tolist() == [[-1]] and out["matches0"].dtype == torch.long and out["matching_scores0"].tolist() == [[0.0]]


def test_header_reader_finds_the_exports():
    import ctypes as C

    from imcui_hip import header

    fns = header.read().functions
    assert fns["imcui_hip_adalam_workspace_bytes"] == (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int])
    ret, args = fns["imcui_hip_adalam_forward"]
    assert ret is C.c_int and len(args) == 31 and args[:4] == [C.c_void_p, C.c_int, C.c_int, C.c_int] and args[14:18] == [C.c_int] * 4
    ret, args = fns["imcui_hip_adalam_filter"]
    assert ret is C.c_int and len(args) == 28 and args[-2] is C.c_size_t


def test_library_exports_and_workspace_query(lib):
    for name in ("imcui_hip_adalam_workspace_bytes", "imcui_hip_adalam_forward", "imcui_hip_adalam_filter"):
        assert hasattr(lib, name)
    small, full = lib.imcui_hip_adalam_workspace_bytes(None, 1, 4096, 0), lib.imcui_hip_adalam_workspace_bytes(None, 1, 4096, 128)
    assert 0 < small < full and lib.imcui_hip_adalam_workspace_bytes(None, 16, 4096, 128) > 15 * full // 2
    assert lib.imcui_hip_adalam_workspace_bytes(None, 1, 4097, 128) == 0 and lib.imcui_hip_adalam_workspace_bytes(None, 0, 16, 128) == 0
