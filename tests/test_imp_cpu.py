"""IMP without a GPU: the restatement against itself, the packer, the refusals, the synthetic calibration, the golden fixture and the
crafted assignment cases (whose expected outputs tests/test_gpu_imp_ot.py asks of the kernels)."""
import os

import numpy as np
import pytest
import torch

import imp_reference as R
from imcui_hip.synth_weights import imp_synth_state

SD = imp_synth_state(0)


def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-300)


def test_restatement_float32_against_float64():
    """The whole network in float32 against float64 on a margin-searched problem: equal matches, scores within the project's 1e-4."""
    torch.set_num_threads(4)
    net64 = R.oracle(SD, 20)
    data, ref = R.search_problem(net64, 40, 130, 257, 30, (20,))
    assert ref[20]["margin"] >= R.MIN_MARGIN and (ref[20]["matches0"] > -1).sum() > 10
    out = R.oracle(SD, 20, double=False).produce_matches(data)
    assert out["matching_scores0"].dtype == torch.float32
    for k in ("matches0", "matches1"):
        assert torch.equal(out[k], ref[20][k]), k
    for k in ("matching_scores0", "matching_scores1"):
        assert (out[k].double() - ref[20][k]).abs().max().item() < R.SCORE_BAR, k


@pytest.mark.parametrize("n,m", [(1, 1), (1, 7), (17, 16), (130, 257), (40, 600)])
@pytest.mark.parametrize("iters", [0, 1, 20])
def test_explicit_order_against_tensor_form(n, m, iters):
    """`sinkhorn_explicit` (the kernels' float32 order) against the float64 tensor form: u, v within 2e-6 of the largest entry -- both are
    float32 evaluations of the same sums (at most 600 terms, each rounding 6e-8), an order of magnitude above what either shows."""
    z, ref = R.search_scores(100, n, m, (iters,))
    ex = R.assign_explicit(z.numpy(), R.RANDOM_BIN, iters)
    r = ref[iters]
    assert _rel(ex["u"], r["u"]) < 2e-6 and _rel(ex["v"], r["v"]) < 2e-6
    assert torch.equal(ex["matches0"], r["matches0"]) and torch.equal(ex["matches1"], r["matches1"])
    assert (ex["matching_scores0"].double() - r["matching_scores0"]).abs().max().item() < 1e-6
    if iters == 0:
        assert (ex["u"] == 1).all() and (ex["v"] == 1).all()


def test_marginals_after_many_rounds():
    """100 rounds: the columns sum to c = [1] * m + [n] up to the epsilon of the last division (v s = c s / (s + eps): a relative 1e-8 / s,
    with column sums s above 1e-3 here, so 1e-5): the last half-round set them.  (The rows are still 0.4 % off r here: rival rows converge
    slowly, which is why the test of the kernels compares u and v themselves.)"""
    z, ref = R.search_scores(100, 17, 16, (100,))
    P = ref[100]["P"][0]
    assert (P.sum(0) / torch.tensor([1.0] * 16 + [17.0], dtype=torch.float64) - 1).abs().max() < 1e-5


def test_crafted_cases_have_the_expected_outputs():
    for name, (z, bin_score, iters, p, expected) in R.crafted_cases().items():
        r = R.assign(z[None].double(), bin_score, iters, p)
        ex = R.assign_explicit(z.numpy(), bin_score, iters, p)
        assert r["matches0"][0].tolist() == expected, name
        assert ex["matches0"][0].tolist() == expected, name
        assert torch.isfinite(ex["u"]).all() and torch.isfinite(ex["v"]).all(), name
        assert (ex["matching_scores0"].double() - r["matching_scores0"]).abs().max().item() < 1e-6, name
        m1 = r["matches1"][0]
        for i, j in enumerate(expected):
            assert j < 0 or m1[j] == i, name
    z, b, it, p, _ = R.crafted_cases()["constant"]
    r = R.assign(z[None].double(), b, it, p)
    assert r["matching_scores0"][0, 0] > p and (r["matching_scores0"][0, 1:] == 0).all()  # rows 1.. lose the tie for column 0
    z, b, it, p, _ = R.crafted_cases()["bin_dominates"]
    assert R.assign(z[None].double(), b, it, p)["matching_scores0"].max() < 1e-6
    z, b, it, p, _ = R.crafted_cases()["underflow_row"]
    pr, binc, u, v = R.sinkhorn_explicit(z.numpy(), b, it)
    assert (pr[2] == 0).all() and binc[2] == 1  # the real entries of row 2 underflowed


def test_score_equal_to_p_is_dropped():
    """The threshold is strict: with p set to a kept score (a float32 value) that match goes, with the next float32 below it stays."""
    z, b, it, _, expected = R.crafted_cases()["bin_minus30"]
    base = R.assign_explicit(z.numpy(), b, it, 0.2)
    s = base["matching_scores0"][0, 3]
    assert base["matches0"][0, 3] == expected[3] and s > 0.2
    at = R.assign_explicit(z.numpy(), b, it, float(s))
    assert at["matches0"][0, 3] == -1 and at["matching_scores0"][0, 3] == s and at["matches1"][0, expected[3]] == -1
    below = R.assign_explicit(z.numpy(), b, it, float(np.nextafter(np.float32(s), np.float32(0))))
    assert below["matches0"][0, 3] == expected[3]


def test_synthetic_weights_resolve_the_true_correspondences():
    """imp_synth_state is calibrated: at 20 rounds the float64 restatement recovers 100 % of the true correspondences at 60 x 55 (8
    outliers: 47 of 47), 130 x 257 (130 of 130) and 300 x 280 (60 outliers: 220 of 220), and matches no outlier of image 1; the
    test asks for at least 95 %."""
    torch.set_num_threads(4)
    net64 = R.oracle(SD, 20)
    for seed, n, m, n_out in ((5, 60, 55, 8), (6, 130, 257, 30), (7, 300, 280, 60)):
        data = R.problem(seed, n, m, n_out)
        out = net64.produce_matches(data)
        partner = data["partner"]
        true = partner >= 0
        got = (out["matches1"][0][true] == partner[true]).sum().item()
        assert got >= 0.95 * int(true.sum()), (n, m, got, int(true.sum()))
        assert (out["matches1"][0][~true] == -1).all(), (n, m)


def test_packer_round_trip(lib):
    """imcui_hip_imp_pack_weights: plain copies come back bit for bit, the folds within float32 round-off of the float64 fold."""
    from imcui_hip import backend

    table = backend.imp_tensor_table()
    assert len(table) == 335 and dict(table)["input_proj.weight"] == (256, 128, 1) and dict(table)["bin_score"] == ()
    assert set(n for n, _ in table) == {k for k in SD if not k.endswith("num_batches_tracked")}
    packed = backend.pack_imp(SD).numpy()
    assert packed.size == lib.imcui_hip_imp_packed_floats()

    def find(vec):
        v = vec.reshape(-1).numpy()
        hits = np.flatnonzero(packed[: packed.size - v.size + 1 : 64] == v[0]) * 64  # every packed tensor starts at a multiple of 64 floats
        return any(np.array_equal(packed[h : h + v.size], v) for h in hits)

    assert find(SD["input_proj.weight"]) and find(SD["input_proj.bias"])
    assert find(SD["final_proj.8.weight"]) and find(SD["final_proj.8.bias"]) and not find(SD["final_proj.3.weight"])
    assert find(SD["gnn.layers.17.mlp.3.weight"]) and find(SD["bin_score"].reshape(1))
    # BatchNorm folded into encoder layer 1 (32 -> 64)
    sc = SD["kenc.encoder.4.weight"].double() / torch.sqrt(SD["kenc.encoder.4.running_var"].double() + 1e-5)
    w = (SD["kenc.encoder.3.weight"][:, :, 0].double() * sc[:, None]).float()
    assert find(w)
    # heads de-interleaved: packed q row head * 64 + d = upstream row d * 4 + head
    q = SD["gnn.layers.0.attn.proj.0.weight"][:, :, 0]
    assert find(q.view(64, 4, 256).permute(1, 0, 2).reshape(256, 256)[:64].contiguous())


def test_refusals_name_their_reason(lib):
    from imcui_hip import backend
    from imcui_hip.lib_loader import ImcuiHipError

    bad = dict(SD)
    bad["gnn.layers.3.mlp.0.weight"] = torch.zeros(512, 256, 1)
    with pytest.raises(ImcuiHipError, match=r"gnn\.layers\.3\.mlp\.0\.weight.*\(512, 256, 1\).*\(512, 512, 1\)"):
        backend.pack_imp(bad)
    extra = dict(SD)
    extra["pos_enc.weight"] = torch.zeros(3)
    with pytest.raises(ImcuiHipError, match=r"pos_enc\.weight"):
        backend.pack_imp(extra)
    missing = {k: v for k, v in SD.items() if k != "final_proj.2.bias"}
    with pytest.raises(ImcuiHipError, match=r"lacks 'final_proj\.2\.bias'"):
        backend.pack_imp(missing)
    with pytest.raises(ImcuiHipError, match="AdaGML"):
        backend.pack_imp(SD, {"model_name": "imp_adagml.80.pth"})
    wide = dict(SD)
    wide["input_proj.weight"] = torch.zeros(256, 256, 1)
    with pytest.raises(ImcuiHipError, match="256-wide descriptors"):
        backend.pack_imp(wide)
    with pytest.raises(ImcuiHipError, match="n_layers=15"):
        backend.pack_imp(SD, {"n_layers": 15})
    with pytest.raises(ImcuiHipError, match="with_sinkhorn=False"):
        backend.pack_imp(SD, {"with_sinkhorn": False})


def test_golden_fixture_is_reproduced_by_the_restatement(golden_dir):
    """tests/golden/imp_golden.npz was written by the REFERENCE's wrapper around the restatement (make_imp_golden.py): the restatement
    alone, fed the stored inputs as the wrapper hands them over, gives the stored outputs -- matches equal, scores within 1e-6."""
    g = np.load(os.path.join(golden_dir, "imp_golden.npz"))
    net = R.oracle(SD, int(g["sinkhorn_iterations"]), double=False)
    net64 = R.oracle(SD, int(g["sinkhorn_iterations"]))
    for p in range(2):
        t = lambda k: torch.from_numpy(g[f"{k}_{p}"])
        (h0, w0), (h1, w1) = g[f"size0_{p}"], g[f"size1_{p}"]
        data = {"image0": torch.zeros(1, 1, int(h0), int(w0)), "image1": torch.zeros(1, 1, int(h1), int(w1)), "keypoints0": t("keypoints0"),
                "keypoints1": t("keypoints1"), "scores0": t("scores0"), "scores1": t("scores1"),
                "descriptors0": t("descriptors0").transpose(2, 1), "descriptors1": t("descriptors1").transpose(2, 1)}  # fmt: skip
        assert t("descriptors0").shape[1] == 128  # stored as the extractor writes them, [B, 128, N]
        out = net.produce_matches(data, p=0.2)
        full = net64.produce_matches(data, p=0.2, full=True)
        assert R.decision_margin(full["P"][0], 0.2) >= R.MIN_MARGIN and float(g[f"margin_{p}"]) >= R.MIN_MARGIN
        assert (t("matches0") > -1).sum() > 10
        for k in ("matches0", "matches1"):
            assert torch.equal(out[k], t(k)), (k, p)
        for k in ("matching_scores0", "matching_scores1"):
            assert (out[k] - t(k)).abs().max().item() < 1e-6, (k, p)
