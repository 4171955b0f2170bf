"""The assignment stage of IMP alone (imcui_hip_imp_ot_probe: dust-bin soft-max, probability-domain Sinkhorn rounds, mutual arg-max,
strict threshold) against the float64 restatement tests/imp_reference.py, on the GPU.

Bars.  Error of u and v (dust-bin entries included; all positive): the largest relative error of an entry, max |x - x64| / x64; their
entries span three orders of magnitude (a dust-bin scaling of 4000 next to rows of 70), so a norm relative to the largest entry would
measure the dust-bin alone.  Error of a score vector (zeros among them): max |x - x64| / max |x64|.  Each of the four vectors must stay
within

    3 x max(error of the float32 restatement on the same input for that vector, 2^-23)

The floor is one float32 ulp: the restatement's own error falls to 0 where a vector happens to be exact (u = v = 1 at 0 rounds, a
1 x 1 problem), while another valid float32 order of the same sums cannot be held below the format's resolution.  Matches: equal, on
matrices found by a seeded search (at most 40 seeds) for a float64 decision margin of at least 1e-3 (imp_reference.decision_margin).

Sizes: the issue's list plus one case either side of every boundary of the kernels: 16 rows per band (16 | 17), 256 columns per lane
chunk and 16 bands per merge group (255 | 256 | 257), 2048 columns per LDS fold (2048 | 2049), and the widest row the registers hold (4096).
"""
import pytest
import torch

import imp_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP = 2.0**-23
ROUNDS = (0, 1, 20, 100)
SIZES = [(1, 1), (1, 7), (2, 300), (17, 16), (16, 40), (130, 257), (255, 256), (256, 255), (257, 257), (33, 2048), (20, 2049), (18, 4096)]


def _impl():
    from imcui_hip import backend

    return backend.IMPHIP()


def _probe(z_list, bin_score, iters, p=0.2, ncap=None, impl=None):
    """z_list: per pair an [n, m] float32 matrix (or None for an empty pair) -> the probe's outputs on the CPU."""
    B = len(z_list)
    ncap = ncap or max(max(z.shape) for z in z_list if z is not None)
    sc = torch.zeros(B, ncap, ncap)
    n0, n1 = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for b, z in enumerate(z_list):
        if z is not None:
            sc[b, : z.shape[0], : z.shape[1]] = z
            n0[b], n1[b] = z.shape
    out = (impl or _impl()).ot_probe(sc.to(DEV), n0.to(DEV), n1.to(DEV), bin_score, iters, p)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _err(x, x64, entrywise):
    d = (x.double() - x64).abs()
    return (d / x64).max().item() if entrywise else d.max().item() / max(x64.abs().max().item(), 1e-300)


def _check(out, b, z, bin_score, iters, p, ref64, tag):
    """Pair b of `out` against the float64 result: u, v, scores within the bar, matches equal, everything beyond the counts -1 / 0."""
    n, m = z.shape
    ref32 = R.assign(z[None], bin_score, iters, p)
    got = {"u": out["u"][b, : n + 1], "v": out["v"][b, : m + 1], "matching_scores0": out["matching_scores0"][b, :n],
           "matching_scores1": out["matching_scores1"][b, :m]}  # fmt: skip
    for k, x in got.items():
        e32, e = _err(ref32[k][0], ref64[k][0], k in "uv"), _err(x, ref64[k][0], k in "uv")
        bar = 3 * max(e32, ULP)
        print(f"{tag} {k}: kernel {e:.3g}  float32 restatement {e32:.3g}  bar {bar:.3g}")
        assert torch.isfinite(x).all() and e <= bar, (tag, k, e, bar)
    assert torch.equal(out["matches0"][b, :n].long(), ref64["matches0"][0]), tag
    assert torch.equal(out["matches1"][b, :m].long(), ref64["matches1"][0]), tag
    assert (out["matches0"][b, n:] == -1).all() and (out["matches1"][b, m:] == -1).all(), tag
    assert (out["matching_scores0"][b, n:] == 0).all() and (out["matching_scores1"][b, m:] == 0).all(), tag


@pytest.mark.parametrize("n,m", SIZES)
def test_probe_against_float64(n, m):
    z, ref = R.search_scores(100, n, m, ROUNDS)
    impl = _impl()
    for it in ROUNDS:
        r = ref[it]
        assert r["margin"] >= R.MIN_MARGIN, (it, r["margin"])
        found = int((r["matches0"] > -1).sum())
        assert found > 10 or found == min(n, m), (it, found)
        _check(_probe([z], R.RANDOM_BIN, it, impl=impl), 0, z, R.RANDOM_BIN, it, 0.2, r, f"{n}x{m} rounds={it}")


@pytest.mark.parametrize("name", sorted(R.crafted_cases()))
def test_crafted_cases(name):
    """Ties to the lowest index, +-80 (the maximum is subtracted), a dominating dust-bin, a dust-bin of -30, a row whose real entries
    underflow: the expected matches of tests/test_imp_cpu.py, scores and scalings within the bar."""
    z, bin_score, iters, p, expected = R.crafted_cases()[name]
    ref = R.assign(z[None].double(), bin_score, iters, p)
    assert ref["matches0"][0].tolist() == expected
    out = _probe([z], bin_score, iters, p)
    assert out["matches0"][0, : z.shape[0]].tolist() == expected
    _check(out, 0, z, bin_score, iters, p, ref, name)


def test_score_equal_to_p_is_dropped():
    z, b, it, _, expected = R.crafted_cases()["bin_minus30"]
    base = _probe([z], b, it, 0.2)
    s = base["matching_scores0"][0, 3]
    assert base["matches0"][0, 3] == expected[3] and s > 0.2
    at = _probe([z], b, it, float(s))  # p is compared as a float32, like `tensor > p`
    assert at["matches0"][0, 3] == -1 and at["matching_scores0"][0, 3] == s and at["matches1"][0, expected[3]] == -1
    below = _probe([z], b, it, float(torch.nextafter(s, torch.tensor(0.0))))
    assert below["matches0"][0, 3] == expected[3] and below["matches1"][0, expected[3]] == 3


def test_batch_of_three_with_an_empty_pair():
    za, ra = R.search_scores(100, 130, 257, (20,))
    zc, rc = R.search_scores(100, 17, 16, (20,))
    out = _probe([za, None, zc], R.RANDOM_BIN, 20)
    _check(out, 0, za, R.RANDOM_BIN, 20, 0.2, ra[20], "slot 0")
    _check(out, 2, zc, R.RANDOM_BIN, 20, 0.2, rc[20], "slot 2")
    assert (out["matches0"][1] == -1).all() and (out["matches1"][1] == -1).all()
    assert (out["matching_scores0"][1] == 0).all() and (out["matching_scores1"][1] == 0).all()
    swapped = _probe([zc, za, None], R.RANDOM_BIN, 20)  # an empty second side, other slots
    for k in out:
        assert torch.equal(swapped[k][1], out[k][0]) and torch.equal(swapped[k][0], out[k][2]), k
    assert (swapped["matches0"][2] == -1).all() and (swapped["matching_scores1"][2] == 0).all()


def test_alone_in_a_batch_and_in_a_graph_replay_equal_bits():
    from imcui_hip import backend

    za, _ = R.search_scores(100, 130, 257, (20,))
    zb, _ = R.search_scores(100, 257, 257, (20,))
    zc, _ = R.search_scores(100, 17, 16, (20,))
    impl = _impl()
    batch = _probe([zb, zc, za], R.RANDOM_BIN, 20, ncap=300, impl=impl)
    alone = _probe([za], R.RANDOM_BIN, 20, ncap=300, impl=impl)
    for k in batch:
        assert torch.equal(alone[k][0], batch[k][2]), k
    sc = torch.zeros(3, 300, 300)
    for b, z in enumerate((zb, zc, za)):
        sc[b, : z.shape[0], : z.shape[1]] = z
    sc = sc.to(DEV)
    n0 = torch.tensor([257, 17, 130], dtype=torch.int32, device=DEV)
    n1 = torch.tensor([257, 16, 257], dtype=torch.int32, device=DEV)
    table = {}
    with backend.workspace_owner(table):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            impl.ot_probe(sc, n0, n1, R.RANDOM_BIN, 20)  # warm-up: allocates the graph-owned workspace
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = impl.ot_probe(sc, n0, n1, R.RANDOM_BIN, 20)
    for _ in range(2):
        for v in cap.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in batch:
            assert torch.equal(batch[k], cap[k].cpu()), k


def test_refusals():
    from imcui_hip import backend

    hd = backend.get_handle(torch.device(DEV))
    lib = hd.lib
    t = torch.zeros(1, device=DEV)
    i = torch.zeros(1, dtype=torch.int32, device=DEV)
    P = backend._ptr
    args = lambda ncap, iters, ws: (P(t), 1, ncap, P(i), P(i), 0.0, iters, 0.2, P(i), P(i), P(t), P(t), None, None, P(t) if ws else None, 4 if ws else 0)
    assert hd.launch(lib.imcui_hip_imp_ot_probe, *args(4097, 1, True), check=False) == -1  # wider than the registers hold
    assert b"4096" in lib.imcui_hip_last_error(hd.h)
    assert hd.launch(lib.imcui_hip_imp_ot_probe, *args(4, -1, True), check=False) == -1
    assert hd.launch(lib.imcui_hip_imp_ot_probe, *args(4, 1, True), check=False) == -2  # workspace too small
    assert lib.imcui_hip_imp_workspace_bytes(2, 4096) > 2 * 4096 * 4096 * 4
