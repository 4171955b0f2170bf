"""LISRD's matcher kernel (csrc/lisrd.hip, `backend.lisrd_match`) alone, against the float64 einsum form of the wrapper's
`_lisrd_matcher` / `_compute_confidence` (imcui/hloc/matchers/lisrd.py:122-149), restated here (GPU box only).

Bars.  A value bar is 3 x the error of the float32 torch restatement on the same input against float64, floored at 1.8e-07 (three
float32 ulps of 1 / 2), plus 2e-6 (exact f32) / 4e-6 (3 x f16 split) for the matrix-core products -- the project's convention for a
launch on the matrix cores.  Indices must agree with float64 except where its top-2 gap is below 1e-5 (the figure of
tests/test_gpu_simred.py; |similarity| <= 1 here), and such rows plus columns may be at most 2 % of all of them.
Every test prints its figures before it asserts."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1.8e-07
SHAPES = [(1, 1, 1), (1, 1, 5), (2, 127, 130), (1, 128, 128), (2, 129, 130), (2, 300, 260)]


def unit(g, *shape):
    x = torch.randn(*shape, generator=g)
    return x / x.norm(dim=-1, keepdim=True)


def problem(seed, B, N, M, Dm):
    g = torch.Generator().manual_seed(seed)
    return unit(g, B, N, 4, 128), unit(g, B, N, 4, Dm), unit(g, B, M, 4, 128), unit(g, B, M, 4, Dm)


def counts(B, N, M):
    """device-side counts below the static sizes (batch 0), and the full size in the last batch entry"""
    c0 = [max(1, N - 3 - 5 * b) for b in range(B)]
    c1 = [max(1, M - 2 - 7 * b) for b in range(B)]
    c0[-1], c1[-1] = (N, M) if B > 1 else (c0[-1], c1[-1])
    return c0, c1


def sims(d0, m0, d1, m1, dtype):
    """`_lisrd_matcher`'s similarity, [B, N, M]: the materialised einsum form"""
    d0, m0, d1, m1 = (t.to(dtype) for t in (d0, m0, d1, m1))
    w = torch.softmax(torch.einsum("bnid,bmid->bnim", m0, m1), dim=2)
    return (torch.einsum("bnid,bmid->bnim", d0, d1) * w).sum(2)


def confidence(d0, d1, m0, m1, dtype):
    """`_compute_confidence` on matched rows [P, 4, D]"""
    nz = lambda t: torch.nn.functional.normalize(t.to(dtype), dim=2)
    return ((nz(d0) * nz(d1)).sum(2) * torch.softmax((nz(m0) * nz(m1)).sum(2), dim=1)).sum(1)


def run(d0, m0, d1, m1, c0=None, c1=None):
    from imcui_hip import backend

    t = lambda c: None if c is None else torch.tensor(c, dtype=torch.int32, device=DEV)
    out = backend.lisrd_match(d0.to(DEV), m0.to(DEV), d1.to(DEV), m1.to(DEV), t(c0), t(c1), want_nn=True)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def value_bar(precision, ref32, ref64):
    return max(3.0 * float((ref32.double() - ref64).abs().max()), FLOOR) + (4e-6 if precision == 1 else 2e-6)


def check_against_f64(precision, tensors, c0, c1, out, what):
    d0, m0, d1, m1 = tensors
    B, N, M = d0.shape[0], d0.shape[1], d1.shape[1]
    s64, s32 = sims(*tensors, torch.float64), sims(*tensors, torch.float32)
    loose = total = 0
    for b in range(B):
        n, m = c0[b], c1[b]
        r, r32 = s64[b, :n, :m], s32[b, :n, :m]
        bar = value_bar(precision, r32, r)
        # rows
        top = r.topk(min(2, m), dim=1)
        err = float((out["best0"][b, :n].double() - top.values[:, 0]).abs().max())
        cerr = float((out["best1"][b, :m].double() - r.max(0).values).abs().max())
        print(f"{what} b={b} {n}x{m}: row-best error {err:.3g}, column-best error {cerr:.3g}, bar {bar:.3g}")
        assert err <= bar and cerr <= bar
        for idx, mat in ((out["nn12"][b, :n].long(), r), (out["nn21"][b, :m].long(), r.t())):
            t2 = mat.topk(min(2, mat.shape[1]), dim=1)
            agree = idx == t2.indices[:, 0]
            if not bool(agree.all()):
                gap = (t2.values[:, 0] - t2.values[:, 1])[~agree]
                print(f"  {int((~agree).sum())} indices differ, largest float64 top-2 gap among them {float(gap.max()):.3g}")
                assert float(gap.max()) < 1e-5
            loose += int((~agree).sum())
            total += idx.numel()
        # past the counts
        assert bool((out["nn12"][b, n:] == -1).all()) and bool((out["nn21"][b, m:] == -1).all()) and bool((out["best1"][b, m:] == 0).all())
        assert bool((out["matches0"][b, n:] == -1).all()) and bool((out["best0"][b, n:] == 0).all()) and bool((out["mconf"][b, n:] == 0).all())
    print(f"{what}: {loose} of {total} rows + columns resolved a near tie differently ({100.0 * loose / total:.2f} %)")
    assert loose <= 0.02 * total


def check_mutual_and_conf(tensors, out):
    d0, m0, d1, m1 = tensors
    B, N = d0.shape[:2]
    for b in range(B):
        nn12, nn21 = out["nn12"][b].long(), out["nn21"][b].long()
        ids = torch.arange(N)
        ok = (nn12 >= 0) & (nn21[nn12.clamp(min=0)] == ids)
        assert torch.equal(out["matches0"][b].long(), torch.where(ok, nn12, torch.full_like(nn12, -1)))  # the device's own arg-maxima, bit for bit
        i, j = ids[ok], nn12[ok]
        if i.numel():
            c64 = confidence(d0[b, i], d1[b, j], m0[b, i], m1[b, j], torch.float64)
            c32 = confidence(d0[b, i], d1[b, j], m0[b, i], m1[b, j], torch.float32)
            bar = max(3.0 * float((c32.double() - c64).abs().max()), FLOOR)
            err = float((out["mconf"][b, i].double() - c64).abs().max())
            print(f"  b={b}: {i.numel()} matches, mconf error {err:.3g}, bar {bar:.3g}")
            assert err <= bar
        assert bool((out["mconf"][b, ~ok] == 0).all())


@pytest.mark.parametrize("Dm", [128, 1024])
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_against_float64(precision, Dm, B, N, M):
    tensors = problem(Dm + 7 * N + M, B, N, M, Dm)
    c0, c1 = counts(B, N, M)
    out = run(*tensors, c0, c1)
    check_against_f64(precision, tensors, c0, c1, out, f"Dm={Dm}")
    check_mutual_and_conf(tensors, out)


def test_without_counts_and_middle_width(precision):
    """null counts = the static sizes; Dm = 384 (a multiple of 128 that is no power of two)"""
    B, N, M = 1, 70, 65
    tensors = problem(5, B, N, M, 384)
    out = run(*tensors)
    check_against_f64(precision, tensors, [N], [M], out, "Dm=384")
    check_mutual_and_conf(tensors, out)


def test_first_index_wins(precision):
    """identical key-points in two columns (one tile, another tile, another chunk) and in two rows (another row block): bitwise equal
    similarities, and the FIRST index is the arg-max in every merge"""
    B, N, M = 1, 300, 260
    d0, m0, d1, m1 = problem(11, B, N, M, 128)
    cols = [(3, 9), (20, 70), (41, 200), (64, 259)]
    rows = [(5, 6), (10, 130), (127, 299)]
    for a, c in cols:
        d1[0, c], m1[0, c] = d1[0, a], m1[0, a]
    for a, c in rows:
        d0[0, c], m0[0, c] = d0[0, a], m0[0, a]
    out = run(d0, m0, d1, m1)
    s64 = sims(d0, m0, d1, m1, torch.float64)[0]
    hit = 0
    for (first, second), idx, ref in [(p, out["nn12"][0], s64.argmax(1)) for p in cols] + [(p, out["nn21"][0], s64.argmax(0)) for p in rows]:
        assert not bool((idx == second).any()), (first, second)
        hit += int(((ref == first) | (ref == second)).sum())
        both = (ref == first) | (ref == second)
        assert bool((idx[both] == first).all())
    print(f"first-index case: {hit} rows / columns have a duplicated key-point as their float64 best")
    assert hit >= len(cols) + len(rows) - 2  # the case is not vacuous


def test_equal_meta_products_weigh_a_quarter(precision):
    """the same meta vector under all four variances: four bitwise equal meta products, weights exactly 1/4.  The local descriptors are
    one-hot, so every local product is 0 or 1 in either arithmetic and the similarity is EXACTLY count / 4"""
    B, N, M = 1, 130, 70
    g = torch.Generator().manual_seed(3)
    m0 = unit(g, B, N, 1, 256).expand(B, N, 4, 256).contiguous()
    m1 = unit(g, B, M, 1, 256).expand(B, M, 4, 256).contiguous()
    d0, d1 = torch.zeros(B, N, 4, 128), torch.zeros(B, M, 4, 128)
    d0.scatter_(3, torch.randint(0, 3, (B, N, 4, 1), generator=g), 1.0)
    d1.scatter_(3, torch.randint(0, 3, (B, M, 4, 1), generator=g), 1.0)
    out = run(d0, m0, d1, m1)
    exact = torch.einsum("nid,mid->nm", d0[0].double(), d1[0].double()) / 4.0  # quarters: exact in float32
    print("equal meta products: similarities", sorted(set(exact.flatten().tolist())), "row maxima", sorted(set(exact.max(1).values.tolist())))
    assert len(set(exact.max(1).values.tolist())) > 1  # (rows whose best is 3 / 4 as well as rows whose best is 1)
    assert torch.equal(out["best0"][0].double(), exact.max(1).values)
    # FIRST index among the (many) exactly equal similarities
    first_r = (exact == exact.max(1, keepdim=True).values).double().argmax(1)
    first_c = (exact == exact.max(0, keepdim=True).values).double().argmax(0)
    assert torch.equal(out["nn12"][0].long(), first_r) and torch.equal(out["nn21"][0].long(), first_c)


def test_dominating_meta_product(precision):
    """one meta product 80 above the other three: its weight is 1 (the others underflow towards exp(-80)), nothing is NaN"""
    B, N, M = 1, 40, 33
    d0, m0, d1, m1 = problem(17, B, N, M, 128)
    u = torch.zeros(128)
    u[5] = 1.0
    w = torch.zeros(128)
    w[9] = 1.0
    m0[:], m1[:] = w, u  # orthogonal: products 0 ...
    m0[:, :, 2], m1[:, :, 2] = 80.0 * u, u  # ... but variance 2: exactly 80
    out = run(d0, m0, d1, m1)
    ref = torch.einsum("nd,md->nm", d0[0, :, 2].double(), d1[0, :, 2].double())
    s32 = torch.einsum("nd,md->nm", d0[0, :, 2], d1[0, :, 2])
    bar = value_bar(precision, s32, ref)
    err = float((out["best0"][0].double() - ref.max(1).values).abs().max())
    print(f"dominating meta product: row-best error {err:.3g} against the variance's own product, bar {bar:.3g}")
    assert bool(torch.isfinite(out["best0"]).all()) and bool(torch.isfinite(out["mconf"]).all())
    assert err <= bar
    check_mutual_and_conf((d0, m0, d1, m1), out)


def test_batch_independence_and_graph_replay(precision):
    from imcui_hip import backend

    B, N, M, Dm = 3, 140, 150, 256
    tensors = [t.to(DEV) for t in problem(23, B, N, M, Dm)]
    c0 = torch.tensor([140, 97, 129], dtype=torch.int32, device=DEV)
    c1 = torch.tensor([150, 64, 131], dtype=torch.int32, device=DEV)
    eager = backend.lisrd_match(*tensors, c0, c1, want_nn=True)
    for b in range(B):
        solo = backend.lisrd_match(*(t[b : b + 1] for t in tensors), c0[b : b + 1].contiguous(), c1[b : b + 1].contiguous(), want_nn=True)
        for k, v in solo.items():
            assert torch.equal(v[0], eager[k][b]), (k, b)
    table = {}
    with backend.workspace_owner(table):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            backend.lisrd_match(*tensors, c0, c1, want_nn=True)  # warm-up: allocates the graph-owned workspace
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = backend.lisrd_match(*tensors, c0, c1, want_nn=True)
    for _ in range(2):
        for v in cap.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(eager[k], cap[k]), k


def test_refusals(precision):
    from imcui_hip import backend
    from imcui_hip.lib_loader import ImcuiHipError

    d0, m0, d1, m1 = (t.to(DEV) for t in problem(1, 1, 4, 5, 128))
    with pytest.raises(ImcuiHipError, match="multiple of 128"):
        backend.lisrd_match(d0, m0[..., :64], d1, m1[..., :64])
    with pytest.raises(ImcuiHipError, match="do not belong together"):
        backend.lisrd_match(d0, m0, d1[:, :, :3], m1)
    hd = backend.get_handle(torch.device(DEV))
    rc = hd.launch(hd.lib.imcui_hip_lisrd_match, None, None, None, None, None, None, 1, 4, 5, 128, None, None, None, None, None, None, None, 0, check=False)
    assert rc == -1
    assert hd.lib.imcui_hip_lisrd_match_workspace_bytes(1, 4, 5, 100) == 0
