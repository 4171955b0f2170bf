"""AdaLAM restated in numpy: the rule of INTEGRATION.md, "AdaLAM: what is pinned" (stages A .. G), which csrc/adalam.hip implements.

Two arithmetic modes: `np.float64` is the oracle, `np.float32` follows the kernel's operation order (every multiply, add and divide
rounds on its own; sums of the refit are the kernel's fixed tree) so that its decisions can be compared by equality.  The one thing
the float32 mode does not mirror is the summation order of the descriptor dot products on the matrix cores: on integer descriptors
(every test that demands equal bits of stage A) any order is exact.

Nothing here is drawn at random: the sample couples are enumerated.  Every intermediate that the library's probes expose is returned.
"""
from __future__ import annotations

import math

import numpy as np

DEFAULT_CONF = {
    "area_ratio": 100,
    "search_expansion": 4,
    "ransac_iters": 128,
    "min_inliers": 6,
    "min_confidence": 200,
    "orientation_difference_threshold": 30,
    "scale_rate_threshold": 1.5,
    "detected_scale_rate_threshold": 5,
    "refit": True,
    "force_seed_mnn": True,
}
MIN_WIDTH = 64  # narrowest tree of the refit sums (AL_MINP of the kernel)


# ------------------------------------------------------------------ A: putative matches
def sq_norms(d, dtype):
    """|d_i|^2, k ascending."""
    d = np.asarray(d, dtype=dtype)
    s = np.zeros(d.shape[0], dtype=dtype)
    for k in range(d.shape[1]):
        s = s + d[:, k] * d[:, k]
    return s


def stage_a(d0, d1, dtype=np.float64):
    """nn, score, mnn (+ dist, d2nd, nn21) of descriptors d0 [n0, D], d1 [n1, D]; n0 < 2 or n1 < 2: everything unmatched."""
    n0, n1 = len(d0), len(d1)
    if n0 < 2 or n1 < 2:
        return {"nn": np.full(n0, -1, dtype=np.int64), "score": np.zeros(n0, dtype=dtype), "mnn": np.zeros(n0, dtype=bool)}
    d0, d1 = np.asarray(d0, dtype=dtype), np.asarray(d1, dtype=dtype)
    rn, cn = sq_norms(d0, dtype), sq_norms(d1, dtype)
    dist = (rn[:, None] - dtype(2) * (d0 @ d1.T)) + cn[None, :]  # the kernel's (2 a.b - |a|^2) - |b|^2, negated
    nn = dist.argmin(1)  # lowest index on equal minima
    part = np.partition(dist, 1, axis=1)
    best, second = part[:, 0], part[:, 1]
    score = best / np.maximum(second, dtype(1e-3))
    nn21 = dist.argmin(0)
    mnn = nn21[nn] == np.arange(n0)
    return {"nn": nn.astype(np.int64), "score": score.astype(dtype), "mnn": mnn, "dist": best, "d2nd": second, "nn21": nn21}


# ------------------------------------------------------------------ helpers of C .. G
def wrap(v, dtype=np.float64):
    """Degrees into [-180, 180)."""
    v = np.asarray(v, dtype=dtype)
    return v - dtype(360) * np.floor((v + dtype(180)) / dtype(360))


def couples(iters: int):
    """b-major enumeration: (0,1), (0,2), (1,2), (0,3), ..."""
    out, b = [], 1
    while len(out) < iters:
        for a in range(b):
            out.append((a, b))
            if len(out) == iters:
                break
        b += 1
    return out


def radii(size, conf):
    """(R^2, R * search_expansion, (R * search_expansion)^2) of an image of size (H, W), in double."""
    H, W = size
    R = math.sqrt(float(H) * float(W) / float(conf["area_ratio"]) / math.pi)
    rs = R * float(conf["search_expansion"])
    return R * R, rs, rs * rs


def _width(n):
    p = MIN_WIDTH
    while p < n:
        p <<= 1
    return p


def tree_sum(terms, flags, P, dtype):
    """Sum of terms[flags] over P slots as the kernel's tree: f[t] += f[t + s], s = P / 2 .. 1."""
    f = np.zeros(P, dtype=dtype)
    f[: len(terms)] = np.where(flags, terms, dtype(0))
    while len(f) > 1:
        h = len(f) // 2
        f = f[:h] + f[h:]
    return f[0]


def residuals(A, xy, dtype):
    ex = (A[0] * xy[:, 0] + A[1] * xy[:, 1]) - xy[:, 2]
    ey = (A[2] * xy[:, 0] + A[3] * xy[:, 1]) - xy[:, 3]
    return (ex * ex + ey * ey).astype(dtype)


def select(r2, wdup, min_conf, dtype):
    """Stage E for one hypothesis -> (accepted [n] bool, weight-1 accepted [n] bool, count, tot, max r^2 over the weight-1 accepted)."""
    tp = r2 <= dtype(1e-8)
    w = wdup & ~tp
    order = np.argsort(r2, kind="stable")  # (r^2, list position)
    cum = np.cumsum(w[order])
    tot = int(w.sum())
    acc_sorted = tp[order].copy()
    if tot > 0:
        with np.errstate(invalid="ignore"):
            acc_sorted |= r2[order] * dtype(min_conf) <= cum.astype(dtype) / dtype(tot)
    acc = np.zeros(len(r2), dtype=bool)
    acc[order] = acc_sorted
    acc1 = acc & w
    count = int(acc1.sum())
    return acc, acc1, count, tot, (r2[acc1].max() if count else dtype(0))


def hypothesis(a, b, xy, conf, dtype):
    """The affine map through members a, b as (a00, a01, a10, a11), or None when the hypothesis is void."""
    if a == b:
        return None
    pa, pb = xy[a], xy[b]
    det = pa[0] * pb[1] - pb[0] * pa[1]
    if abs(det) < dtype(1e-8):
        return None
    with np.errstate(all="ignore"):
        A = (
            (pa[2] * pb[1] - pb[2] * pa[1]) / det,
            (pb[2] * pa[0] - pa[2] * pb[0]) / det,
            (pa[3] * pb[1] - pb[3] * pa[1]) / det,
            (pb[3] * pa[0] - pa[3] * pb[0]) / det,
        )
        dt = conf["detected_scale_rate_threshold"]
        if dt is not None:
            da = A[0] * A[3] - A[1] * A[2]
            if not (da >= dtype(1.0 / float(dt)) and da <= dtype(dt)):
                return None
    return A


# ------------------------------------------------------------------ B .. G
def filter_matches(k0, k1, o0, o1, s0, s1, nn, score, mnn, size0, size1, conf=None, dtype=np.float64):
    """Stages B .. G from given putative matches.  k0 [n0,2], k1 [n1,2] pixels; o / s may be None while their test is off; sizes (H, W).
    Returns matches0 [n0] (-1 = unmatched), seed [n0] bool and, per key-point slot, members (dict seed -> key-point indices in
    (score, index) order), n_members, best_iter (-1 = none), count, conf, passed."""
    conf = {**DEFAULT_CONF, **(conf or {})}
    f = dtype
    n0, n1 = len(k0), len(k1)
    out = {
        "matches0": np.full(n0, -1, dtype=np.int64),
        "seed": np.zeros(n0, dtype=bool),
        "members": {},
        "n_members": np.zeros(n0, dtype=np.int64),
        "best_iter": np.full(n0, -1, dtype=np.int64),
        "count": np.zeros(n0, dtype=np.int64),
        "conf": np.zeros(n0, dtype=dtype),
        "passed": np.zeros(n0, dtype=bool),
    }
    if n0 < 2 or n1 < 2:
        return out
    k0, k1 = np.asarray(k0, dtype=f), np.asarray(k1, dtype=f)
    nn = np.asarray(nn, dtype=np.int64)
    score = np.asarray(score, dtype=f)
    mnn = np.asarray(mnn).astype(bool)
    valid = (nn >= 0) & (nn < n1)
    nnc = np.where(valid, nn, 0)
    r0sq, rs0, nb0sq = radii(size0, conf)
    _, rs1, nb1sq = radii(size1, conf)
    ot, st = conf["orientation_difference_threshold"], conf["scale_rate_threshold"]
    use_ori = ot is not None and float(ot) < 180.0
    use_sc = st is not None and float(st) < 10.0
    force = bool(conf["force_seed_mnn"])
    iters, min_inl, min_conf = int(conf["ransac_iters"]), int(conf["min_inliers"]), f(conf["min_confidence"])

    # ---- B
    elig = valid & (mnn if force else True)
    cand = elig & (score < f(0.8 * 0.8))
    dx = k0[:, None, 0] - k0[None, :, 0]
    dy = k0[:, None, 1] - k0[None, :, 1]
    d2 = dx * dx + dy * dy
    beaten = ((d2 < f(r0sq)) & (score[:, None] > score[None, :]) & elig[None, :]).any(1)
    seed = cand & ~beaten
    out["seed"] = seed

    # ---- C
    p = k1[nnc]
    relo = wrap(np.asarray(o1, dtype=f)[nnc] - np.asarray(o0, dtype=f), f) if use_ori else np.zeros(n0, dtype=f)
    rels = np.asarray(s1, dtype=f)[nnc] / np.asarray(s0, dtype=f) if use_sc else np.ones(n0, dtype=f)
    order = np.lexsort((np.arange(n0), score))
    order = order[valid[order]]
    cps = couples(iters)
    for s in np.flatnonzero(seed):
        i = order
        dx, dy = k0[i, 0] - k0[s, 0], k0[i, 1] - k0[s, 1]
        ex, ey = p[i, 0] - p[s, 0], p[i, 1] - p[s, 1]
        inn = (dx * dx + dy * dy < f(nb0sq)) & (ex * ex + ey * ey < f(nb1sq))
        if use_ori:
            inn &= np.abs(wrap(relo[i] - relo[s], f)) < f(ot)
        if use_sc:
            q = rels[s] / rels[i]
            inn &= (q > f(1.0 / float(st))) & (q < f(st))
        mem = i[inn]
        n = len(mem)
        out["members"][int(s)] = mem
        out["n_members"][s] = n
        if n < min_inl:
            continue
        xy = np.stack([dx[inn] / f(rs0), dy[inn] / f(rs0), ex[inn] / f(rs1), ey[inn] / f(rs1)], axis=1).astype(f)
        # duplicates: the four local coordinates bit-equal to an earlier member's
        _, first = np.unique(xy.view(np.uint32 if f == np.float32 else np.uint64).reshape(n, 4), axis=0, return_index=True)
        wdup = np.zeros(n, dtype=bool)
        wdup[first] = True
        # ---- D, E
        best_it, best_cnt = -1, 0
        for it, (a, b) in enumerate(cps):
            A = hypothesis(a % n, b % n, xy, conf, f)
            if A is None:
                continue
            cnt = select(residuals(A, xy, f), wdup, min_conf, f)[2]
            if cnt > best_cnt:
                best_it, best_cnt = it, cnt
        out["best_iter"][s] = best_it
        if best_it < 0:
            continue
        a, b = cps[best_it]
        A = hypothesis(a % n, b % n, xy, conf, f)
        acc, acc1, count, tot, mx = select(residuals(A, xy, f), wdup, min_conf, f)
        if conf["refit"]:
            # ---- F
            P = _width(n)
            x0, x1, y0, y1 = xy[:, 0], xy[:, 1], xy[:, 2], xy[:, 3]
            sxx, sxy, syy = tree_sum(x0 * x0, acc1, P, f), tree_sum(x0 * x1, acc1, P, f), tree_sum(x1 * x1, acc1, P, f)
            c00, c01 = tree_sum(y0 * x0, acc1, P, f), tree_sum(y0 * x1, acc1, P, f)
            c10, c11 = tree_sum(y1 * x0, acc1, P, f), tree_sum(y1 * x1, acc1, P, f)
            det = sxx * syy - sxy * sxy
            if not (count >= 2 and det >= f(1e-12)):
                continue
            A = ((c00 * syy - c01 * sxy) / det, (c01 * sxx - c00 * sxy) / det, (c10 * syy - c11 * sxy) / det, (c11 * sxx - c10 * sxy) / det)
            acc, acc1, count, tot, mx = select(residuals(A, xy, f), wdup, min_conf, f)
        # ---- G
        if count == 0:
            continue
        c = f(count) / (f(tot) * mx)
        passed = bool(c >= min_conf and f(count) * (f(1) - f(1) / c) >= f(min_inl))
        out["count"][s], out["conf"][s], out["passed"][s] = count, c, passed
        if passed:
            out["matches0"][mem[acc]] = nn[mem[acc]]
    return out


def match_and_filter(k0, k1, d0, d1, o0, o1, s0, s1, size0, size1, conf=None, dtype=np.float64):
    a = stage_a(d0, d1, dtype)
    out = filter_matches(k0, k1, o0, o1, s0, s1, a["nn"], a["score"], a["mnn"], size0, size1, conf, dtype)
    out.update(nn=a["nn"], score=a["score"], mnn=a["mnn"])
    return out


# ------------------------------------------------------------------ the scenes of the tests
SIZE = (240, 320)  # (H, W)
SCENES = {0: (300, 0.5, 0.3, True), 1: (1000, 0.5, 0.4, False), 2: (128, 0.5, 0.4, False), 3: (64, 0.25, 0.2, True), 4: (600, 1.0, 0.5, False),
          5: (2000, 0.5, 0.4, False)}  # seed -> (N, sigma, planted outlier share, relative tests on)  # fmt: skip
FILTERS_OFF = {"orientation_difference_threshold": 180, "scale_rate_threshold": 10}


def make_scene(seed, N=None, sigma=None, p=None, filters=None, D=128):
    """One seeded scene: key-points of image 0 under a similarity (scale 1.2, rotation 10 degrees about the centre) + noise, a share
    `p` of planted outliers; integer descriptors (exact in both arithmetic modes).  Returns a dict with float64 / int arrays and the conf
    overrides that switch the relative tests off where the scene has them off."""
    dN, dsig, dp, dfil = SCENES.get(seed, (300, 0.5, 0.3, True))
    N, sigma, p, filters = dN if N is None else N, dsig if sigma is None else sigma, dp if p is None else p, dfil if filters is None else filters
    rng = np.random.default_rng(seed)
    H, W = SIZE
    q = lambda v: np.round(v * 4) / 4  # noqa: E731  quarter pixels
    k0 = q(np.stack([rng.uniform(8, W - 8, N), rng.uniform(8, H - 8, N)], axis=1))
    th = math.radians(10.0)
    R = 1.2 * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    c = np.array([W / 2, H / 2])
    k1 = q((k0 - c) @ R.T + c + rng.normal(0, sigma, (N, 2)))
    d0 = rng.integers(0, 16, (N, D)).astype(np.float64)
    d1 = d0.copy()
    redraw = rng.random((N, D)) < 0.15
    d1[redraw] = rng.integers(0, 16, int(redraw.sum()))
    outl = rng.random(N) < p
    k1[outl] = np.stack([rng.integers(0, W, int(outl.sum())), rng.integers(0, H, int(outl.sum()))], axis=1)
    o0 = rng.integers(0, 360, N).astype(np.float64)
    o1 = o0 + 10 + rng.integers(-5, 6, N)
    s0 = 2.0 ** rng.integers(0, 4, N)
    s1 = s0.copy()
    return {"k0": k0, "k1": k1, "d0": d0, "d1": d1, "o0": o0, "o1": o1, "s0": s0, "s1": s1, "outlier": outl, "size": SIZE,
            "conf": {} if filters else dict(FILTERS_OFF)}  # fmt: skip


def run_scene(sc, dtype=np.float64, conf=None):
    return match_and_filter(sc["k0"], sc["k1"], sc["d0"], sc["d1"], sc["o0"], sc["o1"], sc["s0"], sc["s1"], sc["size"], sc["size"],
                            {**sc["conf"], **(conf or {})}, dtype)  # fmt: skip
