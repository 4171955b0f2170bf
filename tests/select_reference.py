"""Exact references of the list-building blocks of csrc/select.h and of the two rule stages that have probes (SuperPoint's top-k,
DISK's detection), in numpy with integers only: every output of those kernels is an integer or a float copied bit for bit, so nothing
here rounds and nothing is compared with a tolerance.  No torch.topk / argsort-with-ties anywhere: every order is spelled out.

Next to each rule stands one deliberately WRONG restatement (the `wrong_*` functions and the `wrong=` arguments): the case tables of
tests/test_gpu_select.py must tell each of them from the device's output on the case built for that rule.

Floats travel as their bit patterns (np.uint32); `bits(x)` / `unbits(u)` convert."""
from __future__ import annotations

import numpy as np

SEL_CHUNK = 4096  # csrc/select.h
SP_TOPK_MAX = 16384  # csrc/superpoint.hip


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def unbits(u) -> np.ndarray:
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


# ------------------------------------------------------------------ order_key
def order_key(x, wrong: str | None = None) -> np.ndarray:
    """u32 key with a < b <=> key(a) < key(b); -0.0 and +0.0 share a key.  wrong="signed_zero": -0.0 keeps its own key below +0.0's."""
    u = bits(x).copy()
    if wrong != "signed_zero":
        u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


# ------------------------------------------------------------------ k-th largest
def kth_largest(keys, k: int, wrong: str | None = None):
    """-> (the k-th largest key, n_equal = k - #(keys > kth)).  wrong="off_by_one": the (k+1)-th (the (k-1)-th when k = n)."""
    keys = np.asarray(keys)
    if wrong == "off_by_one":
        k = k + 1 if k < len(keys) else max(k - 1, 1)
    kth = sorted(keys.tolist(), reverse=True)[k - 1]
    return kth, k - int((keys > keys.dtype.type(kth)).sum())


# ------------------------------------------------------------------ compaction
def compact(pred, cap: int, wrong: str | None = None):
    """pred: bool [npix] of one image -> (indices written: the first `cap` in row-major order, the true count).
    wrong="cap_first": the cap is applied before counting (the count is clamped)."""
    idx = np.flatnonzero(np.asarray(pred))
    count = len(idx)
    if wrong == "cap_first":
        count = min(count, cap)
    return idx[:cap].astype(np.int64), count


def chunk_counts(pred):
    """-> (per-chunk counts, their exclusive scan) of one image."""
    pred = np.asarray(pred)
    nchunk = -(-len(pred) // SEL_CHUNK)
    cnt = np.array([int(pred[c * SEL_CHUNK : (c + 1) * SEL_CHUNK].sum()) for c in range(nchunk)], dtype=np.int64)
    return cnt, np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)


# ------------------------------------------------------------------ scan
def exclusive_scan(vals, n_cap: int, n_dev: int | None = None, wrong: str | None = None):
    """-> (out[0 .. n), total) with n = min(n_dev, n_cap) (n_cap without n_dev).  wrong="inclusive"."""
    n = n_cap if n_dev is None else max(0, min(int(n_dev), n_cap))
    v = np.asarray(vals, dtype=np.int64)[:n]
    inc = np.cumsum(v)
    out = inc if wrong == "inclusive" else inc - v
    return out.astype(np.int64), int(v.sum())


# ------------------------------------------------------------------ rank of the flagged entries
def ordered_rank(flags):
    """-> (position of every flagged entry among the flagged ones, -1 elsewhere; the total)."""
    f = np.asarray(flags) != 0
    pos = np.full(len(f), -1, dtype=np.int64)
    pos[f] = np.arange(int(f.sum()))
    return pos, int(f.sum())


# ------------------------------------------------------------------ keep the keys >= the k-th, in list order
def keep_in_order(keys, kth: int, filter_: bool, limit: int, wrong: str | None = None):
    """-> (entries written: the first `limit` that qualify, in list order; the count of all that qualify, not clamped).
    wrong="strict": key > kth."""
    keys = np.asarray(keys, dtype=np.uint64)
    if not filter_:
        q = np.arange(len(keys))
    elif wrong == "strict":
        q = np.flatnonzero(keys > np.uint64(kth))
    else:
        q = np.flatnonzero(keys >= np.uint64(kth))
    return q[:limit].astype(np.int64), len(q)


# ------------------------------------------------------------------ the cut of a multi-scale candidate list and the rank of what is left
def cut(scores, ntotal: int, kcap: int, limit_: int, wrong: str | None = None):
    """scores: f32 [kcap] of one image -> (kslot: the kept slots in slot order, status bits).  Among equal scores at the cut the LATER
    slots stay.  wrong="ties_low": the earlier slots stay."""
    n = min(int(ntotal), kcap)
    status = 2 if ntotal > kcap else 0
    s = np.asarray(scores, dtype=np.float32)[:n]
    if limit_ > 0 and n > limit_:
        ok = order_key(s).astype(np.uint64)
        slot = np.arange(n, dtype=np.uint64)
        key = (ok << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - slot if wrong == "ties_low" else slot)
        kept = np.sort(np.argsort(key, kind="stable")[n - limit_ :])  # the keys are distinct: no tie is left to the sort
    else:
        kept = np.arange(n)
    return kept.astype(np.int64), status


def kept_rank(scores, kslot, wrong: str | None = None):
    """rank of every kept candidate in ascending (score, position in the kept list) order.  wrong="ties_reversed"."""
    s = np.asarray(scores, dtype=np.float32)[np.asarray(kslot, dtype=np.int64)]
    n = len(s)
    rank = np.zeros(n, dtype=np.int64)
    for i in range(n):
        before = (np.arange(n) > i) if wrong == "ties_reversed" else (np.arange(n) < i)
        rank[i] = int(((s < s[i]) | ((s == s[i]) & before)).sum())
    return rank


# ------------------------------------------------------------------ SuperPoint's selection stage
def superpoint_select(nms, thr: float, border: int, max_keypoints: int, kcap: int, cand_cap: int | None = None, wrong: str | None = None):
    """nms: f32 [H, W] post-NMS map of one image -> (flat indices, score bits (u32), count, status).
    Candidates: nms > thr inside the border band, row-major, the first cand_cap (status 1 when there are more).  k = all of them when
    max_keypoints < 0, else min(n, max_keypoints); k > kcap: status 2, k = kcap.  n <= k or max_keypoints < 0: the first k row-major.
    Otherwise k > 16384: status 4, count 0, nothing written; else the k largest by (score bits descending, flat index ascending), in
    that order.  wrong="ties_high": equal bits -> the HIGHER index first; wrong="thr_ge": nms >= thr."""
    nms = np.asarray(nms, dtype=np.float32)
    H, W = nms.shape
    cand_cap = H * W if cand_cap is None else cand_cap
    thr32 = np.float32(thr)
    above = (nms >= thr32) if wrong == "thr_ge" else (nms > thr32)
    yy, xx = np.mgrid[0:H, 0:W]
    inside = (yy >= border) & (yy < H - border) & (xx >= border) & (xx < W - border)
    idx = np.flatnonzero((above & inside).ravel())
    status = 0
    if len(idx) > cand_cap:
        status |= 1
        idx = idx[:cand_cap]
    n = len(idx)
    k = n if max_keypoints < 0 else min(n, max_keypoints)
    if k > kcap:
        status |= 2
        k = kcap
    sb = bits(nms.ravel()[idx])
    if n <= k or max_keypoints < 0:
        return idx[:k].astype(np.int64), sb[:k], k, status
    if k > SP_TOPK_MAX:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint32), 0, status | 4
    low = idx.astype(np.uint64) if wrong == "ties_high" else np.uint64(0xFFFFFFFF) - idx.astype(np.uint64)
    key = (sb.astype(np.uint64) << np.uint64(32)) | low
    order = np.argsort(key, kind="stable")[::-1][:k]  # distinct keys
    return idx[order].astype(np.int64), sb[order], k, status


# ------------------------------------------------------------------ DISK's detection stage
def disk_nms(heat, window: int, thr: float) -> np.ndarray:
    """bool [H, W]: heat > thr, strictly above every EARLIER pixel (row-major) of its window and not below any later one -- the first
    maximum of a window wins a tie, as max_pool2d(return_indices=True) does."""
    heat = np.asarray(heat, dtype=np.float32)
    H, W = heat.shape
    r = window // 2
    pad = np.full((H + 2 * r, W + 2 * r), -np.inf, dtype=np.float32)
    pad[r : r + H, r : r + W] = heat
    keep = heat > np.float32(thr)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy == 0 and dx == 0:
                continue
            u = pad[r + dy : r + dy + H, r + dx : r + dx + W]
            keep &= (heat > u) if (dy < 0 or (dy == 0 and dx < 0)) else ~(u > heat)
    return keep


def disk_select(heat, window: int, thr: float, max_keypoints: int, kcap: int, ccap: int | None = None, wrong: str | None = None):
    """heat: f32 [H, W] -> (flat indices, score bits, count, status).  Candidates: the NMS survivors, row-major, the first ccap.
    max_keypoints < 0: all of them.  Else n_ = min(max_keypoints + 1, n), t = the n_-th largest score; the scores STRICTLY above t, then
    the first max_keypoints in row-major order.  Zero candidates: zero key-points.  More than kcap: status 2 and the first kcap.
    wrong="ge": scores >= t; wrong="kth_off_by_one": n_ = min(max_keypoints, n)."""
    heat = np.asarray(heat, dtype=np.float32)
    idx = np.flatnonzero(disk_nms(heat, window, thr).ravel())
    if ccap is not None:
        idx = idx[:ccap]
    n = len(idx)
    s = heat.ravel()[idx]
    limit, status = n, 0
    q = np.arange(n)
    if max_keypoints >= 0 and n > 0:
        limit = min(max_keypoints, n)
        n_ = min(max_keypoints, n) if wrong == "kth_off_by_one" else min(max_keypoints + 1, n)
        key = order_key(s)
        t = sorted(key.tolist(), reverse=True)[max(n_, 1) - 1]
        q = np.flatnonzero(key >= np.uint32(t)) if wrong == "ge" else np.flatnonzero(key > np.uint32(t))
    if limit > kcap:
        status |= 2
        limit = kcap
    q = q[:limit]
    return idx[q].astype(np.int64), bits(s[q]), len(q), status
