"""The list-building blocks of csrc/select.h, entered one by one through imcui_hip_select_probe, and the selection stages of SuperPoint
and DISK, entered through the launcher their `forward` calls (imcui_hip_superpoint_select_probe, imcui_hip_disk_select_probe), on
crafted lists and maps, against the exact integer references of tests/select_reference.py.

Every output is an integer or a float copied bit for bit: every comparison here is `np.array_equal` on integers (scores as uint32),
there is no tolerance anywhere.  Every output buffer is pre-filled with a sentinel (-1, or a NaN bit pattern for floats); `expected_*`
builds the WHOLE buffer -- sentinel included wherever the block is documented not to write (past cap, past the count, past
min(n_dev, n_cap)); DISK documents zeros past the count and SuperPoint leaves those slots alone -- so one comparison checks the written
part and the untouched part.

Each table row has an id.  A row may name `wrong` references (select_reference's deliberately wrong restatements of a tie or boundary
rule): the device's output must DIFFER from each of them on that row.  tests/test_select_probe_cpu.py checks on the CPU that the tables
are well formed, hold every coverage row and that every wrong reference is named by a row on which it differs from the right one.

The select.h probe runs the copy of the blocks compiled into csrc/select_probe.hip: it tests the source of select.h, not the copies
inside each owner.  The two stage probes and the network tests reach the owners' copies."""
from __future__ import annotations

import zlib

import numpy as np
import pytest
import torch

import select_reference as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN_F32 = 0x7FC00ABC  # float32 NaN with a payload no arithmetic produces
ERR_ARG = -1
SEL_CHUNK = 4096
DIGITS = (255, 254, 253, 252, 3, 2, 1, 0)  # the four bins of lane 0 and of lane 63 of radix_select_kth's downward walk


def _be():
    from imcui_hip import backend

    return backend


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- host <-> device, bit for bit
def _dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _dev_bits32(u):
    """uint32 bit patterns -> float32 device tensor with those bits"""
    return torch.from_numpy(np.ascontiguousarray(u, dtype=np.uint32).view(np.int32)).to(DEV).view(torch.float32)


def _dev_u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def _sent_i32(*shape):
    return torch.full(shape, -1, dtype=torch.int32, device=DEV)


def _sent_f32(*shape):
    return torch.full(shape, NAN_F32, dtype=torch.int32, device=DEV).view(torch.float32)


def _sent_i64(*shape):
    return torch.full(shape, -1, dtype=torch.int64, device=DEV)


def _host(t) -> np.ndarray:
    """device tensor -> numpy integers holding its bits (float32 -> uint32, int64 -> uint64)"""
    if t.dtype == torch.float32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    if t.dtype == torch.int64:
        return t.cpu().numpy().view(np.uint64)
    return t.cpu().numpy()


def _same(dev: dict, exp: dict) -> list:
    """names of the outputs that differ"""
    assert set(dev) == set(exp)
    return [k for k in exp if not (dev[k].shape == exp[k].shape and np.array_equal(dev[k], exp[k].astype(dev[k].dtype)))]


def _check(case, dev, expected):
    bad = _same(dev, expected(case))
    assert not bad, f"{case['id']}: outputs {bad} differ from the reference"
    for w in case.get("wrong", ()):
        assert _same(dev, expected(case, wrong=w)), f"{case['id']}: the wrong reference '{w}' is not told apart"


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


# ================================================================== COMPACT
COMPACT_CASES = [
    dict(id="partial_last_chunk", npix=2 * SEL_CHUNK + 37, kind="random", wrong=("pred_ge",)),
    dict(id="npix_15", npix=15, kind="random"),
    dict(id="npix_4096", npix=SEL_CHUNK, kind="random"),
    dict(id="no_candidate", npix=SEL_CHUNK + 100, kind="none"),
    dict(id="every_pixel", npix=SEL_CHUNK + 100, kind="all"),
    dict(id="last_chunk_only", npix=2 * SEL_CHUNK + 37, kind="tail"),
    dict(id="cap_mid_thread", npix=2 * SEL_CHUNK + 37, kind="all", cap=SEL_CHUNK + 16 * 5 + 7, wrong=("cap_first",)),
    dict(id="cap_0", npix=SEL_CHUNK + 100, kind="random", cap=0, wrong=("cap_first",)),
]


def compact_inputs(c):
    """-> (img f32 [2][npix], thr f32 [2]); the two images differ in contents, threshold and count"""
    rng, npix = _rng("compact" + c["id"]), c["npix"]
    img = rng.random((2, npix)).astype(np.float32)
    thr = _f32([0.3, 0.7])
    if c["kind"] == "random":
        for b in range(2):
            img[b, rng.random(npix) < 0.05] = thr[b]  # exactly at the threshold: no candidates (the rule is strict)
    elif c["kind"] == "none":
        thr = _f32([0.5, 0.5])
        img = (img * 0.5).astype(np.float32)
        img[0, ::9] = 0.5
        img[1, [3, npix // 2, npix - 1]] = 0.75
    elif c["kind"] == "all":
        thr = _f32([-1.0, 0.25])
        img[1] = 0.3 + 0.5 * img[1]
        img[1, ::7] = 0.25
    elif c["kind"] == "tail":
        img = (img * 0.25).astype(np.float32)
        img[0, 2 * SEL_CHUNK :] = 0.9
        img[1, 2 * SEL_CHUNK + 20 :: 2] = 0.8
    return img, thr


def expected_compact(c, wrong=None):
    img, thr = compact_inputs(c)
    npix = c["npix"]
    cap, nchunk = c.get("cap", npix), -(-npix // SEL_CHUNK)
    out = dict(cscore=np.full((2, npix), NAN_F32, np.uint32), cidx=np.full((2, npix), -1, np.int32), ncand=np.zeros(2, np.int32),
               blkcnt=np.zeros((2, nchunk), np.int32), blkoff=np.zeros((2, nchunk), np.int32))  # fmt: skip
    for b in range(2):
        pred = img[b] >= thr[b] if wrong == "pred_ge" else img[b] > thr[b]
        idx, count = R.compact(pred, cap, wrong)
        out["cidx"][b, : len(idx)] = idx
        out["cscore"][b, : len(idx)] = R.bits(img[b][idx])
        out["ncand"][b] = count
        out["blkcnt"][b], out["blkoff"][b] = R.chunk_counts(pred)
    return out


@pytest.mark.parametrize("c", COMPACT_CASES, ids=[c["id"] for c in COMPACT_CASES])
def test_compact(c):
    img, thr = compact_inputs(c)
    npix = c["npix"]
    nchunk = -(-npix // SEL_CHUNK)
    cscore, cidx, ncand = _sent_f32(2, npix), _sent_i32(2, npix), _sent_i32(2)
    blkcnt, blkoff = _sent_i32(2, nchunk), _sent_i32(2, nchunk)
    _be().select_probe(DEV, op="compact", B=2, n=npix, capacity=npix, cap=c.get("cap", npix), score=torch.from_numpy(img).to(DEV),
                       thr=torch.from_numpy(thr).to(DEV), out_score=cscore, out_idx=cidx, out_count=ncand, out_aux=blkcnt, out_i32=blkoff)  # fmt: skip
    torch.cuda.synchronize()
    _check(c, dict(cscore=_host(cscore), cidx=_host(cidx), ncand=_host(ncand), blkcnt=_host(blkcnt), blkoff=_host(blkoff)), expected_compact)


# ================================================================== SCAN
SCAN_CASES = [dict(id=f"n{n}_{'in_place' if ip else 'out_of_place'}", n=n, inplace=ip, wrong=("inclusive",) if n > 1 else ())
              for n in (1, 1023, 1024, 1025, 2500) for ip in (False, True)]  # fmt: skip
SCAN_CASES += [
    dict(id="n_dev_zero_and_above_cap", n=2500, n_dev=[0, 3000], inplace=False),
    dict(id="n_dev_partial_in_place", n=2500, n_dev=[1025, 2499], inplace=True, wrong=("inclusive",)),
    dict(id="n_cap_0", n=0, inplace=False),
]


def scan_inputs(c):
    """int32 [2][capacity], capacity = n + 13: many zeros and one large entry in every batch of 1024, so that the carry matters"""
    rng, cap = _rng("scan" + c["id"]), c["n"] + 13
    v = rng.integers(0, 4, (2, cap)) * (rng.random((2, cap)) < 0.5)
    for b in range(2):
        for base in range(0, cap, 1024):
            v[b, base + int(rng.integers(0, min(1024, cap - base)))] = 100000 + 1000 * b + base
    return v.astype(np.int32)


def expected_scan(c, wrong=None):
    v = scan_inputs(c)
    out = v.copy() if c["inplace"] else np.full(v.shape, -1, np.int32)
    total = np.zeros(2, np.int32)
    for b in range(2):
        o, t = R.exclusive_scan(v[b], c["n"], c["n_dev"][b] if "n_dev" in c else None, wrong)
        out[b, : len(o)] = o
        total[b] = t
    return dict(out=out, total=total)


@pytest.mark.parametrize("c", SCAN_CASES, ids=[c["id"] for c in SCAN_CASES])
def test_scan(c):
    v = _dev_i32(scan_inputs(c))
    out = v if c["inplace"] else _sent_i32(*v.shape)
    total = _sent_i32(2)
    _be().select_probe(DEV, op="scan", B=2, n=c["n"], capacity=v.shape[1], in_i32=v, out_i32=out, out_count=total,
                       n_dev=_dev_i32(c["n_dev"]) if "n_dev" in c else None)  # fmt: skip
    torch.cuda.synchronize()
    _check(c, dict(out=_host(out), total=_host(total)), expected_scan)


# ================================================================== ORDER_KEY
# a sorted ladder: -inf, negative normals, negative denormals, -0.0, +0.0, positive denormals, positive normals, +inf
LADDER_BITS = np.array([0xFF800000, 0xFF7FFFFF, 0xC0490FDB, 0xBF800000, 0x80800001, 0x80800000, 0x807FFFFF, 0x80000002, 0x80000001, 0x80000000,
                        0x00000000, 0x00000001, 0x00000002, 0x007FFFFF, 0x00800000, 0x00800001, 0x3F800000, 0x40490FDB, 0x7F7FFFFF, 0x7F800000],
                       dtype=np.uint32)  # fmt: skip
ORDER_KEY_CASES = [dict(id="ladder", wrong=("signed_zero",))]


def expected_order_key(c, wrong=None):
    return dict(key=np.concatenate([R.order_key(R.unbits(LADDER_BITS), wrong), np.full(5, 0xFFFFFFFF, np.uint32)]))


def test_order_key_ladder():
    c = ORDER_KEY_CASES[0]
    n = len(LADDER_BITS)
    out = _sent_i32(n + 5)
    _be().select_probe(DEV, op="order_key", B=1, n=n, capacity=n + 5, score=_dev_bits32(LADDER_BITS), out_key32=out)
    torch.cuda.synchronize()
    key = _host(out).view(np.uint32)
    _check(c, dict(key=key), expected_order_key)
    zero = int(np.flatnonzero(LADDER_BITS == 0x80000000)[0])
    d = np.diff(key[:n].astype(np.int64))
    assert d[zero] == 0 and (np.delete(d, zero) > 0).all(), "strictly increasing except the one zero pair"


# ================================================================== KTH32 / KTH64
KTH_NS = (1, 2, 1024, 1025, 3000)
KTH_FAMILIES = {32: ("all_equal", "two_plateaus", "byte0_only", "negatives", "mixed_zero", "bins"),
                64: ("all_equal", "two_plateaus", "low_word_only", "high_word_only", "bins")}  # fmt: skip


def _inverse_order_key(key):
    """float32 bit patterns whose order_key is `key` (uint32; 0x7FFFFFFF has none)"""
    key = np.asarray(key, dtype=np.uint32)
    return np.where((key & np.uint32(0x80000000)) != 0, key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32)


def kth_raw(width: int, family: str, n: int) -> np.ndarray:
    """32: float32 bit patterns (the kernel applies order_key); 64: the raw keys"""
    rng = _rng(f"kth{width}{family}{n}")
    nbytes = width // 8
    if family == "all_equal":
        return R.bits(np.full(n, 0.5)) if width == 32 else np.full(n, 0x0123456789ABCDEF, np.uint64)
    if family == "two_plateaus":  # a third high, the rest low
        hi = np.arange(n) % 3 == 1
        return R.bits(np.where(hi, 2.0, 1.0)) if width == 32 else np.where(hi, np.uint64(7 << 40), np.uint64(5 << 40))
    if family == "byte0_only":
        return (np.uint32(0x3F800000) | rng.integers(0, 256, n).astype(np.uint32)).astype(np.uint32)
    if family == "negatives":
        return R.bits(-rng.integers(1, 40, n) * 0.125)
    if family == "mixed_zero":
        return R.bits(rng.choice(_f32([-1.5, -1e-40, -0.0, 0.0, 1e-40, 2.5]), n))
    if family == "low_word_only":
        return (np.uint64(0xDEADBEEF << 32) | rng.integers(0, 1 << 32, n, dtype=np.uint64)).astype(np.uint64)
    if family == "high_word_only":
        return ((rng.integers(0, 1 << 32, n, dtype=np.uint64) << np.uint64(32)) | np.uint64(0x00C0FFEE)).astype(np.uint64)
    assert family == "bins"  # every byte of every key is one of DIGITS
    key = np.zeros(n, np.uint64)
    for byte in range(nbytes):
        key |= rng.choice(np.array(DIGITS, np.uint64), n) << np.uint64(8 * byte)
    return _inverse_order_key(key.astype(np.uint32)) if width == 32 else key


def kth_keys(width: int, family: str, n: int, wrong=None) -> np.ndarray:
    """the keys the radix select sees"""
    raw = kth_raw(width, family, n)
    return R.order_key(R.unbits(raw), wrong) if width == 32 else raw


def _kth_rows(width: int, family: str):
    rows = []
    if family == "bins":
        n = 3000
        s = np.sort(kth_keys(width, family, n))[::-1]
        for byte in range(width // 8):
            digit = (s >> s.dtype.type(8 * byte)) & s.dtype.type(0xFF)
            for d in DIGITS:
                p = np.flatnonzero(digit == d)
                rows.append(dict(id=f"kth{width}_bins_byte{byte}_digit{d}", width=width, family=family, n=n, k=int(p[len(p) // 2]) + 1, byte=byte, digit=d))
        return rows
    for n in KTH_NS:
        for k in sorted({1, 2, n // 2, n - 1, n} & set(range(1, n + 1))):
            rows.append(dict(id=f"kth{width}_{family}_n{n}_k{k}", width=width, family=family, n=n, k=k, wrong=("off_by_one",) if n > 1 else ()))
    if family == "mixed_zero":  # k = the last of the zeros: a key that put -0.0 below +0.0 would answer with -0.0's
        keys = kth_keys(width, family, 3000)
        rows.append(dict(id=f"kth{width}_mixed_zero_last_zero", width=width, family=family, n=3000, k=int((keys >= R.order_key(_f32([0.0]))[0]).sum()),
                         wrong=("off_by_one", "signed_zero")))  # fmt: skip
    return rows


KTH_ROWS = [r for w in (32, 64) for f in KTH_FAMILIES[w] for r in _kth_rows(w, f)]


def expected_kth(r, wrong=None):
    if wrong == "signed_zero":
        kth, ne = R.kth_largest(kth_keys(r["width"], r["family"], r["n"], wrong), r["k"])
    else:
        kth, ne = R.kth_largest(kth_keys(r["width"], r["family"], r["n"]), r["k"], wrong)
    return dict(key=np.array([kth], np.uint64), n_equal=np.array([ne], np.int32))


@pytest.mark.parametrize("width,family", [(w, f) for w in (32, 64) for f in KTH_FAMILIES[w]])
def test_kth(width, family):
    rows = [r for r in KTH_ROWS if r["width"] == width and r["family"] == family]
    be = _be()
    for g in range(0, len(rows), be.SELECT_MAXB):
        grp = rows[g : g + be.SELECT_MAXB]
        cap = max(r["n"] for r in grp) + 9
        # past a row's n the buffer holds the largest key: a read past n would change the answer
        buf = np.full((len(grp), cap), 0x7F800000 if width == 32 else 0xFFFFFFFFFFFFFFFF, np.uint32 if width == 32 else np.uint64)
        for i, r in enumerate(grp):
            buf[i, : r["n"]] = kth_raw(width, family, r["n"])
        ne = _sent_i32(len(grp))
        f = dict(B=len(grp), capacity=cap, n_row=[r["n"] for r in grp], k_row=[r["k"] for r in grp], out_count=ne)
        if width == 32:
            key = _sent_i32(len(grp))
            be.select_probe(DEV, op="kth32", score=_dev_bits32(buf), out_key32=key, **f)
        else:
            key = _sent_i64(len(grp))
            be.select_probe(DEV, op="kth64", key64=_dev_u64(buf), out_key64=key, **f)
        torch.cuda.synchronize()
        hk = _host(key).view(np.uint32).astype(np.uint64) if width == 32 else _host(key)
        hn = _host(ne)
        for i, r in enumerate(grp):
            _check(r, dict(key=hk[i : i + 1], n_equal=hn[i : i + 1]), expected_kth)


# ================================================================== RANK4 / RANK16
RANK_CASES = [dict(id=f"rank{nw}_{kind}", nw=nw, kind=kind) for nw in (4, 16) for kind in ("none", "all", "last_lane_of_last_wave", "partial_second_batch")]


def rank_inputs(c):
    """-> (flags int32 [2][capacity], n per row)"""
    wg, rng = 64 * c["nw"], _rng("rank" + c["id"])
    n = {"none": (wg + 17, 5), "all": (2 * wg + 3, wg), "last_lane_of_last_wave": (wg, 2 * wg), "partial_second_batch": (wg + 100, 2500)}[c["kind"]]
    cap = max(n) + 7
    f = np.zeros((2, cap), np.int32)
    if c["kind"] == "all":
        f[:] = 1
    elif c["kind"] == "last_lane_of_last_wave":
        f[0, wg - 1] = 1
        f[1, 2 * wg - 1] = 7
    elif c["kind"] == "partial_second_batch":
        f[:] = rng.integers(0, 3, (2, cap))
    for b in range(2):
        f[b, n[b] :] = 1  # past n: flags that must not be read
    return f, n


def expected_rank(c, wrong=None):
    f, n = rank_inputs(c)
    pos, total = np.full(f.shape, -1, np.int32), np.zeros(2, np.int32)
    for b in range(2):
        pos[b, : n[b]], total[b] = R.ordered_rank(f[b, : n[b]])
    return dict(pos=pos, total=total)


@pytest.mark.parametrize("c", RANK_CASES, ids=[c["id"] for c in RANK_CASES])
def test_block_ordered_rank(c):
    f, n = rank_inputs(c)
    pos, total = _sent_i32(*f.shape), _sent_i32(2)
    _be().select_probe(DEV, op=f"rank{c['nw']}", B=2, capacity=f.shape[1], n_row=n, in_i32=_dev_i32(f), out_idx=pos, out_count=total)
    torch.cuda.synchronize()
    _check(c, dict(pos=_host(pos), total=_host(total)), expected_rank)


# ================================================================== KEEP
KEEP_N = (2500, 1500)
KEEP_CASES = [dict(id=f"filter_on_limit_{lim}", filter=1, limit=lim, wrong=("strict",)) for lim in ("below", "equal_row0", "equal_row1", "above")]
KEEP_CASES += [dict(id=f"filter_off_limit_{lim}", filter=0, limit=lim) for lim in (100, 2500, 4000)]


def keep_inputs(c):
    """-> (keys u64 [2][capacity], kth, limit): few distinct keys, kth one of them, so that many keys EQUAL it"""
    rng = _rng("keep")
    keys = (rng.integers(0, 40, (2, KEEP_N[0] + 11)).astype(np.uint64) << np.uint64(32)) | rng.integers(0, 3, (2, KEEP_N[0] + 11)).astype(np.uint64)
    kth = int((np.uint64(25) << np.uint64(32)) | np.uint64(1))
    q = [int((keys[b, : KEEP_N[b]] >= np.uint64(kth)).sum()) for b in range(2)]
    lim = c["limit"]
    limit = {"below": min(q) - 7, "equal_row0": q[0], "equal_row1": q[1], "above": max(q) + 9}[lim] if isinstance(lim, str) else lim
    return keys, kth, limit


def expected_keep(c, wrong=None):
    keys, kth, limit = keep_inputs(c)
    out, count = np.full(keys.shape, -1, np.int32), np.zeros(2, np.int32)
    for b in range(2):
        q, count[b] = R.keep_in_order(keys[b, : KEEP_N[b]], kth, bool(c["filter"]), limit, wrong)
        out[b, : len(q)] = q
    return dict(out=out, count=count)


@pytest.mark.parametrize("c", KEEP_CASES, ids=[c["id"] for c in KEEP_CASES])
def test_keep_kth_in_order(c):
    keys, kth, limit = keep_inputs(c)
    out, count = _sent_i32(*keys.shape), _sent_i32(2)
    _be().select_probe(DEV, op="keep", B=2, capacity=keys.shape[1], n_row=KEEP_N, filter=c["filter"], kth=kth, limit=limit, key64=_dev_u64(keys),
                       out_idx=out, out_count=count)  # fmt: skip
    torch.cuda.synchronize()
    _check(c, dict(out=_host(out), count=_host(count)), expected_keep)


# ================================================================== CUT (zero, advance, cut, rank)
CUT_CASES = [
    dict(id="fewer_than_limit", kcap=800, levels=[[100, 20], [150, 60], [50, 40]], limit=500),
    dict(id="plateau_across_the_cut", kcap=800, levels=[[300, 150], [250, 200], [150, 100]], limit=200, wrong=("ties_low", "ties_reversed")),
    dict(id="limit_0_three_tiles", kcap=800, levels=[[400, 100], [300, 200]], limit=0, wrong=("ties_reversed",)),
    dict(id="more_than_kcap", kcap=800, levels=[[500, 200], [400, 300]], limit=300, wrong=("ties_low",)),
    dict(id="more_than_kcap_no_limit", kcap=300, levels=[[200, 100], [101, 50]], limit=0),
    dict(id="zero_total", kcap=64, levels=[[0, 2], [0, 3]], limit=10),
    # the ranked rows (ranked_rows_kernel, workgroups of 256 kept candidates)
    dict(id="kept_256", kcap=1024, levels=[[200, 100], [56, 50]], limit=0, wrong=("ties_reversed",)),
    dict(id="kept_257_one_row_in_the_second_workgroup", kcap=1024, levels=[[200, 100], [57, 50]], limit=0, wrong=("ties_reversed",)),
    dict(id="one_image_keeps_nothing", kcap=1024, levels=[[300, 0], [100, 0]], limit=0, wrong=("ties_reversed",)),
    dict(id="all_equal_across_256", kcap=1024, levels=[[400, 300], [200, 250]], limit=300, equal=True, wrong=("ties_low", "ties_reversed")),
]


def cut_inputs(c):
    """-> (scores f32 [2][kcap] from a few values (negative, -0.0, +0.0, positive; `equal`: image 0 holds one value), level counts int32 [nlev][2])"""
    rng = _rng("cut" + c["id"])
    s = rng.choice(_f32([-1.0, -0.0, 0.0, 0.25, 0.5, 1.0]), (2, c["kcap"])).astype(np.float32)
    if c.get("equal"):
        s[0] = 0.5
    return s, np.array(c["levels"], np.int32)


def expected_cut(c, wrong=None):
    s, lev = cut_inputs(c)
    kcap = c["kcap"]
    out = dict(kslot=np.full((2, kcap), -1, np.int32), nkept=np.zeros(2, np.int32), base=lev.sum(0).astype(np.int32), status=np.zeros(1, np.int32),
               rank=np.full((2, kcap), -1, np.int32))  # fmt: skip
    for b in range(2):
        kept, st = R.cut(s[b], int(lev[:, b].sum()), kcap, c["limit"], wrong)
        out["kslot"][b, : len(kept)] = kept
        out["nkept"][b] = len(kept)
        out["status"][0] |= st
        out["rank"][b, : len(kept)] = R.kept_rank(s[b], kept, wrong)
    return out


@pytest.mark.parametrize("c", CUT_CASES, ids=[c["id"] for c in CUT_CASES])
def test_cut_and_rank(c):
    s, lev = cut_inputs(c)
    kcap = c["kcap"]
    kslot, nkept, base, status, rank = _sent_i32(2, kcap), _sent_i32(2), _sent_i32(2), _sent_i32(1), _sent_i32(2, kcap)
    _be().select_probe(DEV, op="cut", B=2, capacity=kcap, limit=c["limit"], nlev=len(lev), score=torch.from_numpy(s).to(DEV), in_i32=_dev_i32(lev),
                       out_idx=kslot, out_count=nkept, out_aux=base, out_i32=rank, status=status)  # fmt: skip
    torch.cuda.synchronize()
    _check(c, dict(kslot=_host(kslot), nkept=_host(nkept), base=_host(base), status=_host(status), rank=_host(rank)), expected_cut)


# ================================================================== refusals of the select.h probe
def select_refusals():
    """(rule of imcui_hip_select_desc_check, fields with host stand-ins for the pointers: any non-zero integer)"""
    P = 4096
    base = {
        "compact": dict(op="compact", B=2, n=100, capacity=100, cap=100, score=P, thr=P, out_score=P, out_idx=P, out_count=P, out_i32=P, out_aux=P),
        "scan": dict(op="scan", B=2, n=100, capacity=100, in_i32=P, out_i32=P, out_count=P),
        "order_key": dict(op="order_key", B=1, n=100, capacity=100, score=P, out_key32=P),
        "kth32": dict(op="kth32", B=2, capacity=100, n_row=[100, 50], k_row=[1, 50], score=P, out_key32=P, out_count=P),
        "kth64": dict(op="kth64", B=2, capacity=100, n_row=[100, 50], k_row=[1, 50], key64=P, out_key64=P, out_count=P),
        "rank4": dict(op="rank4", B=2, capacity=100, n_row=[100, 0], in_i32=P, out_idx=P, out_count=P),
        "rank16": dict(op="rank16", B=2, capacity=100, n_row=[100, 0], in_i32=P, out_idx=P, out_count=P),
        "keep": dict(op="keep", B=2, capacity=100, n_row=[100, 0], limit=5, key64=P, out_idx=P, out_count=P),
        "cut": dict(op="cut", B=2, capacity=100, limit=5, nlev=2, score=P, in_i32=P, out_idx=P, out_count=P, out_i32=P, out_aux=P, status=P),
    }
    bad = [(0, f) for f in base.values()]
    bad += [(1, {**base["scan"], "op": 9}), (1, {**base["scan"], "op": -1})]
    for f in base.values():
        bad += [(2, {**f, "B": 0}), (2, {**f, "B": 9}), (3, {**f, "capacity": 0})]
        bad += [(6, {**f, k: 0}) for k, v in f.items() if v == P]
    bad += [(3, {**base[o], "n": -1}) for o in ("compact", "scan", "order_key")] + [(3, {**base[o], "n": 101}) for o in ("scan", "order_key")]
    bad += [(3, {**base["compact"], "n": 0})]
    for o in ("kth32", "kth64", "rank4", "rank16", "keep"):
        bad += [(3, {**base[o], "n_row": [100, 101]}), (3, {**base[o], "n_row": [-1, 0]})]
    for o in ("kth32", "kth64"):
        bad += [(4, {**base[o], "k_row": [0, 50]}), (4, {**base[o], "k_row": [1, 51]}), (4, {**base[o], "n_row": [100, 0], "k_row": [1, 0]})]
    bad += [(5, {**base["compact"], "cap": -1}), (5, {**base["compact"], "cap": 101}), (5, {**base["keep"], "limit": -1}), (5, {**base["cut"], "limit": -1})]
    bad += [(7, {**base["cut"], "nlev": 1}), (7, {**base["cut"], "nlev": 17})]
    return bad


def test_select_probe_refuses_a_bad_descriptor_and_launches_nothing():
    be = _be()
    out = _sent_i32(4096)
    for rule, f in select_refusals():
        if rule == 0:
            continue
        f = {k: (out if v == 4096 and k not in ("op", "B", "n", "capacity", "cap", "limit", "nlev") else v) for k, v in f.items()}
        assert be.select_probe(DEV, check=False, **f) == ERR_ARG, (rule, f["op"])
    torch.cuda.synchronize()
    assert (out == -1).all(), "a refused call wrote to its buffers"


# ================================================================== SuperPoint's selection stage
SP_H, SP_W, SP_THR, SP_BORDER = 96, 128, 0.05, 4
SP_KS = (-1, 0, 1, 2, 3, 64, 65, 128, 129, 1024, 1025, 2049)
SP_CASES = [dict(id=f"k{k}", maxk=k, wrong=("ties_high",) if 0 < k < 2049 else (("thr_ge",) if k == -1 else ())) for k in SP_KS]
SP_CASES += [
    dict(id="all_candidates_equal", maxk=129, kind="equal", wrong=("ties_high",)),
    dict(id="n_below_k", maxk=4000),
    dict(id="kcap_below_k_topk", maxk=500, kcap=300, wrong=("ties_high",)),
    dict(id="kcap_below_n_all", maxk=-1, kcap=1000),
    dict(id="cand_cap_below_n", maxk=700, cand_cap=1000, wrong=("ties_high",)),
    dict(id="border_band_only", maxk=100, kind="border"),
    dict(id="k_above_topk_max", maxk=R.SP_TOPK_MAX + 1, kind="dense", H=160, W=160),
]


def sp_inputs(c):
    """post-NMS maps f32 [2][H][W]: about 3000 / 1800 candidates with scores from 8 distinct values (equal score bits straddle every
    cut), pixels exactly at the threshold, and candidates inside the border band that the rule must drop"""
    H, W = c.get("H", SP_H), c.get("W", SP_W)
    rng, kind = _rng("sp" + c.get("kind", "plain") + str(H)), c.get("kind", "plain")
    m = np.zeros((2, H, W), np.float32)
    vals = _f32([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8])
    for b, frac in enumerate((0.29, 0.17)):
        on = rng.random((H, W)) < frac
        m[b][on] = _f32(0.5) if kind == "equal" else rng.choice(vals, int(on.sum()))
        m[b][(rng.random((H, W)) < 0.02) & ~on] = _f32(SP_THR)
    if kind == "border":
        inner = np.zeros((H, W), bool)
        inner[SP_BORDER : H - SP_BORDER, SP_BORDER : W - SP_BORDER] = True
        m[:, inner] = 0.0
    if kind == "dense":  # image 0: more than TOPK_MAX + 1 candidates; image 1: a hundred, which take the row-major path
        m[0] = rng.choice(vals, (H, W))
        m[1] = 0.0
        m[1].reshape(-1)[rng.choice(np.arange(H * W), 400, replace=False)] = 0.3
    return m


def sp_params(c):
    H, W = c.get("H", SP_H), c.get("W", SP_W)
    k = c["maxk"]
    return dict(thr=SP_THR, border=SP_BORDER, maxk=k, kcap=c.get("kcap", H * W if k < 0 else max(1, k)), cand_cap=c.get("cand_cap", H * W))


def expected_sp(c, wrong=None):
    m, p = sp_inputs(c), sp_params(c)
    W, kcap = m.shape[2], p["kcap"]
    out = dict(keypoints=np.full((2, kcap, 2), NAN_F32, np.uint32), scores=np.full((2, kcap), NAN_F32, np.uint32), nk=np.zeros(2, np.int32),
               status=np.zeros(1, np.int32))  # fmt: skip
    for b in range(2):
        idx, sb, k, st = R.superpoint_select(m[b], p["thr"], p["border"], p["maxk"], kcap, p["cand_cap"], wrong)
        out["keypoints"][b, : len(idx), 0] = R.bits(_f32(idx % W))
        out["keypoints"][b, : len(idx), 1] = R.bits(_f32(idx // W))
        out["scores"][b, : len(idx)] = sb
        out["nk"][b] = k
        out["status"][0] |= st
    return out


def _stage_outputs(kcap):
    return dict(keypoints=_sent_f32(2, kcap, 2), scores=_sent_f32(2, kcap), num_keypoints=_sent_i32(2), status=_sent_i32(1))


def _stage_host(o):
    return dict(keypoints=_host(o["keypoints"]), scores=_host(o["scores"]), nk=_host(o["num_keypoints"]), status=_host(o["status"]))


@pytest.mark.parametrize("c", SP_CASES, ids=[c["id"] for c in SP_CASES])
def test_superpoint_select_stage(c):
    m, p = sp_inputs(c), sp_params(c)
    o = _stage_outputs(p["kcap"])
    _be().SuperPointHIP().select_probe(torch.from_numpy(m).to(DEV), p["thr"], p["border"], p["maxk"], p["kcap"], cand_cap=p["cand_cap"], out=o)
    torch.cuda.synchronize()
    _check(c, _stage_host(o), expected_sp)


# ================================================================== DISK's detection stage
DK_H, DK_W = 96, 128
DK_CASES = [dict(id=f"maxk_{name}", maxk=name, window=5, wrong=w) for name, w in
            (("all", ()), ("0", ()), ("1", ("ge",)), ("n-1", ("ge",)), ("n", ()), ("n+5", ()))]  # fmt: skip
DK_CASES += [
    dict(id="plateau_at_the_cut", maxk=600, window=5, wrong=("ge",)),
    dict(id="distinct_scores", maxk=600, window=5, kind="distinct", wrong=("ge", "kth_off_by_one")),
    dict(id="window_1", maxk=2000, window=1, wrong=("ge",)),
    dict(id="window_1_all", maxk="all", window=1),
    dict(id="kcap_below_the_limit", maxk=300, window=5, kcap=100),
    dict(id="ccap_below_n", maxk=500, window=5, ccap=700),
    dict(id="zero_candidates", maxk=50, window=5, kind="empty"),
]


def dk_inputs(c):
    """heat maps f32 [2][H][W]: peaks 3 apart (more than 1024 survive a window of 5 in image 0, fewer in image 1) with scores from a few
    distinct values, pairs of equal neighbours (the first of a window's maxima wins), a background below the threshold"""
    rng = _rng("disk" + c.get("kind", "plain"))
    m = np.full((2, DK_H, DK_W), -1.0, np.float32)
    vals = _f32([0.5, 1.0, 1.5, 2.0, 2.5, 3.0])
    for b, frac in enumerate((0.95, 0.6)):
        on = np.zeros((DK_H, DK_W), bool)
        on[1::3, 1::3] = rng.random(on[1::3, 1::3].shape) < frac
        m[b][on] = rng.choice(vals, int(on.sum())) if c.get("kind") != "distinct" else _f32(0.5 + 1e-3 * rng.permutation(int(on.sum())))
        twin = on & (rng.random(on.shape) < 0.1)
        m[b][:, 1:][twin[:, :-1]] = m[b][:, :-1][twin[:, :-1]]  # the right neighbour ties its peak
    if c.get("kind") == "empty":
        m[0] = -1.0
        m[1, :, 20:] = -1.0
    return m


def dk_params(c):
    m = dk_inputs(c)
    n0 = int(R.disk_nms(m[0], c["window"], 0.0).sum())
    maxk = {"all": -1, "0": 0, "1": 1, "n-1": n0 - 1, "n": n0, "n+5": n0 + 5}[c["maxk"]] if isinstance(c["maxk"], str) else c["maxk"]
    bound = (-(-DK_H // (c["window"] // 2 + 1))) * (-(-DK_W // (c["window"] // 2 + 1)))
    return dict(window=c["window"], thr=0.0, maxk=maxk, kcap=c.get("kcap", bound if maxk < 0 else max(1, min(maxk, bound))), ccap=c.get("ccap", DK_H * DK_W))


def expected_dk(c, wrong=None):
    m, p = dk_inputs(c), dk_params(c)
    W, kcap = m.shape[2], p["kcap"]
    out = dict(keypoints=np.zeros((2, kcap, 2), np.uint32), scores=np.zeros((2, kcap), np.uint32), nk=np.zeros(2, np.int32), status=np.zeros(1, np.int32))
    for b in range(2):
        idx, sb, k, st = R.disk_select(m[b], p["window"], p["thr"], p["maxk"], kcap, p["ccap"], wrong)
        out["keypoints"][b, :k, 0] = R.bits(_f32(idx % W))
        out["keypoints"][b, :k, 1] = R.bits(_f32(idx // W))
        out["scores"][b, :k] = sb
        out["nk"][b] = k
        out["status"][0] |= st
    return out


@pytest.mark.parametrize("c", DK_CASES, ids=[c["id"] for c in DK_CASES])
def test_disk_select_stage(c):
    m, p = dk_inputs(c), dk_params(c)
    o = _stage_outputs(p["kcap"])
    _be().DiskHIP().select_probe(torch.from_numpy(m).to(DEV), p["window"], p["thr"], p["maxk"], p["kcap"], ccap=p["ccap"], out=o)
    torch.cuda.synchronize()
    _check(c, _stage_host(o), expected_dk)


# ================================================================== refusals of the two stage probes
def test_stage_probes_refuse_bad_arguments_and_launch_nothing():
    be = _be()
    m = torch.zeros(2, 16, 24, device=DEV)
    sp, dk = be.SuperPointHIP(), be.DiskHIP()
    o = _stage_outputs(8)
    assert sp.select_probe(m, 0.1, 0, 4, 0, out=o, check=False) == ERR_ARG  # kcap
    assert sp.select_probe(m, 0.1, 0, 4, 8, cand_cap=0, out=o, check=False) == ERR_ARG
    assert dk.select_probe(m, 5, 0.0, 4, 0, out=o, check=False) == ERR_ARG
    assert dk.select_probe(m, 5, 0.0, 4, 8, ccap=0, out=o, check=False) == ERR_ARG
    assert dk.select_probe(m, 4, 0.0, 4, 8, out=o, check=False) == ERR_ARG  # even window
    assert dk.select_probe(m, 0, 0.0, 4, 8, out=o, check=False) == ERR_ARG
    for k in ("keypoints", "scores", "num_keypoints", "status"):
        assert sp.select_probe(m, 0.1, 0, 4, 8, out={**o, k: None}, check=False) == ERR_ARG, k
        assert dk.select_probe(m, 5, 0.0, 4, 8, out={**o, k: None}, check=False) == ERR_ARG, k
    torch.cuda.synchronize()
    h = _stage_host(o)
    assert (h["keypoints"] == NAN_F32).all() and (h["scores"] == NAN_F32).all() and (h["nk"] == -1).all() and (h["status"] == -1).all()


# ================================================================== forward and probe are one path
def test_superpoint_forward_equals_the_probe_on_its_own_map():
    from imcui_hip.hloc.extractors.superpoint import SuperPoint
    from imcui_hip.synth import make_pair
    from imcui_hip.synth_weights import superpoint_state_dict

    conf = dict(nms_radius=3, max_keypoints=150, keypoint_threshold=0.005, remove_borders=4)
    model = SuperPoint({**conf, "state_dict": superpoint_state_dict(0)}).eval().to(DEV)
    img0, img1, _ = make_pair(3, 120, 160, n_blobs=150)
    out = model.forward_batched(torch.cat([img0, img1]).to(DEV), want_score_map=True)
    nms = _be().simple_nms(out["score_map"], conf["nms_radius"])
    kcap = out["scores"].shape[1]
    o = _stage_outputs(kcap)
    model._impl.select_probe(nms, conf["keypoint_threshold"], conf["remove_borders"], conf["max_keypoints"], kcap, out=o)
    torch.cuda.synchronize()
    n = out["num_keypoints"].cpu()
    assert int(n.min()) > 20 and int(out["status"][0]) == 0 == int(o["status"][0])
    assert torch.equal(n, o["num_keypoints"].cpu())
    for b in range(2):
        assert torch.equal(out["keypoints"][b, : n[b]].cpu(), o["keypoints"][b, : n[b]].cpu())
        assert np.array_equal(_host(out["scores"][b, : n[b]]), _host(o["scores"][b, : n[b]]))


def test_disk_forward_equals_the_probe_on_its_own_heatmap():
    from imcui_hip.hloc.extractors.disk import DISK
    from imcui_hip.synth_weights import disk_state_dict

    conf = dict(max_keypoints=200, nms_window_size=5, detection_threshold=-100.0)  # (every local maximum of the synthetic weights' map counts)
    model = DISK({**conf, "state_dict": disk_state_dict(0)}).eval().to(DEV)
    g = torch.Generator().manual_seed(4)
    img = torch.rand(2, 3, 96, 128, generator=g)
    out = model.forward_batched(img.to(DEV), want_heatmap=True)
    kcap = out["scores"].shape[1]
    o = _stage_outputs(kcap)
    model._impl.select_probe(out["heatmap"], 5, -100.0, 200, kcap, out=o)
    torch.cuda.synchronize()
    assert int(out["num_keypoints"].min()) > 20 and int(out["status"][0]) == int(o["status"][0])
    assert torch.equal(out["num_keypoints"].cpu(), o["num_keypoints"].cpu())
    assert np.array_equal(_host(out["keypoints"]), _host(o["keypoints"])) and np.array_equal(_host(out["scores"]), _host(o["scores"]))
