"""CPU side of the selection tests (tests/test_gpu_select.py): the descriptor mirror, the refusals the three probes make before any
launch, the exact references of tests/select_reference.py against brute force, every wrong reference against the right one on its
row, and the case tables themselves (well formed, every coverage row, every kernel and device function of csrc/select.h named)."""
import ctypes
import os
import re

import numpy as np
import torch

import select_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECT_H = os.path.join(ROOT, "image-matching-webui_amd", "csrc", "select.h")
ERR_ARG = -1

# every __global__ / __device__ name of select.h -> the ops of imcui_hip_select_probe that run it
COVERAGE = {
    "wave_ordered_rank": ("rank4", "rank16", "keep", "cut"),
    "block_ordered_rank": ("rank4", "rank16", "keep", "cut"),
    "cand_count_kernel": ("compact",),
    "operator": ("compact",),  # EmitScoreIndex::operator()
    "cand_compact_kernel": ("compact",),
    "exclusive_scan_kernel": ("scan", "compact"),
    "order_key": ("order_key", "kth32", "cut"),
    "radix_select_kth": ("kth32", "kth64", "cut"),
    "keep_kth_in_order": ("keep", "cut"),
    "zero_i32_kernel": ("cut",),
    "advance_base_kernel": ("cut",),
    "score_index_key": ("cut",),
    "cand_cut_kernel": ("cut",),
    "kept_rank_ascending": ("cut",),
    "ranked_rows_kernel": ("cut",),
}
# blocks the probe reaches through the host launchers of select.h, as the extractors do: block -> the chain of callers inside select.h,
# the last of which the probe names
VIA = {"cand_count_kernel": ("cand_count_scan", "cand_list"), "cand_compact_kernel": ("cand_compact", "cand_list"), "cand_cut_kernel": ("cand_cut",),
       "kept_rank_ascending": ("ranked_rows_kernel", "ranked_rows"), "ranked_rows_kernel": ("ranked_rows",)}  # fmt: skip
WRONG = {"pred_ge", "cap_first", "inclusive", "signed_zero", "off_by_one", "strict", "ties_low", "ties_reversed", "ties_high", "thr_ge", "ge",
         "kth_off_by_one"}  # fmt: skip


def _t():
    import test_gpu_select as t

    return t


def _tables(t):
    """op / stage -> (rows, expected)"""
    return {"compact": (t.COMPACT_CASES, t.expected_compact), "scan": (t.SCAN_CASES, t.expected_scan), "order_key": (t.ORDER_KEY_CASES, t.expected_order_key),
            "kth32": ([r for r in t.KTH_ROWS if r["width"] == 32], t.expected_kth), "kth64": ([r for r in t.KTH_ROWS if r["width"] == 64], t.expected_kth),
            "rank4": ([c for c in t.RANK_CASES if c["nw"] == 4], t.expected_rank), "rank16": ([c for c in t.RANK_CASES if c["nw"] == 16], t.expected_rank),
            "keep": (t.KEEP_CASES, t.expected_keep), "cut": (t.CUT_CASES, t.expected_cut), "superpoint": (t.SP_CASES, t.expected_sp),
            "disk": (t.DK_CASES, t.expected_dk)}  # fmt: skip


# ------------------------------------------------------------------ the ABI
def test_descriptor_mirror_matches_the_library(lib):
    from imcui_hip import backend

    assert ctypes.sizeof(backend.SelectDesc) == lib.imcui_hip_select_desc_bytes()
    hdr = open(os.path.join(ROOT, "include", "imcui_hip.h")).read()
    assert int(re.search(r"#define IMCUI_SELECT_MAXB (\d+)", hdr).group(1)) == backend.SELECT_MAXB
    assert sorted(backend.SELECT_OPS.values()) == list(range(9))


def test_probes_refuse_null_handle_and_descriptor(lib):
    from imcui_hip import backend

    d = backend.select_desc(**_t().select_refusals()[0][1])
    assert lib.imcui_hip_select_desc_check(ctypes.byref(d)) == 0
    assert lib.imcui_hip_select_probe(None, ctypes.byref(d), None) == ERR_ARG
    assert lib.imcui_hip_select_probe(None, None, None) == ERR_ARG
    assert lib.imcui_hip_select_desc_check(None) == 6
    P = ctypes.c_void_p(4096)
    assert lib.imcui_hip_superpoint_select_probe(None, P, 2, 16, 24, 0.1, 0, 4, 8, 384, P, P, P, P, P, 1 << 20, None) == ERR_ARG
    assert lib.imcui_hip_disk_select_probe(None, P, 2, 16, 24, 5, 0.0, 4, 8, 384, P, P, P, P, P, 1 << 20, None) == ERR_ARG


def test_descriptor_check_names_the_violated_rule(lib):
    """every out-of-range field is refused by the host check the probe makes before it launches anything"""
    from imcui_hip import backend

    seen = set()
    for rule, f in _t().select_refusals():
        d = backend.select_desc(**f)
        assert lib.imcui_hip_select_desc_check(ctypes.byref(d)) == rule, (rule, f)
        seen.add(rule)
    assert seen == {0, *backend.SELECT_RULES}


def test_stage_probe_workspaces_refuse_bad_shapes(lib):
    for fn in (lib.imcui_hip_superpoint_select_workspace_bytes, lib.imcui_hip_disk_select_workspace_bytes):
        assert fn(2, 96, 128, 96 * 128) > 0
        for bad in ((0, 96, 128, 100), (1025, 96, 128, 100), (2, 0, 128, 100), (2, 96, 0, 100), (2, 96, 128, 0), (2, 8192, 4096, 100), (2, 96, 128, (1 << 24) + 1)):
            assert fn(*bad) == 0, bad


# ------------------------------------------------------------------ the references against brute force
def _random_floats(rng, n):
    u = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    x = R.unbits(u)
    return x[~np.isnan(x)]


def test_order_key_orders_like_the_floats():
    t = _t()
    rng = np.random.default_rng(1)
    x = np.concatenate([_random_floats(rng, 4000), R.unbits(t.LADDER_BITS)])
    k = R.order_key(x).astype(np.int64)
    i, j = rng.integers(0, len(x), 20000), rng.integers(0, len(x), 20000)
    assert ((x[i] < x[j]) == (k[i] < k[j])).all() and ((x[i] == x[j]) == (k[i] == k[j])).all()
    lad = R.order_key(R.unbits(t.LADDER_BITS))
    assert lad[0] == 0x007FFFFF and lad[-1] == 0xFF800000 and R.order_key([-0.0])[0] == R.order_key([0.0])[0] == 0x80000000
    x = R.unbits(t.LADDER_BITS)
    classes = [np.isneginf(x), (x < 0) & (np.abs(x) >= 2.0**-126) & np.isfinite(x), (x < 0) & (np.abs(x) < 2.0**-126), t.LADDER_BITS == 0x80000000,
               t.LADDER_BITS == 0, (x > 0) & (x < 2.0**-126), (x >= 2.0**-126) & np.isfinite(x), np.isposinf(x)]  # fmt: skip
    assert all(c.any() for c in classes) and (np.diff(x.astype(np.float64)) >= 0).all(), "the ladder is sorted and has every class"


def test_kth_compact_scan_keep_rank_agree_with_brute_force():
    rng = np.random.default_rng(2)
    for n in (1, 2, 7, 300):
        keys = rng.integers(0, 20, n).astype(np.uint64)
        for k in {1, n, (n + 1) // 2}:
            kth, ne = R.kth_largest(keys, k)
            assert kth == np.sort(keys)[n - k] and ne == k - sum(1 for v in keys if v > kth) and 1 <= ne <= sum(1 for v in keys if v == kth)
        pred = rng.random(n) < 0.4
        for cap in (0, 3, n):
            loop = [i for i in range(n) if pred[i]]
            idx, cnt = R.compact(pred, cap)
            assert idx.tolist() == loop[:cap] and cnt == len(loop)
        v = rng.integers(0, 9, n)
        for n_dev in (None, 0, n // 2, n + 5):
            out, tot = R.exclusive_scan(v, n, n_dev)
            m = n if n_dev is None else min(n_dev, n)
            assert out.tolist() == [int(v[:i].sum()) for i in range(m)] and tot == int(v[:m].sum())
        kth = int(keys[rng.integers(0, n)])
        for filt in (False, True):
            for limit in (0, 2, n + 1):
                loop = [i for i in range(n) if not filt or keys[i] >= kth]
                q, cnt = R.keep_in_order(keys, kth, filt, limit)
                assert q.tolist() == loop[:limit] and cnt == len(loop)
        pos, tot = R.ordered_rank(pred)
        assert tot == int(pred.sum()) and [int(p) for p in pos if p >= 0] == list(range(tot)) and ((pos >= 0) == pred).all()


def test_cut_and_rank_agree_with_a_stable_sort():
    rng = np.random.default_rng(3)
    for n, kcap, limit in ((50, 64, 20), (64, 64, 64), (90, 64, 10), (30, 64, 0), (0, 8, 3)):
        s = rng.choice(np.array([-1.0, -0.0, 0.0, 0.5, 2.0], np.float32), kcap)
        kept, st = R.cut(s, n, kcap, limit)
        m = min(n, kcap)
        order = sorted(range(m), key=lambda i: (float(s[i]), i))  # a stable argsort of (score, index): -0.0 == 0.0 compare equal
        want = sorted(order[m - limit :]) if 0 < limit < m else list(range(m))
        assert kept.tolist() == want and st == (2 if n > kcap else 0)
        rank = R.kept_rank(s, kept)
        by = sorted(range(len(kept)), key=lambda i: (float(s[kept[i]]), i))
        assert [by.index(i) for i in range(len(kept))] == rank.tolist()


def test_superpoint_reference_agrees_with_a_python_loop():
    t = _t()
    for c in t.SP_CASES:
        if c.get("H"):
            continue
        m, p = t.sp_inputs(c), t.sp_params(c)
        H, W = m.shape[1:]
        for b in range(2):
            cand = [(y * W + x) for y in range(p["border"], H - p["border"]) for x in range(p["border"], W - p["border"]) if m[b, y, x] > np.float32(p["thr"])]
            st = 1 if len(cand) > p["cand_cap"] else 0
            cand = cand[: p["cand_cap"]]
            n = len(cand)
            k = n if p["maxk"] < 0 else min(n, p["maxk"])
            if k > p["kcap"]:
                st, k = st | 2, p["kcap"]
            if not (n <= k or p["maxk"] < 0):
                cand = sorted(cand, key=lambda i: (-int(R.bits(m[b].ravel()[i : i + 1])[0]), i))
            idx, sb, kk, status = R.superpoint_select(m[b], p["thr"], p["border"], p["maxk"], p["kcap"], p["cand_cap"])
            assert (idx.tolist(), kk, status) == (cand[:k], k, st), c["id"]
            assert np.array_equal(sb, R.bits(m[b].ravel()[idx]))


def test_disk_restatement_equals_the_rule_of_disk_reference():
    from disk_reference import heatmap_to_keypoints

    t = _t()
    for c in t.DK_CASES:
        if c.get("kcap") or c.get("ccap"):
            continue  # the reference has no capacities
        m, p = t.dk_inputs(c), t.dk_params(c)
        for b in range(2):
            if not R.disk_nms(m[b], p["window"], p["thr"]).any():
                continue  # (the reference raises on zero candidates; the kernel returns none)
            (xy, lp), = heatmap_to_keypoints(torch.from_numpy(m[b])[None, None], n=None if p["maxk"] < 0 else p["maxk"], window_size=p["window"],
                                             score_threshold=p["thr"])  # fmt: skip
            idx, sb, k, st = R.disk_select(m[b], p["window"], p["thr"], p["maxk"], 1 << 24)
            assert st == 0 and k == len(xy), c["id"]
            assert np.array_equal(idx, (xy[:, 1] * m.shape[2] + xy[:, 0]).numpy()) and np.array_equal(sb, R.bits(lp.numpy())), c["id"]


# ------------------------------------------------------------------ the case tables
def test_every_wrong_reference_differs_from_the_right_one_on_its_row():
    t = _t()
    named = set()
    for name, (rows, expected) in _tables(t).items():
        for r in rows:
            for w in r.get("wrong", ()):
                assert t._same(expected(r), expected(r, wrong=w)), f"{name} {r['id']}: '{w}' equals the right reference"
                named.add(w)
    assert named == WRONG


def test_case_tables_are_well_formed():
    t = _t()
    for name, (rows, expected) in _tables(t).items():
        assert rows, name
        ids = [r["id"] for r in rows]
        assert len(set(ids)) == len(ids), name
    # B = 2 wherever a per-image offset exists, and the two images differ in contents and counts
    for c in t.COMPACT_CASES:
        img, thr = t.compact_inputs(c)
        e = t.expected_compact(c)
        assert not np.array_equal(img[0], img[1]) and (e["ncand"][0] != e["ncand"][1] or c["id"] == "npix_15")
        assert 0 <= c.get("cap", c["npix"]) <= c["npix"]
    for c in t.SCAN_CASES:
        v = t.scan_inputs(c)
        assert v.shape[1] > c["n"] and not np.array_equal(v[0], v[1])
    for c in t.RANK_CASES:
        f, n = t.rank_inputs(c)
        assert n[0] != n[1] and max(n) < f.shape[1]
    for c in t.CUT_CASES:
        s, lev = t.cut_inputs(c)
        e = t.expected_cut(c)
        assert len(lev) >= 2 and not np.array_equal(s[0], s[1]) and e["base"][0] != e["base"][1]
    for c, inputs, expected in [(c, t.sp_inputs, t.expected_sp) for c in t.SP_CASES] + [(c, t.dk_inputs, t.expected_dk) for c in t.DK_CASES]:
        m = inputs(c)
        assert m.shape[0] == 2 and not np.array_equal(m[0], m[1]) and m.size <= 2 * 160 * 160
    for r in t.KTH_ROWS:
        assert 1 <= r["k"] <= r["n"] <= 3000
    for rule, f in t.select_refusals():
        assert 0 <= rule <= 7


def test_case_tables_have_every_coverage_row():
    t = _t()
    C = t.SEL_CHUNK
    # ---- COMPACT
    cc = {c["id"]: c for c in t.COMPACT_CASES}
    assert any(c["npix"] > C and c["npix"] % C for c in cc.values()) and any(c["npix"] < 16 for c in cc.values()) and any(c["npix"] == C for c in cc.values())
    assert t.expected_compact(cc["no_candidate"])["ncand"][0] == 0
    assert t.expected_compact(cc["every_pixel"])["ncand"][0] == cc["every_pixel"]["npix"]
    e = t.expected_compact(cc["last_chunk_only"])
    assert (e["blkcnt"][:, :-1] == 0).all() and (e["blkcnt"][:, -1] > 0).all() and cc["last_chunk_only"]["npix"] % C
    mid = cc["cap_mid_thread"]
    assert t.expected_compact(mid)["ncand"][0] == mid["npix"] and mid["cap"] % 16 and 0 < mid["cap"] < mid["npix"], "every pixel a candidate: position = pixel"
    assert cc["cap_0"]["cap"] == 0 and t.expected_compact(cc["cap_0"])["ncand"].min() > 0
    img, thr = t.compact_inputs(cc["partial_last_chunk"])
    assert thr[0] != thr[1] and (img[0] == thr[0]).any() and (img[1] == thr[1]).any(), "bind(b), and pixels exactly at the threshold"
    # ---- SCAN
    sc = t.SCAN_CASES
    assert {c["n"] for c in sc if "n_dev" not in c} >= {1, 1023, 1024, 1025, 2500}
    assert {(c["n"], c["inplace"]) for c in sc if "n_dev" not in c} >= {(n, ip) for n in (1, 1023, 1024, 1025, 2500) for ip in (False, True)}
    assert any(0 in c["n_dev"] for c in sc if "n_dev" in c) and any(max(c["n_dev"]) > c["n"] for c in sc if "n_dev" in c)
    v = t.scan_inputs(next(c for c in sc if c["n"] == 2500))
    assert all((v[b, base : base + 1024] >= 100000).any() and (v[b, base : base + 1024] == 0).any() for b in range(2) for base in (0, 1024, 2048))
    # ---- KTH32 / KTH64
    for width in (32, 64):
        rows = [r for r in t.KTH_ROWS if r["width"] == width]
        for fam in t.KTH_FAMILIES[width]:
            if fam == "bins":
                continue
            fr = [r for r in rows if r["family"] == fam]
            assert {r["n"] for r in fr} == {1, 2, 1024, 1025, 3000}, fam
            for n in (1024, 1025, 3000):
                assert {r["k"] for r in fr if r["n"] == n} >= {1, 2, n // 2, n - 1, n}, fam
        assert len(set(t.kth_keys(width, "all_equal", 1025))) == 1
        n_eq = [int(t.expected_kth(r)["n_equal"][0]) for r in rows if r["family"] == "two_plateaus" and r["n"] == 3000 and r["k"] == 1500]
        assert n_eq and 0 < n_eq[0] < 2000, "k cuts the lower plateau"
        bins = [r for r in rows if r["family"] == "bins"]
        assert {(r["byte"], r["digit"]) for r in bins} == {(b, d) for b in range(width // 8) for d in t.DIGITS}
        for r in bins:
            kth = int(t.expected_kth(r)["key"][0])
            assert (kth >> (8 * r["byte"])) & 0xFF == r["digit"], r["id"]
    k = t.kth_keys(32, "byte0_only", 3000)
    assert len(set(k >> 8)) == 1 and len(set(k & 0xFF)) > 100
    assert (R.unbits(t.kth_raw(32, "negatives", 3000)) < 0).all()
    z = t.kth_raw(32, "mixed_zero", 3000)
    assert (z == 0x80000000).any() and (z == 0).any() and (R.unbits(z) < 0).any() and (R.unbits(z) > 0).any()
    lo, hi = t.kth_keys(64, "low_word_only", 3000), t.kth_keys(64, "high_word_only", 3000)
    assert len(set(lo >> np.uint64(32))) == 1 and len(set(lo)) > 2900 and len(set(hi & np.uint64(0xFFFFFFFF))) == 1 and len(set(hi)) > 2900
    # ---- RANK4 / RANK16
    for nw in (4, 16):
        rc = {c["kind"]: c for c in t.RANK_CASES if c["nw"] == nw}
        wg = 64 * nw
        assert t.expected_rank(rc["none"])["total"].tolist() == [0, 0]
        f, n = t.rank_inputs(rc["all"])
        assert t.expected_rank(rc["all"])["total"].tolist() == list(n)
        f, n = t.rank_inputs(rc["last_lane_of_last_wave"])
        assert n[0] == wg and np.flatnonzero(f[0, :wg]).tolist() == [wg - 1]
        f, n = t.rank_inputs(rc["partial_second_batch"])
        assert wg < n[0] < 2 * wg and n[0] % wg
    # ---- KEEP
    assert t.KEEP_N[0] == 2500 and {c["filter"] for c in t.KEEP_CASES} == {0, 1}
    for c in t.KEEP_CASES:
        if c["filter"]:
            keys, kth, limit = t.keep_inputs(c)
            q0 = t.expected_keep(c)["count"][0]
            assert {"below": limit < q0, "equal_row0": limit == q0, "equal_row1": limit == t.expected_keep(c)["count"][1], "above": limit > q0}[c["limit"]]
            assert (keys[0, :2500] == np.uint64(kth)).sum() > 1
    # ---- CUT
    ct = {c["id"]: (c, t.expected_cut(c)) for c in t.CUT_CASES}
    c, e = ct["fewer_than_limit"]
    assert (e["base"] < c["limit"]).all() and (e["nkept"] == e["base"]).all() and e["status"][0] == 0
    c, e = ct["plateau_across_the_cut"]
    s, _ = t.cut_inputs(c)
    kept = e["kslot"][0, : e["nkept"][0]]
    out = np.setdiff1d(np.arange(e["base"][0]), kept)
    low = R.order_key(s[0][kept]).min()
    assert e["nkept"][0] == c["limit"] < e["base"][0] and (R.order_key(s[0][out]) == low).any(), "equal scores on both sides of the cut"
    assert kept[R.order_key(s[0][kept]) == low].min() > out[R.order_key(s[0][out]) == low].max(), "the later slots of the plateau stay"
    c, e = ct["limit_0_three_tiles"]
    assert c["limit"] == 0 and e["nkept"][0] == 700 and e["status"][0] == 0
    assert ct["more_than_kcap"][1]["status"][0] == 2 and ct["more_than_kcap"][1]["base"][0] > ct["more_than_kcap"][0]["kcap"]
    assert ct["zero_total"][1]["base"][0] == 0 and ct["zero_total"][1]["nkept"][0] == 0
    # ---- SuperPoint's stage
    sp = {c["id"]: c for c in t.SP_CASES}
    assert {c["maxk"] for c in t.SP_CASES} >= {-1, 0, 1, 2, 3, 64, 65, 128, 129, 1024, 1025, 2049}
    full = t.expected_sp(sp["k-1"])
    assert 2500 < full["nk"][0] < 3500 and full["nk"][1] != full["nk"][0]
    m = t.sp_inputs(sp["k1"])
    idx, sb, n, _ = R.superpoint_select(m[0], t.SP_THR, t.SP_BORDER, 1 << 20, 1 << 20)
    ranked = np.sort(sb)[::-1]
    assert all(ranked[k - 1] == ranked[k] for k in (1, 2, 3, 64, 65, 128, 129, 1024, 1025, 2049)), "equal score bits straddle every cut"
    assert len(set(t.expected_sp(sp["all_candidates_equal"])["scores"][0, :129])) == 1
    e = t.expected_sp(sp["n_below_k"])
    assert (e["nk"] < 4000).all() and (e["nk"] > 0).all() and e["status"][0] == 0
    assert t.expected_sp(sp["kcap_below_k_topk"])["status"][0] == 2 and t.expected_sp(sp["kcap_below_k_topk"])["nk"][0] == 300
    assert t.expected_sp(sp["kcap_below_n_all"])["status"][0] == 2
    assert t.expected_sp(sp["cand_cap_below_n"])["status"][0] == 1
    e = t.expected_sp(sp["border_band_only"])
    assert e["nk"].tolist() == [0, 0] and (t.sp_inputs(sp["border_band_only"]) > t.SP_THR).sum() > 100
    big = sp["k_above_topk_max"]
    e = t.expected_sp(big)
    assert big["maxk"] == R.SP_TOPK_MAX + 1 and t.sp_inputs(big).shape[1:] == (160, 160) and e["status"][0] == 4 and e["nk"][0] == 0 and e["nk"][1] > 0
    assert (e["scores"][0] == t.NAN_F32).all() and (e["keypoints"][0] == t.NAN_F32).all(), "nothing is written under status 4"
    # ---- DISK's stage
    dk = {c["id"]: c for c in t.DK_CASES}
    assert {c["maxk"] for c in t.DK_CASES} >= {"all", "0", "1", "n-1", "n", "n+5"} and {c["window"] for c in t.DK_CASES} == {1, 5}
    assert t.expected_dk(dk["maxk_all"])["nk"][0] > 1024, "two batches of 1024"
    e, p = t.expected_dk(dk["plateau_at_the_cut"]), t.dk_params(dk["plateau_at_the_cut"])
    assert 0 < e["nk"][0] < p["maxk"], "strictly above the (maxk + 1)-th keeps fewer than maxk"
    assert t.expected_dk(dk["kcap_below_the_limit"])["status"][0] == 2 and t.expected_dk(dk["kcap_below_the_limit"])["nk"][0] == 100
    assert t.expected_dk(dk["zero_candidates"])["nk"][0] == 0 and t.expected_dk(dk["zero_candidates"])["nk"][1] > 0
    m = t.dk_inputs(dk["maxk_all"])
    assert ((m[0][:, 1:] == m[0][:, :-1]) & (m[0][:, 1:] > 0)).any(), "equal neighbours: the first maximum of a window wins"


def test_every_block_of_select_h_has_a_row():
    """a new kernel or device function in select.h fails here until it is named in COVERAGE and an op of the probe runs it"""
    src = re.sub(r"__launch_bounds__\(\d+\)", "", open(SELECT_H).read())
    names = set(re.findall(r"__(?:global|device)__[^;{(]*?(\w+)\s*\(", src))
    assert names == set(COVERAGE), names ^ set(COVERAGE)
    from imcui_hip import backend

    tables = _tables(_t())
    for name, ops in COVERAGE.items():
        for op in ops:
            assert op in backend.SELECT_OPS and tables[op][0], (name, op)
    probe = open(os.path.join(os.path.dirname(SELECT_H), "select_probe.hip")).read()
    for name in set(COVERAGE) - {"wave_ordered_rank", "operator", "score_index_key"}:  # (those three are reached through their callers)
        for caller in VIA.get(name, ()):
            body = re.search(r"\b" + caller + r"\([^;{]*\{.*?\n}", src, re.S)
            assert body and re.search(r"\b" + name + r"\b", body.group(0)), (name, caller)
            name = caller
        assert re.search(r"\b" + name + r"\b", probe), name
    assert "EmitScoreIndex" in probe
