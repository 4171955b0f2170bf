"""AdaLAM (`adalam`) timings on one MI355X: the HIP path (B pairs per `forward_batched` call, no host synchronisation inside a call)
vs the float32 numpy restatement tests/adalam_reference.py on the host of the same machine, one pair per call.  `sift`-shaped input:
N x N key-points with scales and orientations, D = 128.  Median of `--reps` calls after warm-up; one JSON line per row, appended to
profiles/adalam_bench.jsonl.

    python tools/adalam_bench.py [--reps 7] [--rows 4096x1,4096x16] [--commit <base commit>] [--out <file>] [--no-numpy]
    python tools/adalam_bench.py --trace      one `rocprofv3 --kernel-trace --stats` run of the 4096 x 16 row, in a process of its own

Per row: hip_ms (the whole call), filter_ms (stages B .. G alone: imcui_hip_adalam_filter on the same putative matches), and
numpy_fp32_ms = B x the restatement's median time for one pair (`--ref-reps` calls of pair 0).  There is no target ratio.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "image-matching-webui_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def once_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def median_ms(f, reps):
    f()
    f()
    return sorted(once_ms(f) for _ in range(reps))[reps // 2]


def trace(args):
    """One kernel-trace run of the 4096 x 16 row (HIP path only) in a child process; prints the kernel shares."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--rows", "4096x16", "--reps", "3",
               "--no-numpy", "--out", os.path.join(tmp, "ignored.jsonl")]  # fmt: skip
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"rocprofv3 failed ({r.returncode}):\n{r.stderr[-2000:]}")
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        with open(files[0]) as fd:
            rows = list(csv.DictReader(fd))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    shares = sorted(((float(r["TotalDurationNs"]) / total, r["Name"], int(r["Calls"])) for r in rows), reverse=True)[:12]
    rec = {"commit": args.commit, "row": "trace 4096x4096x16", "kernel_shares": [{"kernel": n[:60], "share": round(s, 4), "calls": c} for s, n, c in shares]}
    line = json.dumps(rec)
    print(line)
    with open(args.out, "a") as fd:
        fd.write(line + "\n")
    with open(os.path.join(os.path.dirname(args.out), "adalam_kernel_trace.txt"), "w") as fd:
        fd.write("rocprofv3 --kernel-trace --stats of tools/adalam_bench.py --rows 4096x16 --reps 3 --no-numpy (HIP path only)\n")
        for sh, n, c in shares:
            fd.write(f"{100 * sh:6.2f} %  {c:5d} calls  {n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ref-reps", type=int, default=3)
    ap.add_argument("--rows", default="4096x1,4096x16")
    ap.add_argument("--commit", default="", help="base commit the lines are stamped with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adalam_bench.jsonl"))
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if args.trace:
        return trace(args)
    import adalam_reference as R
    from imcui_hip import backend
    from imcui_hip.hloc.matchers.adalam import AdaLAM

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    model = AdaLAM({}).eval().to(dev)
    impl = backend.AdaLAMHIP()
    H, W = R.SIZE
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for row in args.rows.split(","):
        N, B = map(int, row.split("x"))
        scs = [R.make_scene(100 + b, N=N, sigma=0.5, p=0.4, filters=True) for b in range(B)]
        t = lambda k: torch.as_tensor(np.stack([s[k] for s in scs]), dtype=torch.float32, device=dev)  # noqa: E731
        k0, k1, d0, d1 = t("k0"), t("k1"), t("d0"), t("d1")
        so = (t("s0"), t("o0"), t("s1"), t("o1"))
        cnt = torch.full((B,), N, dtype=torch.int32, device=dev)

        def hip():
            return model.forward_batched(k0, k1, d0, d1, cnt, cnt, (W, H), (W, H), scales_oris=so)

        a = model.forward_batched(k0, k1, d0, d1, cnt, cnt, (W, H), (W, H), scales_oris=so, probe=True)

        def filt():
            return impl.filter(k0, k1, a["nn"], a["score"], a["mnn"], cnt, cnt, (W, H), (W, H), model.conf, scales_oris=so, probe=False)

        rec = {"commit": args.commit, "row": f"{N}x{N}x{B}", "D": 128, "hip_ms": median_ms(hip, args.reps), "filter_ms": median_ms(filt, args.reps),
               "seeds": int(a["seed"].sum()), "matches": int((a["matches0"] > -1).sum())}  # fmt: skip
        if not args.no_numpy:
            ts = []
            for _ in range(args.ref_reps):
                t0 = time.perf_counter()
                ref = R.run_scene(scs[0], np.float32)
                ts.append(1e3 * (time.perf_counter() - t0))
            assert np.array_equal(ref["matches0"], a["matches0"][0].cpu().numpy()), "HIP and the float32 restatement disagree"
            per = sorted(ts)[len(ts) // 2]
            rec.update({"numpy_fp32_ms_per_pair": per, "numpy_fp32_ms": per * B, "speedup": per * B / rec["hip_ms"]})
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as fd:
            fd.write(line + "\n")


if __name__ == "__main__":
    main()
