"""SIFT extractor throughput on one MI355X: `forward_batched` images/s of the HIP path (csrc/sift.hip), default conf with
`max_keypoints` 4096.  No CPU cv2 exists where this runs, so the numbers are absolute: no speed-up is claimed.  One JSON line per size,
stamped with the commit, appended to profiles/sift_bench.jsonl.

    python tools/sift_bench.py [--reps 7] [--sizes 480x640:16,480x640:1,1200x1600:4,60x80:1] [--commit ID]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/sift_bench.py --profile-run      # one size, a few calls, no timing
    python tools/sift_bench.py --stats DIR/*_results.db | *_kernel_stats.csv [--commit ID]    # per-kernel shares of that run

The pyramid's bytes are a MODEL of buffer traffic, not a counter: every level is written once and read once by the next blur (halo rows and
columns of a tile come from the cache), the DoG is never stored: 8 bytes per pixel and level.  `--stats` divides them by the time of the
gray / blur / down-sampling kernels and prints the result beside the HBM figure a copy kernel reaches on this part.
The 60x80 entry is a proxy for the tail octaves: its whole pyramid is what a 480x640 image has from octave 3 on, one launch per level.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "image-matching-webui_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

HBM_COPY_TBPS = 6.29  # what a float4 copy kernel reaches on one MI355X (8.0 TB/s specified)
PROFILE_SIZE = (480, 640, 16)


def commit_id(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001
        return "unknown"


def pyramid_bytes(lib, B, h, w, layers=4):
    return 8.0 * lib.imcui_hip_sift_pyramid_floats(B, h, w, layers)


def append(path, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as fd:
        fd.write(line + "\n")


def stats(args):
    from imcui_hip import load_library

    if args.stats.endswith(".db"):  # rocprofv3's default output: an SQLite file whose `kernels` view holds one row per dispatch
        import sqlite3

        name, total, calls = "name", "total_ns", "calls"
        rows = [dict(zip((name, calls, total), r)) for r in sqlite3.connect(args.stats).execute("select name, count(*), sum(duration) from kernels group by name")]
    else:  # --output-format csv: *_kernel_stats.csv
        rows = list(csv.DictReader(open(args.stats)))
        name = next(k for k in rows[0] if k.lower() == "name")
        total = next(k for k in rows[0] if "total" in k.lower() and "ns" in k.lower())
        calls = next(k for k in rows[0] if k.lower() in ("calls", "count"))
    t = {}
    for r in rows:
        if "sf_" in r[name]:
            key = r[name].split("(")[0].split("<")[0].replace("void ", "")
            t[key] = t.get(key, 0.0) + float(r[total])
    n_calls = max(int(r[calls]) for r in rows if "sf_final_kernel" in r[name])
    whole = sum(t.values())
    h, w, B = PROFILE_SIZE
    pyr_ns = sum(v for k, v in t.items() if any(s in k for s in ("sf_blur", "sf_down", "sf_gray"))) / n_calls
    pb = pyramid_bytes(load_library(), B, h, w)
    append(args.out, {"commit": commit_id(args.commit), "kind": "kernel_shares", "size": f"{h}x{w}", "batch": B, "calls": n_calls,
                      "gpu_ms_per_call": whole / n_calls / 1e6, "shares": {k: round(v / whole, 4) for k, v in sorted(t.items(), key=lambda kv: -kv[1])},
                      "pyramid_ms_per_call": pyr_ns / 1e6, "pyramid_modelled_mb": pb / 1e6, "pyramid_tb_per_s": pb / pyr_ns / 1e3, "hbm_copy_tb_per_s": HBM_COPY_TBPS})  # fmt: skip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="480x640:16,480x640:1,1200x1600:4,60x80:1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift_bench.jsonl"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--stats", default=None)
    args = ap.parse_args()
    if args.stats:
        return stats(args)
    import numpy as np
    import torch

    import sift_reference as R
    from imcui_hip import load_library
    from imcui_hip.hloc.extractors.sift import SIFT

    dev = torch.device("cuda:0")
    m = SIFT({"max_keypoints": 4096}).eval().to(dev)
    lib = load_library()
    sizes = [PROFILE_SIZE] if args.profile_run else [tuple(map(int, s.replace(":", "x").split("x"))) for s in args.sizes.split(",")]
    for h, w, B in sizes:
        x = torch.from_numpy(np.stack([R.seeded_image(h, w, 10 + i)[None] for i in range(B)])).to(dev)
        out, counts = m.forward_checked(x)  # warm-up; also settles the capacities
        ccap = max(m._impl.default_ccap(h, w), int(out["counts"][:, :2].max()))
        for _ in range(2):
            m.forward_batched(x, ccap=ccap)
        torch.cuda.synchronize()
        if args.profile_run:
            continue
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.forward_batched(x, ccap=ccap)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        med = sorted(ts)[len(ts) // 2]
        append(args.out, {"commit": commit_id(args.commit), "kind": "throughput", "size": f"{h}x{w}", "batch": B, "mean_keypoints": sum(counts) / B,
                          "mean_extrema": float(out["counts"][:, 0].float().mean()), "images_per_s": B / med, "ms_per_call": 1e3 * med, "min_ms": 1e3 * min(ts),
                          "pyramid_modelled_mb_per_image": pyramid_bytes(lib, 1, h, w) / 1e6})  # fmt: skip


if __name__ == "__main__":
    main()
