"""LiftFeat extractor throughput on one MI355X: the HIP path (default conf, split arithmetic, max_keypoints 5000, one batched
`forward_batched` call, no host synchronisation), alternated with two comparisons on the same images:
  (a) the torch restatement (tests/liftfeat_reference.py) run by PyTorch-ROCm in fp32 on the same card, one image per call with its
      synchronising `nonzero`, as imcui/hloc/extractors/liftfeat.py runs it;
  (b) the XFeat call of this backend (the same trunk): what lifting and the normal head add.
After warm-up; the median of `--reps` calls; one JSON line per row, appended to profiles/liftfeat_bench.jsonl.

    python tools/liftfeat_bench.py [--reps 7] [--rows 480x640:16,480x640:1,1200x1600:4] [--commit <base commit>] [--out <file>]
    python tools/liftfeat_bench.py --trace [--trace-row 480x640:16]

Every row also times the three up-conv stages alone (imcui_hip_liftfeat_upconv_probe) on maps of the batch's sizes.  Their HBM figure is a
MODEL of compulsory traffic, not a measurement: per 1/8-resolution cell the stages read 64, 4 x 32 and 16 x 16 floats and write 4 x 32,
16 x 16 and 192 (the up-sampled maps and the 3x3 windows are LDS / cache traffic), 1024 floats = 4 KiB per cell, against the 6.29 TB/s
device-to-device copy figure.

`--trace` runs `rocprofv3 --kernel-trace --stats` on the HIP path of one row in a child process of its own and summarises it into
profiles/liftfeat_kernel_trace.txt.
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

import torch  # noqa: E402

COPY_TBPS = 6.29  # the device-to-device copy figure of this project's measurements (README)
LAUNCHES_PER_CALL = 45  # 26 kernels of csrc/liftfeat.hip and its shared headers + 19 GEMM launches, whatever the batch (plus one 4-byte memset)
UPCONV_BYTES_PER_CELL = 4096.0


def once_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def trace(args):
    """The kernel trace in a run of its own: a fresh child under rocprofv3, nothing else collected."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--hip-only", "--rows", args.trace_row,
               "--reps", "3"]  # fmt: skip
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise SystemExit(f"rocprofv3 run failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        stats = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)
        if not stats:
            raise SystemExit(f"rocprofv3 left no kernel_stats csv under its output directory: {os.listdir(d)}")
        lines = [f"rocprofv3 --kernel-trace --stats of tools/liftfeat_bench.py --hip-only --rows {args.trace_row} --reps 3 (two warm-up calls and three timed",
                 f"calls each of LiftFeat's forward_batched, XFeat's and the up-conv stages alone), one MI355X, split arithmetic, base commit {args.commit}.",
                 "Kernel statistics:", "", " calls   total ms     avg us  share %  kernel"]  # fmt: skip
        rows = sorted(csv.DictReader(open(stats[0])), key=lambda q: -float(q["TotalDurationNs"]))
        tot = sum(float(q["TotalDurationNs"]) for q in rows)
        for q in rows[:28]:
            lines.append(f'{int(q["Calls"]):6d} {float(q["TotalDurationNs"]) / 1e6:10.3f} {float(q["AverageNs"]) / 1e3:10.1f} {100 * float(q["TotalDurationNs"]) / tot:8.2f}  {q["Name"][:110]}')
    os.makedirs(os.path.dirname(args.trace_out), exist_ok=True)
    with open(args.trace_out, "w") as fd:
        fd.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="480x640:16,480x640:1,1200x1600:4", help="HxW:batch, comma separated")
    ap.add_argument("--commit", default="", help="base commit the lines are stamped with")
    ap.add_argument("--hip-only", action="store_true", help="time the HIP paths alone (for a kernel trace)")
    ap.add_argument("--trace", action="store_true", help="only the rocprofv3 run of --trace-row, in a child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "liftfeat_bench.jsonl"))
    ap.add_argument("--trace-out", default=os.path.join(ROOT, "profiles", "liftfeat_kernel_trace.txt"))
    ap.add_argument("--trace-row", default="480x640:16", help="the row the --trace run profiles")
    args = ap.parse_args()
    if args.trace:
        return trace(args)
    import torch.nn.functional as F

    import liftfeat_reference as R
    from imcui_hip import backend
    from imcui_hip.hloc.extractors.liftfeat import Liftfeat
    from imcui_hip.hloc.extractors.xfeat import XFeat
    from imcui_hip.synth_weights import liftfeat_synth_state, xfeat_state_dict

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    sd = liftfeat_synth_state(0)
    plugin = Liftfeat({"state_dict": sd}).eval().to(dev)  # the default conf: threshold 0.05, max_keypoints 5000
    xfeat = XFeat({"max_keypoints": 5000, "state_dict": xfeat_state_dict(0)}).eval().to(dev)
    conf = dict(Liftfeat.default_conf)
    ref = None if args.hip_only else R.load_model(sd).to(dev)
    for spec in args.rows.split(","):
        hw, b = spec.split(":")
        h, w = map(int, hw.split("x"))
        B = int(b)
        x = (torch.randint(0, 256, (B, 3, h, w), generator=torch.Generator().manual_seed(h + B), dtype=torch.uint8).float() / 255.0).to(dev)

        def run_hip():
            return plugin.forward_batched(x)

        def run_xfeat():
            return xfeat.forward_batched(x)

        def run_torch():  # one image per call: pad, / 255, forward1, forward2, the selection and the wrapper's cut (liftfeat.py:35-46)
            with torch.no_grad():
                for i in range(B):
                    xi = F.pad(x[i : i + 1] * 255, (0, (-w) % 32, 0, (-h) % 32)) / 255
                    M1, K1, D1 = ref.forward1(xi)
                    boosted = ref.forward2(M1, K1, D1)
                    heat = R.X.unshuffle_heatmap(F.softmax(K1, 1)[:, :64])
                    R.wrapper_cut(R.select(heat, boosted, h, w, conf["keypoint_threshold"]), conf["max_keypoints"])

        runs = (("hip", run_hip), ("xfeat", run_xfeat)) + (() if args.hip_only else (("torch", run_torch),))
        for _, f in runs:  # warm-up (MIOpen picks its kernels here)
            f()
            f()
        torch.cuda.synchronize()
        t = {name: [] for name, _ in runs}
        for _ in range(args.reps):
            for name, f in runs:
                t[name].append(once_ms(f))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        n = float(plugin.forward_batched(x)["num_keypoints"].float().mean())
        # ---- the three up-conv stages alone, on maps of the batch's sizes
        Hp, Wp = backend.liftfeat_pad(h), backend.liftfeat_pad(w)
        g = torch.Generator().manual_seed(1)
        maps = [torch.randn(B, Hp >> (3 - s), Wp >> (3 - s), 64 >> s, generator=g).to(dev) for s in range(3)]
        impl = plugin._impl

        def run_upconv():
            for s in range(3):
                impl.upconv_probe(plugin.packed, maps[s], s, fused=(s == 2))

        run_upconv()
        run_upconv()
        ums = sorted(once_ms(run_upconv) for _ in range(args.reps))[args.reps // 2]
        tbps = UPCONV_BYTES_PER_CELL * B * (Hp // 8) * (Wp // 8) / ums / 1e9
        rec = {"commit": args.commit, "size": f"{h}x{w}", "batch": B, "mean_keypoints": n, "launches_per_call": LAUNCHES_PER_CALL, "hip_ms": med["hip"],
               "hip_images_per_s": 1e3 * B / med["hip"], "xfeat_ms": med["xfeat"], "cost_over_xfeat_ms": med["hip"] - med["xfeat"],
               "cost_over_xfeat_ratio": med["hip"] / med["xfeat"]}  # fmt: skip
        if "torch" in med:
            rec.update(torch_fp32_ms=med["torch"], torch_fp32_images_per_s=1e3 * B / med["torch"], speedup=med["torch"] / med["hip"])
        rec.update(upconv_ms=ums, upconv_modelled_TBps=tbps, upconv_share_of_copy=tbps / COPY_TBPS)
        line = json.dumps(rec)
        print(line, flush=True)
        if not args.hip_only:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as fd:
                fd.write(line + "\n")


if __name__ == "__main__":
    main()
