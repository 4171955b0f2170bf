"""LANet throughput on one MI355X: the HIP path (default conf, split arithmetic, max_keypoints 5000, one batched `forward_batched`
call, no host synchronisation) vs the torch restatement (tests/lanet_reference.py + the wrapper's rule) run by PyTorch-ROCm in fp32 on
the same GPU, one image per call as the reference's wrapper runs it.  Alternated, after warm-up; the median of `--reps` calls; one JSON
line per row, appended to profiles/lanet_bench.jsonl.

    python tools/lanet_bench.py [--reps 7] [--rows 480x640:16,480x640:1,1200x1600:4] [--commit <base commit>] [--out <file>]
                                [--hip-only] [--trace [--trace-row 480x640:16 --trace-out <file>]]

Every row also times the descriptor head both ways on the key-points of its first image: the sparse head (imcui_hip_lanet_desc_probe)
against the dense form the forward never runs (imcui_hip_lanet_dense_levels, then torch's grid_sample of the three maps, the weighted
sum and the norm).

--trace: ONE `rocprofv3 --kernel-trace --stats` run of the 480x640 x 16 row in a fresh child process (`--hip-only`, two warm-up and
three timed calls), summarised into profiles/lanet_kernel_trace.txt.
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
        lines = [f"rocprofv3 --kernel-trace --stats of tools/lanet_bench.py --hip-only --rows {args.trace_row} --reps 3 (two warm-up calls, three timed forward_batched",
                 f"calls and the two descriptor-head timings), one MI355X, split arithmetic, base commit {args.commit}.  Kernel statistics:", "",
                 " calls   total ms     avg us  share %  kernel"]  # fmt: skip
        rows = sorted(csv.DictReader(open(stats[0])), key=lambda q: -float(q["TotalDurationNs"]))
        tot = sum(float(q["TotalDurationNs"]) for q in rows)
        for q in rows[:24]:
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
    ap.add_argument("--hip-only", action="store_true", help="time the HIP path alone (for a kernel trace)")
    ap.add_argument("--trace", action="store_true", help="only the rocprofv3 run of --trace-row, in a child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lanet_bench.jsonl"))
    ap.add_argument("--trace-out", default=os.path.join(ROOT, "profiles", "lanet_kernel_trace.txt"))
    ap.add_argument("--trace-row", default="480x640:16", help="the row the --trace run profiles")
    args = ap.parse_args()
    if args.trace:
        return trace(args)
    import lanet_reference as R
    from imcui_hip import backend
    from imcui_hip.hloc.extractors.lanet import LANet
    from imcui_hip.synth_weights import lanet_synth_state

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    sd = lanet_synth_state(0)
    conf = {"keypoint_threshold": 0.1, "max_keypoints": 5000}
    plugin = LANet({**conf, "state_dict": sd}).eval().to(dev)
    ref = None if args.hip_only else R.build(sd).to(dev)
    for spec in args.rows.split(","):
        hw, b = spec.split(":")
        h, w = map(int, hw.split("x"))
        B = int(b)
        x = torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(h + B)).to(dev)

        def run_hip():
            return plugin.forward_batched(x)

        def run_torch():  # one image per call, the wrapper's rule behind it (lanet.py:41-57)
            with torch.no_grad():
                for i in range(B):
                    score, coord, desc = ref(x[i : i + 1])
                    R.wrapper_rule(score[0, 0].flatten(), coord[0].flatten(1).t(), desc[0].flatten(1).t(), conf["keypoint_threshold"], conf["max_keypoints"])

        runs = (("hip", run_hip),) if args.hip_only else (("hip", run_hip), ("torch", run_torch))
        for _, f in runs:  # warm-up (MIOpen picks its kernels here)
            f()
            f()
        torch.cuda.synchronize()
        t = {name: [] for name, _ in runs}
        for _ in range(args.reps):
            for name, f in runs:
                t[name].append(once_ms(f))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        # ---- the descriptor head both ways on the key-points of image 0
        out = plugin.forward_batched(x[:1], want_maps=True)
        n = int(out["num_keypoints"][0])
        kp = out["keypoints"][0, :n].contiguous()
        cells = (torch.floor(kp[:, 1] / 8) * (w // 8) + torch.floor(kp[:, 0] / 8)).long().clamp(0, (h // 8) * (w // 8) - 1)
        aw = out["cell_aware"][0][cells].contiguous()  # (any weights do for a timing; these are close to the key-points' own)
        impl, packed = plugin._impl, plugin.packed
        x2, x3, x4 = out["x2"], out["x3"], out["x4"]

        def sparse():
            return impl.desc_probe(packed, x2[0], x3[0], x4[0], h, w, kp, aw)

        def dense():
            d2, d3 = impl.dense_levels(packed, x2, x3)
            grid = R.normalised_grid(kp, h, w).view(1, 1, -1, 2)
            return R.blend_levels(d2.permute(0, 3, 1, 2), d3.permute(0, 3, 1, 2), x4.permute(0, 3, 1, 2), grid, aw.t().reshape(1, 3, 1, -1))

        head = {}
        if n > 0:
            for name, f in (("sparse", sparse), ("dense", dense)):
                f()
                f()
                head[name] = sorted(once_ms(f) for _ in range(args.reps))[args.reps // 2]
            diff = (sparse() - dense()[0, :, 0].t()).abs().max().item()
        rec = {"commit": args.commit, "size": f"{h}x{w}", "batch": B, "keypoints_image0": n, "hip_ms": med["hip"], "hip_images_per_s": 1e3 * B / med["hip"]}
        if "torch" in med:
            rec.update(torch_fp32_ms=med["torch"], torch_fp32_images_per_s=1e3 * B / med["torch"], speedup=med["torch"] / med["hip"])
        if head:
            rec.update(desc_head_sparse_ms=head["sparse"], desc_head_dense_ms=head["dense"], desc_head_max_abs_diff=diff)
        line = json.dumps(rec)
        print(line, flush=True)
        if not args.hip_only:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as fd:
                fd.write(line + "\n")


if __name__ == "__main__":
    main()
