"""SFD2 throughput on one MI355X: the HIP path (default conf: max_keypoints 4096, conf_th 0.001; split arithmetic, one batched
`forward_batched` call, no host synchronisation) vs the torch restatement (tests/sfd2_reference.py: Normalize + `extract_local_global`)
run by PyTorch-ROCm in fp32 on the same GPU, one image per call as the reference's wrapper runs it.  Alternated, after warm-up; the
median of `--reps` calls; one JSON line per row, appended to profiles/sfd2_bench.jsonl.

    python tools/sfd2_bench.py [--reps 7] [--rows 480x640:16,480x640:1,1200x1600:4] [--commit <base commit>] [--out <file>]
                               [--hip-only] [--trace [--trace-row 480x640:16 --trace-out <file>]]

Every row also times the grouped 3x3 convolution alone (imcui_hip_sfd2_gconv_probe) on a 256-channel map of the batch's 1/4-resolution
size and reports its achieved bytes/s against the bytes it must move (the map read once and written once) and that figure's share of the
6.29 TB/s device copy this project measured.

--trace: ONE `rocprofv3 --kernel-trace --stats` run of the 480x640 x 16 row in a fresh child process (`--hip-only`, two warm-up and
three timed calls), summarised into profiles/sfd2_kernel_trace.txt.
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
        lines = [f"rocprofv3 --kernel-trace --stats of tools/sfd2_bench.py --hip-only --rows {args.trace_row} --reps 3 (two warm-up calls, three timed",
                 f"forward_batched calls and the grouped-convolution timing), one MI355X, split arithmetic, base commit {args.commit}.  Kernel statistics:", "",
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sfd2_bench.jsonl"))
    ap.add_argument("--trace-out", default=os.path.join(ROOT, "profiles", "sfd2_kernel_trace.txt"))
    ap.add_argument("--trace-row", default="480x640:16", help="the row the --trace run profiles")
    args = ap.parse_args()
    if args.trace:
        return trace(args)
    import sfd2_reference as R
    from imcui_hip import backend
    from imcui_hip.hloc.extractors.sfd2 import SFD2
    from imcui_hip.synth_weights import sfd2_synth_state

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    sd = sfd2_synth_state(0)
    plugin = SFD2({"state_dict": sd}).eval().to(dev)  # the default conf
    conf = dict(SFD2.default_conf)
    ref = None if args.hip_only else R.load_sfd2(state_dict=sd).to(dev)
    for spec in args.rows.split(","):
        hw, b = spec.split(":")
        h, w = map(int, hw.split("x"))
        B = int(b)
        x = torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(h + B)).to(dev)

        def run_hip():
            return plugin.forward_batched(x)

        def run_torch():  # one image per call: Normalize, then extract_local_global (sfd2.py:36-38)
            with torch.no_grad():
                for i in range(B):
                    ref.extract_local_global({"image": R.normalise_image(x[i : i + 1])}, conf)

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
        n = int(plugin.forward_batched(x)["num_keypoints"][0])
        # ---- the grouped 3x3 convolution alone, on a 256-channel map of the batch's 1/4-resolution size
        _, _, Hc, Wc = backend.sfd2_map_sizes(h, w)
        g = torch.Generator().manual_seed(1)
        xm = torch.randn(B, Hc, Wc, 256, generator=g).to(dev)
        wg, shift = (torch.randn(256, 8, 3, 3, generator=g) / 8.5).to(dev), torch.zeros(256, device=dev)
        impl = plugin._impl

        def run_gconv():
            return impl.gconv_probe(xm, wg, shift, True)

        run_gconv()
        run_gconv()
        gms = sorted(once_ms(run_gconv) for _ in range(args.reps))[args.reps // 2]
        tbps = 2 * xm.numel() * 4 / gms / 1e9
        rec = {"commit": args.commit, "size": f"{h}x{w}", "batch": B, "keypoints_image0": n, "hip_ms": med["hip"], "hip_images_per_s": 1e3 * B / med["hip"]}
        if "torch" in med:
            rec.update(torch_fp32_ms=med["torch"], torch_fp32_images_per_s=1e3 * B / med["torch"], speedup=med["torch"] / med["hip"])
        rec.update(gconv_ms=gms, gconv_modelled_TBps=tbps, gconv_share_of_copy=tbps / COPY_TBPS)
        line = json.dumps(rec)
        print(line, flush=True)
        if not args.hip_only:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as fd:
                fd.write(line + "\n")


if __name__ == "__main__":
    main()
