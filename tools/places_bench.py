"""CosPlace / EigenPlaces throughput on one MI355X: the HIP path (split arithmetic, one batched `forward_batched` call, no host
synchronisation) vs the torch restatement (tests/places_reference.py) run by PyTorch-ROCm in fp32 on the same GPU (MIOpen convolutions,
rocBLAS head), which is what the reference's wrappers run once torch.hub has built upstream's module.  Alternated, after warm-up; the
median of `--reps` calls; one JSON line per row, appended to profiles/places_bench.jsonl.

    python tools/places_bench.py [--reps 7] [--rows 768x1024:1,768x1024:8,480x640:16] [--nets 18:512,50:2048] [--commit <base commit>]
                                 [--hip-only] [--trace [--trace-row 768x1024:1 --trace-out <file>]]

--trace: ONE `rocprofv3 --kernel-trace --stats` run of the ResNet-50 / 2048 768x1024 x 8 row in a fresh child process (`--hip-only`, two
warm-up and three timed calls), summarised into profiles/places_kernel_trace.txt: the kernel statistics, and the launches grouped by
kernel and grid size so that the launches of one stage of the trunk can be told apart.

One MODEL, not a measurement, goes with every row: the arithmetic of the stem (2 x 147 x 64 per conv1 position) and of the trunk
(2 x k x k x cin x cout per output pixel of every convolution at its resolution, the downsamples included); the split arithmetic executes
three f16 products per element pair of the trunk.  GeM and the head are 2 x F x D + a few F per image and are left out.
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

DEPTHS = {18: (2, 2, 2, 2), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}


def down(n):
    return (n - 1) // 2 + 1


def model(backbone, h, w):
    """(stem FLOP, trunk FLOP, layer4 FLOP, layer4 pixels) per image."""
    hc, wc = down(h), down(w)
    stem = 2.0 * 147 * 64 * hc * wc
    hh, ww, cin, bott = down(hc), down(wc), 64, backbone != 18
    trunk = l4 = 0.0
    for L, depth in enumerate(DEPTHS[backbone]):
        width = 64 << L
        cout = 4 * width if bott else width
        for i in range(depth):
            s = 2 if (i == 0 and L > 0) else 1
            ho, wo = (down(hh), down(ww)) if s == 2 else (hh, ww)
            if bott:
                f = 2.0 * cin * width * hh * ww + 2.0 * 9 * width * width * ho * wo + 2.0 * width * cout * ho * wo
            else:
                f = 2.0 * 9 * cin * width * ho * wo + 2.0 * 9 * width * width * ho * wo
            if s != 1 or cin != cout:
                f += 2.0 * cin * cout * ho * wo
            trunk += f
            l4 += f if L == 3 else 0.0
            hh, ww, cin = ho, wo, cout
    return stem, trunk, l4, hh * ww


def median_ms(f, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * sorted(ts)[len(ts) // 2]


def trace(args):
    """The kernel trace in a run of its own: a fresh child under rocprofv3, nothing else collected."""
    out = args.trace_out
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--hip-only", "--rows", args.trace_row, "--nets",
               "50:2048", "--reps", "3"]  # fmt: skip
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise SystemExit(f"rocprofv3 run failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        stats = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)
        traces = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
        if not stats or not traces:
            raise SystemExit(f"rocprofv3 left no kernel_stats / kernel_trace csv under its output directory: {os.listdir(d)}")
        lines = [f"rocprofv3 --kernel-trace --stats of tools/places_bench.py --hip-only --rows {args.trace_row} --nets 50:2048 --reps 3 (two warm-up calls and three",
                 f"timed forward_batched calls of {args.trace_row.split(':')[1]} image(s), ResNet-50 / 2048), one MI355X, split arithmetic, base commit {args.commit}.  Kernel statistics:", "",
                 " calls   total ms     avg us  share %  kernel"]  # fmt: skip
        if stats:
            rows = sorted(csv.DictReader(open(stats[0])), key=lambda q: -float(q["TotalDurationNs"]))
            tot = sum(float(q["TotalDurationNs"]) for q in rows)
            for q in rows[:20]:
                lines.append(f'{int(q["Calls"]):6d} {float(q["TotalDurationNs"]) / 1e6:10.3f} {float(q["AverageNs"]) / 1e3:10.1f} {100 * float(q["TotalDurationNs"]) / tot:8.2f}  {q["Name"][:110]}')
        if traces:
            groups = {}
            for q in csv.DictReader(open(traces[0])):
                name = q.get("Kernel_Name", "?")
                wg = max(1, int(q.get("Workgroup_Size_X", 1) or 1))
                nwg = int(q.get("Grid_Size_X", 0) or 0) // wg * max(1, int(q.get("Grid_Size_Y", 1) or 1)) * max(1, int(q.get("Grid_Size_Z", 1) or 1))
                g = groups.setdefault((name[:70], nwg), [0, 0.0])
                g[0] += 1
                g[1] += float(q["End_Timestamp"]) - float(q["Start_Timestamp"])
            tot = sum(v[1] for v in groups.values())
            lines += ["", "Launches grouped by kernel and workgroup count (the trunk's stages differ in their grids: layer1 has the most workgroups, layer4 the fewest):", "",
                      " calls  workgroups   total ms     avg us  share %  kernel"]  # fmt: skip
            for (name, nwg), (n, ns) in sorted(groups.items(), key=lambda kv: -kv[1][1])[:40]:
                lines.append(f"{n:6d} {nwg:11d} {ns / 1e6:10.3f} {ns / n / 1e3:10.1f} {100 * ns / tot:8.2f}  {name}")
    with open(out, "w") as fd:
        fd.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="768x1024:1,768x1024:8,480x640:16")
    ap.add_argument("--nets", default="18:512,50:2048", help="backbone:fc_output_dim, comma separated")
    ap.add_argument("--commit", default="", help="base commit the lines are stamped with")
    ap.add_argument("--hip-only", action="store_true", help="time the HIP path alone (for a kernel trace)")
    ap.add_argument("--trace", action="store_true", help="only the rocprofv3 run of the ResNet-50 768x1024 x 8 row, in a child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "places_bench.jsonl"))
    ap.add_argument("--trace-out", default=os.path.join(ROOT, "profiles", "places_kernel_trace.txt"))
    ap.add_argument("--trace-row", default="768x1024:8", help="the row the --trace run profiles")
    args = ap.parse_args()
    if args.trace:
        return trace(args)
    import places_reference as rr
    from imcui_hip import backend
    from imcui_hip.synth_weights import places_synth_state

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    lines = []
    for net in args.nets.split(","):
        backbone, dim = map(int, net.split(":"))
        sd = places_synth_state(backbone, dim, 0)
        packed = backend.pack_places(sd, backbone, dim).to(dev)
        hip = backend.PlacesHIP(backbone, dim)
        ref = None if args.hip_only else rr.build(sd, backbone, dim).to(dev)
        for spec in args.rows.split(","):
            hw, b = spec.split(":")
            h, w_ = map(int, hw.split("x"))
            B = int(b)
            x = torch.rand(B, 3, h, w_, generator=torch.Generator().manual_seed(h + B)).to(dev)
            stem, trunk, l4, n4 = model(backbone, h, w_)

            def run_hip():
                return hip.forward_batched(packed, x)["global_descriptor"]

            def run_torch():
                with torch.no_grad():
                    return ref(rr.normalize_rgb(x))

            runs = (("hip", run_hip),) if args.hip_only else (("hip", run_hip), ("torch", run_torch))
            for _, f in runs:  # warm-up (MIOpen picks its kernels here)
                f()
                f()
            torch.cuda.synchronize()
            t = {name: [] for name, _ in runs}
            for _ in range(args.reps):
                for name, f in runs:
                    t[name].append(median_ms(f, 1))
            med = {k: sorted(v)[len(v) // 2] * 1e-3 for k, v in t.items()}
            rec = {"commit": args.commit, "backbone": f"ResNet{backbone}", "fc_output_dim": dim, "size": f"{h}x{w_}", "batch": B, "hip_ms": 1e3 * med["hip"],
                   "hip_images_per_s": B / med["hip"], "model_stem_gflop_per_image": stem / 1e9, "model_trunk_gflop_per_image": trunk / 1e9,
                   "model_layer4_gflop_per_image": l4 / 1e9, "layer4_gemm_rows": B * n4, "model_tflops": (stem + trunk) * B / med["hip"] / 1e12,
                   "executed_split_tflops": (stem + 3 * trunk) * B / med["hip"] / 1e12}  # fmt: skip
            if "torch" in med:
                err = (run_hip() - run_torch()).abs().max().item() / run_torch().abs().max().item()
                rec.update(torch_ms=1e3 * med["torch"], torch_fp32_images_per_s=B / med["torch"], speedup=med["torch"] / med["hip"], max_rel_diff_vs_torch=err)
            lines.append(rec)
            line = json.dumps(rec)
            print(line, flush=True)
            if not args.hip_only:
                os.makedirs(os.path.dirname(args.out), exist_ok=True)
                with open(args.out, "a") as fd:
                    fd.write(line + "\n")
        del packed, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
