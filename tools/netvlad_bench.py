"""NetVLAD throughput on one MI355X: the HIP path (split arithmetic, one batched `forward_batched` call, no host synchronisation) vs the
torch restatement (tests/netvlad_reference.py) run by PyTorch-ROCm in fp32 on the same GPU (MIOpen convolutions, rocBLAS whitening), which
is what imcui/hloc/extractors/netvlad.py runs.  Alternated, after warm-up; the median of `--reps` calls; one JSON line per row, appended
to profiles/netvlad_bench.jsonl.  The whitening launch (skinny GEMM + fold) is timed alone at B = 1 and B = 16 as well, next to its floor:
512 MB of weights at the 6.29 TB/s this project measured for a copy kernel (about 85 us).

    python tools/netvlad_bench.py [--reps 7] [--rows 768x1024:1,768x1024:8,480x640:16] [--commit <base commit>] [--hip-only] [--no-whiten]

One MODEL, not a measurement, goes with every row: the trunk's arithmetic, 2 x 9 x cin x cout per output pixel of each convolution at its
resolution (the split arithmetic executes three f16 products per element pair of layers 1-12); the NetVLAD layer adds 2 x 512 x 64 x 2
per conv5_3 pixel and the whitening 2 x 32768 x 4096 per image.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "image-matching-webui_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

# (cin, cout, resolution divisor of the layer's output before its pool)
LAYERS = ((3, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 2), (128, 256, 4), (256, 256, 4), (256, 256, 4), (256, 512, 8), (512, 512, 8), (512, 512, 8),
          (512, 512, 16), (512, 512, 16), (512, 512, 16))  # fmt: skip


def model(h, w):
    """(trunk FLOP, NetVLAD-layer FLOP) per image."""
    flop = 0.0
    for cin, cout, d in LAYERS:
        flop += 2.0 * 9 * cin * cout * (h // d) * (w // d)
    return flop, 2.0 * 2 * 512 * 64 * (h // 16) * (w // 16)


def median_ms(f, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="768x1024:1,768x1024:8,480x640:16")
    ap.add_argument("--commit", default="", help="base commit the lines are stamped with")
    ap.add_argument("--hip-only", action="store_true", help="time the HIP path alone (for a kernel trace)")
    ap.add_argument("--no-whiten", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "netvlad_bench.jsonl"))
    args = ap.parse_args()
    import netvlad_reference as rr
    from imcui_hip import backend
    from imcui_hip.synth_weights import netvlad_synth_state

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    whiten = not args.no_whiten
    sd = netvlad_synth_state(0, whiten=whiten)
    packed = backend.pack_netvlad(sd, whiten).to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    hip = backend.NetVLADHIP()
    lines = []

    if whiten:  # the whitening launch alone
        w, b = sd_dev["whiten.weight"], sd_dev["whiten.bias"]
        for B in (1, 16):
            x = torch.nn.functional.normalize(torch.randn(B, 32768, device=dev), dim=1)
            hip.whiten_probe(w, b, x)
            ms = median_ms(lambda: hip.whiten_probe(w, b, x), args.reps)
            t_ms = median_ms(lambda: torch.nn.functional.normalize(torch.nn.functional.linear(x, w, b), dim=1), args.reps)
            lines.append({"commit": args.commit, "row": "whitening launch (probe: GEMM + fold, host launch included)", "batch": B, "hip_us": 1e3 * ms, "torch_us": 1e3 * t_ms,
                          "floor_us_512MB_at_6.29TBps": 512 * 1.048576 / 6.29, "achieved_weight_gb_per_s": 4 * 4096 * 32768 / (ms * 1e-3) / 1e9})  # fmt: skip

    for spec in args.rows.split(","):
        hw, b = spec.split(":")
        h, w_ = map(int, hw.split("x"))
        B = int(b)
        x = torch.rand(B, 3, h, w_, generator=torch.Generator().manual_seed(h + B)).to(dev)
        flop, vflop = model(h, w_)

        def run_hip():
            return hip.forward_batched(packed, x, whiten)["global_descriptor"]

        def run_torch():
            with torch.no_grad():
                return rr.forward(sd_dev, x, whiten)["global_descriptor"]

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
        rec = {"commit": args.commit, "size": f"{h}x{w_}", "batch": B, "whiten": whiten, "hip_ms": 1e3 * med["hip"], "hip_images_per_s": B / med["hip"],
               "model_trunk_gflop_per_image": flop / 1e9, "model_vlad_mflop_per_image": vflop / 1e6, "model_tflops": flop * B / med["hip"] / 1e12,
               "executed_split_tflops": 3 * flop * B / med["hip"] / 1e12}  # fmt: skip
        if "torch" in med:
            err = (run_hip() - run_torch()).abs().max().item() / run_torch().abs().max().item()
            rec.update(torch_ms=1e3 * med["torch"], torch_fp32_images_per_s=B / med["torch"], speedup=med["torch"] / med["hip"], max_rel_diff_vs_torch=err)
        lines.append(rec)
    for rec in lines:
        line = json.dumps(rec)
        print(line, flush=True)
        if not args.hip_only:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as fd:
                fd.write(line + "\n")


if __name__ == "__main__":
    main()
