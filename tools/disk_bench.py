"""DISK extractor throughput on one MI355X: the HIP path (split arithmetic) vs the torch restatement of kornia's DISK
(tests/disk_reference.py) run by PyTorch-ROCm in fp32 on the same GPU -- what a user of the `disk` zoo entries gets without this
backend.  Alternated, after warm-up, one JSON line per size.  Also prints the executed vs dense-equivalent FLOPs per image.

    python tools/disk_bench.py [--reps 5] [--sizes 480x640:16,1200x1600:4]
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

# (cin, cout, level) of the 5x5 convolutions; level l = 1/2^l resolution
LAYERS = [(3, 16, 0), (16, 32, 1), (32, 64, 2), (64, 64, 3), (64, 64, 4), (128, 64, 3), (128, 64, 2), (96, 64, 1), (80, 129, 0)]


def flops(h, w, npts):
    """(executed, dense-equivalent) FLOPs per image: 2 x MACs of the convolutions.  Dense = the network as defined.  Executed = what
    the HIP path multiplies: the dense layers except the last one with their input channels as stored (16 -> 32 zero-padded on down 1,
    the GEMM's K = 25 x 32), the heatmap row of the last layer on 80 channels, and its 128 descriptor rows at `npts` key-points with
    K = 25 x 96 (80 padded to 96).  Column tiles are not counted: a 32- or 64-channel layer runs on 128-column MFMA tiles."""
    hp, wp = -(-h // 16) * 16, -(-w // 16) * 16
    pad = {16: 32, 80: 96}
    dense = sum(2 * 25 * ci * co * (hp >> l) * (wp >> l) for ci, co, l in LAYERS)
    executed = sum(2 * 25 * pad.get(ci, ci) * co * (hp >> l) * (wp >> l) for ci, co, l in LAYERS[:-1] if ci != 3)
    executed += 2 * 25 * 3 * 16 * hp * wp + 2 * 25 * 80 * hp * wp + 2 * 25 * 96 * 128 * npts
    return executed, dense


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="480x640:16,1200x1600:4")
    ap.add_argument("--n", type=int, default=5000)
    args = ap.parse_args()
    from disk_reference import DISKReference
    from imcui_hip import backend
    from imcui_hip.hloc.extractors.disk import DISK
    from imcui_hip.synth_weights import disk_state_dict

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    sd = disk_state_dict(0)
    conf = {"max_keypoints": args.n, "nms_window_size": 5, "detection_threshold": 0.0, "pad_if_not_divisible": True}
    hip = DISK({**conf, "state_dict": sd}).eval().to(dev)
    ref = DISKReference(sd).to(dev)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False

    def run_hip(x):
        out = hip.forward_batched(x)
        return out["num_keypoints"]

    def run_torch(x):
        with torch.no_grad():
            feats = ref(x, n=args.n, window_size=5, score_threshold=0.0, pad_if_not_divisible=True)
        return feats[-1]["scores"]

    for spec in args.sizes.split(","):
        hw, b = spec.split(":")
        h, w = map(int, hw.split("x"))
        B = int(b)
        x = torch.rand(B, 3, h, w, device=dev)
        for f in (run_hip, run_torch):  # warm-up (MIOpen picks its kernels here)
            f(x)
            f(x)
        torch.cuda.synchronize()
        t = {"hip": [], "torch": []}
        for _ in range(args.reps):
            for name, f in (("hip", run_hip), ("torch", run_torch)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f(x)
                torch.cuda.synchronize()
                t[name].append(time.perf_counter() - t0)
        nk = float(hip.forward_batched(x)["num_keypoints"].float().mean())
        ex, de = flops(h, w, nk)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        print(json.dumps({"size": f"{h}x{w}", "batch": B, "n": args.n, "mean_keypoints": nk,
                          "hip_images_per_s": B / med["hip"], "torch_fp32_images_per_s": B / med["torch"], "speedup": med["torch"] / med["hip"],
                          "hip_ms": 1e3 * med["hip"], "torch_ms": 1e3 * med["torch"],
                          "executed_gflop_per_image": ex / 1e9, "dense_gflop_per_image": de / 1e9}), flush=True)  # fmt: skip


if __name__ == "__main__":
    main()
