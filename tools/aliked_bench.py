"""ALIKED extractor throughput on one MI355X: the HIP path (split arithmetic) vs the torch restatement of upstream's ALIKED
(tests/aliked_reference.py: dense 128-channel maps, deformable convolution by explicit gathers) run by PyTorch-ROCm in fp32 on the
same GPU -- what a user of `aliked+lightglue` gets without this backend (upstream itself needs torchvision's deform_conv2d).
Alternated, after warm-up; one JSON line per size, appended to profiles/aliked_bench.jsonl.

    python tools/aliked_bench.py [--reps 5] [--sizes 480x640:16,768x1024:8]

The HBM figures are a MODEL of buffer traffic (floats written + read per padded pixel at each resolution, counted from the launch
list of csrc/aliked.hip; cache hits of overlapping windows are not counted as traffic), not a measurement:
  HIP    1/1: 125, 1/2: 448 / 4, 1/8: 2600 / 64, 1/32: 5300 / 1024 floats per pixel, + 1.4 k floats per key-point (SDDH: the samples stay in LDS; 25 gathered positions x ~50 floats + the descriptor row)
  dense  the same trunk + SDDH as materialised by torch (14.7 k floats per key-point) + f1 (32 w, 32 r), the up-sampled branches (96 w), x1234 (128 w, 128 r by the score head,
         128 r + 128 w by F.normalize) and the padded copy SDDH gathers patches from (128 r, 128 w): 928 floats per pixel more.
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


def hbm_bytes(h, w, npts):
    """(HIP path, dense implementation) modelled bytes per image, see the module docstring."""
    px = (-(-h // 32) * 32) * (-(-w // 32) * 32)
    trunk = px * (125 + 448 / 4 + 2600 / 64 + 5300 / 1024)
    return 4.0 * (trunk + npts * 1.4e3), 4.0 * (trunk + px * 928 + npts * 14.7e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="480x640:16,768x1024:8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aliked_bench.jsonl"))
    args = ap.parse_args()
    from aliked_reference import ALIKEDReference
    from imcui_hip import backend
    from imcui_hip.hloc.extractors.aliked import ALIKED
    from imcui_hip.synth_weights import aliked_state_dict
    from test_aliked_cpu import image

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    sd = aliked_state_dict(0)
    hip = ALIKED({"state_dict": sd}).eval().to(dev)  # the default conf: threshold 0.2, radius 2, no key-point limit
    ref = ALIKEDReference(sd).to(dev)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False

    def run_hip(x):
        return hip.forward_batched(x)["num_keypoints"]

    def run_torch(x):
        with torch.no_grad():
            return ref(x, hip.conf)["scores"]

    for spec in args.sizes.split(","):
        hw, b = spec.split(":")
        h, w = map(int, hw.split("x"))
        B = int(b)
        x = torch.cat([image(h, w, 10 + i) for i in range(B)]).to(dev)
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
        hb, db = hbm_bytes(h, w, nk)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        line = json.dumps({"size": f"{h}x{w}", "batch": B, "mean_keypoints": nk,
                           "hip_images_per_s": B / med["hip"], "torch_fp32_images_per_s": B / med["torch"], "speedup": med["torch"] / med["hip"],
                           "hip_ms": 1e3 * med["hip"], "torch_ms": 1e3 * med["torch"],
                           "modelled_hbm_mb_per_image": hb / 1e6, "modelled_dense_hbm_mb_per_image": db / 1e6})  # fmt: skip
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fd:
            fd.write(line + "\n")


if __name__ == "__main__":
    main()
