"""XFeat extractor throughput on one MI355X: the HIP path (split arithmetic, one batched `forward_batched` call, no host
synchronisation) vs the torch restatement of upstream's XFeat.detectAndCompute (tests/xfeat_reference.py) run by PyTorch-ROCm in fp32
on the same GPU, one image per call with its synchronising `nonzero`, as imcui/hloc/extractors/xfeat.py runs it -- what a user of the
`xfeat(sparse)` zoo entry gets without this backend.  Alternated, after warm-up; the median of `--reps` calls; one JSON line per row,
appended to profiles/xfeat_bench.jsonl.

    python tools/xfeat_bench.py [--reps 7] [--sizes 480x640:16,480x640:1,1200x1600:4] [--commit <base commit>]

The HBM figure is a MODEL of compulsory buffer traffic (floats written + read per pixel of the resized image, counted from the launch
list of csrc/xfeat.hip; re-reads of overlapping convolution windows are taken as cache hits), not a measurement:
  input 5 (3 channels read, gray written, read again by the statistics), stem 19 (1 + 4 | 4 + 2 | 2 + 2 | 2 + 1 + 2),
  1/4 maps stored as 32 channels 9 (block2: 2 + 2 twice, block3.0: 2 + 1), 1/8 maps of 64 channels 1 each way: block3 4, block4 2.25,
  block5 1.1875, fuse 2.3125, block_fusion 6, reliability head 4 + head epilogue 3, unfold 2, key-point head 6 + 2.02, soft-max 2.02,
  NMS 2 (two passes over K1h) = 72 floats = 288 bytes per pixel, + 0.3 kB per key-point (16 taps x 64 channels are cache hits of M1;
  the row written, the list entries).
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

LAUNCHES_PER_CALL = 39  # 18 kernels of csrc/xfeat.hip + 21 GEMM launches, whatever the batch (plus two 4-byte memsets)
FLOATS_PER_PIXEL = 72.0


def hbm_bytes(h, w, npts):
    """Modelled compulsory bytes per image, see the module docstring."""
    px = (h // 32 * 32) * (w // 32 * 32)
    return 4.0 * px * FLOATS_PER_PIXEL + 300.0 * npts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="480x640:16,480x640:1,1200x1600:4")
    ap.add_argument("--max-keypoints", type=int, default=5000)
    ap.add_argument("--commit", default="", help="base commit the lines are stamped with")
    ap.add_argument("--hip-only", action="store_true", help="time the HIP path alone (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xfeat_bench.jsonl"))
    args = ap.parse_args()
    import xfeat_reference as xr
    from imcui_hip import backend
    from imcui_hip.hloc.extractors.xfeat import XFeat
    from imcui_hip.synth_weights import xfeat_state_dict
    from test_xfeat_cpu import _image

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    sd = xfeat_state_dict(0)
    hip = XFeat({"max_keypoints": args.max_keypoints, "state_dict": sd}).eval().to(dev)  # the `xfeat` extractor conf: max_keypoints 5000
    ref = xr.load_model(sd).to(dev)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False

    def run_hip(x):
        return hip.forward_batched(x)["num_keypoints"]

    def run_torch(x):
        return [o["scores"] for o in xr.detect_and_compute(ref, x, top_k=args.max_keypoints)]

    for spec in args.sizes.split(","):
        hw, b = spec.split(":")
        h, w = map(int, hw.split("x"))
        B = int(b)
        x = torch.cat([_image(h, w, 10 + i) for i in range(B)]).to(dev)
        runs = (("hip", run_hip),) if args.hip_only else (("hip", run_hip), ("torch", run_torch))
        for _, f in runs:  # warm-up (MIOpen picks its kernels here)
            f(x)
            f(x)
        torch.cuda.synchronize()
        t = {name: [] for name, _ in runs}
        for _ in range(args.reps):
            for name, f in runs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f(x)
                torch.cuda.synchronize()
                t[name].append(time.perf_counter() - t0)
        nk = float(run_hip(x).float().mean())
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        hb = hbm_bytes(h, w, nk)
        rec = {"commit": args.commit, "size": f"{h}x{w}", "batch": B, "max_keypoints": args.max_keypoints, "mean_keypoints": nk,
               "hip_ms": 1e3 * med["hip"], "hip_images_per_s": B / med["hip"], "launches_per_call": LAUNCHES_PER_CALL,
               "modelled_hbm_mb_per_image": hb / 1e6, "achieved_modelled_gb_per_s": hb * B / med["hip"] / 1e9}  # fmt: skip
        if "torch" in med:
            rec.update(torch_ms=1e3 * med["torch"], torch_fp32_images_per_s=B / med["torch"], speedup=med["torch"] / med["hip"])
        line = json.dumps(rec)
        print(line, flush=True)
        if not args.hip_only:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as fd:
                fd.write(line + "\n")


if __name__ == "__main__":
    main()
