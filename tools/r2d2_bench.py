"""R2D2 extractor throughput on one MI355X: the HIP path (split arithmetic, one batched `forward_batched` call over the whole pyramid, no
host synchronisation) vs the torch restatement (tests/r2d2_reference.py) run by PyTorch-ROCm in fp32 on the same GPU, one image per call
with its synchronising `nonzero` per level, as imcui/hloc/extractors/r2d2.py runs it -- what a user of the `r2d2` zoo entry gets without
this backend.  Default conf, alternated, after warm-up; the median of `--reps` calls; one JSON line per row, appended to
profiles/r2d2_bench.jsonl.

    python tools/r2d2_bench.py [--reps 7] [--sizes 480x640:8,480x640:1,768x1024:2] [--commit <base commit>] [--hip-only]

Two MODELS, not measurements, go with every row (counted from the launch list of csrc/r2d2.hip, per pixel of every level that runs):
  arithmetic  2 x (27 x 32 + 288 x 32 + 288 x 64 + 576 x 64 + 576 x 128 + 1152 x 128 + 3 x 512 x 128) = 0.966 MFLOP; the split
              arithmetic executes three f16 products per element pair of layers 1-8 (2.89 MFLOP executed)
  traffic     every buffer written once and read once: level 3, layer outputs 32 + 32 + 64 + 64 + 5 x 128 = 832 floats written and read,
              the two head maps written and read by the detector: 3 + 2 x 832 + 2 x 2 + 2 = 1673 floats = 6.7 kB.  The implicit GEMM
              re-fetches its input once per tap (4 or 9 times); those re-reads are taken as cache hits here.
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

FLOP_PER_PIXEL = 2.0 * (27 * 32 + 288 * 32 + 288 * 64 + 576 * 64 + 576 * 128 + 1152 * 128 + 3 * 512 * 128)
FLOATS_PER_PIXEL = 1673.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="480x640:8,480x640:1,768x1024:2")
    ap.add_argument("--max-keypoints", type=int, default=5000)
    ap.add_argument("--commit", default="", help="base commit the lines are stamped with")
    ap.add_argument("--hip-only", action="store_true", help="time the HIP path alone (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r2d2_bench.jsonl"))
    args = ap.parse_args()
    import r2d2_reference as rr
    from imcui_hip import backend
    from imcui_hip.hloc.extractors.r2d2 import R2D2
    from imcui_hip.synth_weights import r2d2_state_dict
    from test_r2d2_cpu import image

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    sd = r2d2_state_dict(0)
    conf = {**rr.DEFAULT_CONF, "max_keypoints": args.max_keypoints}  # the extractor's default conf
    hip = R2D2({**conf, "state_dict": sd}).eval().to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}

    def run_hip(x):
        return hip.forward_batched(x)["num_keypoints"]

    def run_torch(x):
        with torch.no_grad():
            return [rr.extract(sd_dev, x[b : b + 1], conf)["scores"] for b in range(x.shape[0])]  # one image per call, as the wrapper does

    for spec in args.sizes.split(","):
        hw, b = spec.split(":")
        h, w = map(int, hw.split("x"))
        B = int(b)
        x = torch.cat([image(h, w, 10 + i) for i in range(B)]).to(dev)
        levels = [l for l in backend.r2d2_levels(h, w) if l[2]]
        npix = sum(l[0] * l[1] for l in levels)
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
        out = hip.forward_batched(x)
        nk, status = float(out["num_keypoints"].float().mean()), int(out["status"][0])
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        rec = {"commit": args.commit, "size": f"{h}x{w}", "batch": B, "levels": len(levels), "pixels_per_image": npix, "max_keypoints": args.max_keypoints,
               "mean_keypoints": nk, "status": status, "hip_ms": 1e3 * med["hip"], "hip_images_per_s": B / med["hip"],
               "model_tflop_per_image": FLOP_PER_PIXEL * npix / 1e12, "model_tflops": FLOP_PER_PIXEL * npix * B / med["hip"] / 1e12,
               "executed_split_tflops": 3 * FLOP_PER_PIXEL * npix * B / med["hip"] / 1e12,
               "modelled_hbm_mb_per_image": 4 * FLOATS_PER_PIXEL * npix / 1e6, "achieved_modelled_gb_per_s": 4 * FLOATS_PER_PIXEL * npix * B / med["hip"] / 1e9}  # fmt: skip
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
