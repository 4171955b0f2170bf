"""ALIKE extractor throughput on one MI355X: the HIP path (split arithmetic, one batched `forward_batched` call, no host
synchronisation) vs the torch restatement of upstream's ALIKE (tests/alike_reference.py) run by PyTorch-ROCm in fp32 on the same GPU,
one image per call with its synchronising `nonzero`, as imcui/hloc/extractors/alike.py runs it -- what a user of the `alike` zoo entry
gets without this backend.  Alternated, after warm-up; the median of `--reps` calls; one JSON line per row, appended to
profiles/alike_bench.jsonl.

    python tools/alike_bench.py [--reps 7] [--models alike-t,alike-n] [--sizes 480x640:16,480x640:1,1200x1600:4] [--commit <base commit>]

The HBM figure is a MODEL of compulsory buffer traffic (floats written + read per padded pixel, counted from the launch list of
csrc/alike.hip; re-reads of overlapping convolution windows and of the weights are taken as cache hits), not a measurement:
  image 3, block 1: c1 written + read by its second layer, x1 written (3 c1), read by the pool, the score kernel and (sparsely) the
  descriptors (2 c1); 1/2 maps: pooled input 32, t2 / x2 / shortcut P2 each written and read (8 P2 + 64) / 4; 1/8 and 1/32 maps
  likewise / 64 and / 1024; score written, read by the NMS, the mean, the sample (4), NMS planes 4, candidate lists 2
  -> alike-t: 3 + 5 x 8 + (8 x 32 + 64 + 2 x 17) / 4 + ~6 + 10 = 147 floats; alike-n: 3 + 5 x 16 + 88.5 + ~12 + 10 = 194 floats
  per padded pixel, + (dim + 3) x 4 bytes per key-point written and ~2 kB gathered (cache hits of x1 / f2..f4 for most).
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

FLOATS_PER_PIXEL = {"alike-t": 147.0, "alike-s": 160.0, "alike-n": 194.0}


def hbm_bytes(model, h, w, npts, dim):
    """Modelled compulsory bytes per image, see the module docstring."""
    px = ((h + 31) // 32 * 32) * ((w + 31) // 32 * 32)
    return 4.0 * px * FLOATS_PER_PIXEL[model] + 4.0 * (dim + 3) * npts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--models", default="alike-t,alike-n")
    ap.add_argument("--sizes", default="480x640:16,480x640:1,1200x1600:4")
    ap.add_argument("--max-keypoints", type=int, default=5000)
    ap.add_argument("--commit", default="", help="base commit the lines are stamped with")
    ap.add_argument("--hip-only", action="store_true", help="time the HIP path alone (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alike_bench.jsonl"))
    args = ap.parse_args()
    import alike_reference as ar
    from imcui_hip import backend
    from imcui_hip.hloc.extractors.alike import Alike
    from imcui_hip.synth_weights import alike_state_dict
    from test_aliked_cpu import image

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    conf = dict(max_keypoints=args.max_keypoints, detection_threshold=0.5, top_k=-1, sub_pixel=False)  # the `alike` extractor conf
    for model in args.models.split(","):
        sd = alike_state_dict(model, 0)
        hip = Alike({**conf, "model_name": model, "state_dict": sd}).eval().to(dev)
        ref = ar.ALIKEReference(sd, model).to(dev)

        def run_hip(x):
            return hip.forward_batched(x)["num_keypoints"]

        def run_torch(x):
            with torch.no_grad():
                return [ref.forward(x[b : b + 1], conf)["scores"][0] for b in range(x.shape[0])]  # one image per call, as the wrapper does

        for spec in args.sizes.split(","):
            hw, b = spec.split(":")
            h, w = map(int, hw.split("x"))
            B = int(b)
            x = torch.cat([image(h, w, 10 + i) for i in range(B)]).to(dev)
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
            hb = hbm_bytes(model, h, w, nk, hip._impl.dims[4])
            rec = {"commit": args.commit, "model": model, "size": f"{h}x{w}", "batch": B, "max_keypoints": args.max_keypoints, "mean_keypoints": nk,
                   "hip_ms": 1e3 * med["hip"], "hip_images_per_s": B / med["hip"],
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
