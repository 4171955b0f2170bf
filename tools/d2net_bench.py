"""D2-Net extractor throughput on one MI355X: the HIP path (split arithmetic, one batched `forward_batched` call over all levels, no host
synchronisation) vs the torch restatement (tests/d2net_reference.py) run by PyTorch-ROCm in fp32 on the same GPU (MIOpen convolutions),
one image per call with its synchronising `nonzero` per level, as imcui/hloc/extractors/d2net.py runs it -- what a user of the `d2net` /
`rord` zoo entries gets without this backend.  Alternated, after warm-up; the median of `--reps` calls; one JSON line per row, appended
to profiles/d2net_bench.jsonl.

    python tools/d2net_bench.py [--reps 7] [--rows 480x640:8:ss,480x640:1:ss,1200x1600:1:ss,480x640:1:ms] [--commit <base commit>] [--hip-only]

Two MODELS, not measurements, go with every row (counted from the launch list of csrc/d2net.hip):
  arithmetic  2 x 9 x cin x cout per output pixel of each convolution at its resolution (335 GFLOP for 480 x 640, two thirds of it in
              the two 512 -> 512 dilated layers and conv4_1); the split arithmetic executes three f16 products per element pair of
              layers 1-9
  traffic     every layer output written once and read once (the un-pooled maps of odd sizes too), the 512-channel map read again by
              the detector; re-reads of the patch staging and of the implicit GEMM's taps are taken as cache hits.
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

# (cin, cout, resolution divisor of the layer's OUTPUT before its pool, pooled afterwards)
LAYERS = ((3, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 2), (128, 256, 4), (256, 256, 4), (256, 256, 4))
TAIL = ((256, 512), (512, 512), (512, 512))  # on the (h / 4 - 1) x (w / 4 - 1) map


def model(levels):
    """(FLOP, floats moved) per image for the level images [(h, w)]."""
    flop = floats = 0.0
    for h, w in levels:
        floats += 3 * h * w
        for cin, cout, d in LAYERS:
            px = (h // d) * (w // d)
            flop += 2.0 * 9 * cin * cout * px
            floats += 2.0 * cout * px
        fp = (h // 4 - 1) * (w // 4 - 1)
        floats += 2.0 * 256 * fp
        for cin, cout in TAIL:
            flop += 2.0 * 9 * cin * cout * fp
            floats += 2.0 * cout * fp
        floats += 512.0 * fp  # the detector's pass
    return flop, floats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="480x640:8:ss,480x640:1:ss,1200x1600:1:ss,480x640:1:ms")
    ap.add_argument("--max-keypoints", type=int, default=5000)
    ap.add_argument("--commit", default="", help="base commit the lines are stamped with")
    ap.add_argument("--hip-only", action="store_true", help="time the HIP path alone (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "d2net_bench.jsonl"))
    args = ap.parse_args()
    import d2net_reference as rr
    from imcui_hip import backend
    from imcui_hip.hloc.extractors.d2net import D2Net
    from imcui_hip.synth_weights import d2net_state_dict
    from test_d2net_cpu import image

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    sd = d2net_state_dict(0)
    hip = D2Net({"max_keypoints": args.max_keypoints, "state_dict": sd}).eval().to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}

    for spec in args.rows.split(","):
        hw, b, mode = spec.split(":")
        h, w = map(int, hw.split("x"))
        B, ms = int(b), mode == "ms"
        conf = {"multiscale": ms, "use_relu": True, "max_keypoints": args.max_keypoints}
        hip.conf.update(conf)
        x = torch.cat([image(h, w, 10 + i) for i in range(B)]).to(dev)
        levels = backend.d2net_levels(h, w, backend.D2NET_SCALES_MS if ms else backend.D2NET_SCALES_SS)
        flop, floats = model(levels)

        def run_hip(x):
            return hip.forward_batched(x)["num_keypoints"]

        def run_torch(x):
            with torch.no_grad():
                return [rr.extract(sd_dev, x[i : i + 1], conf)["scores"] for i in range(x.shape[0])]  # one image per call, as the wrapper does

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
        rec = {"commit": args.commit, "size": f"{h}x{w}", "batch": B, "multiscale": ms, "levels": levels, "max_keypoints": args.max_keypoints,
               "mean_keypoints": nk, "status": status, "hip_ms": 1e3 * med["hip"], "hip_images_per_s": B / med["hip"],
               "model_gflop_per_image": flop / 1e9, "model_tflops": flop * B / med["hip"] / 1e12, "executed_split_tflops": 3 * flop * B / med["hip"] / 1e12,
               "modelled_hbm_mb_per_image": 4 * floats / 1e6, "achieved_modelled_gb_per_s": 4 * floats * B / med["hip"] / 1e9}  # fmt: skip
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
