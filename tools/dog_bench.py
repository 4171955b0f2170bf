"""DoG + HardNet / SOSNet throughput on one MI355X: the HIP descriptor stage (imcui_hip_patchdesc_forward: pyramid, LAF patches, the
7-layer network, output normalisation; split arithmetic, one batched call, no host synchronisation) vs the same stage of the torch
restatement (tests/dog_reference.py) run by PyTorch-ROCm in fp32 on the same GPU on the SAME key-points (MIOpen convolutions,
grid_sample), which is what imcui/hloc/extractors/dog.py:87-105 runs.  Key-points come from the HIP detector (csrc/sift.hip) with the
confs' `max_keypoints: 5000`; detection is timed next to it.  Alternated, after warm-up; the median of `--reps` calls; one JSON line per
row, appended to profiles/dog_bench.jsonl.  The last layer ([n, 8192] x [8192, 128] as 8 K groups in one batched launch, then the fold) is timed
alone at n = 1024 next to its byte floor: the activations (32 MiB), the weight matrix (4 MiB), the partial products written and read
back (2 x 4 MiB) at the 6.29 TB/s this project measured for a copy kernel.

    python tools/dog_bench.py [--reps 7] [--rows 480x640:1,480x640:8,768x1024:2] [--confs hardnet,sosnet] [--commit <base commit>] [--hip-only]

One MODEL, not a measurement, goes with every row: 2 x K x cout per output pixel of each convolution, 38.9 M multiply-adds per patch
(the split arithmetic executes three f16 products per element pair of layers 2-7)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "image-matching-webui_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# (cin, cout, kernel, output pixels) of the seven layers
LAYERS = ((1, 32, 3, 1024), (32, 32, 3, 1024), (32, 64, 3, 256), (64, 64, 3, 256), (64, 128, 3, 64), (128, 128, 3, 64), (128, 128, 8, 1))
FLOP_PER_PATCH = sum(2.0 * k * k * cin * cout * px for cin, cout, k, px in LAYERS)
FINAL_FLOOR_BYTES = 1024 * 8192 * 4 + 2 * 128 * 8192 * 2 + 8 * 2 * 1024 * 128 * 4


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
    ap.add_argument("--rows", default="480x640:1,480x640:8,768x1024:2")
    ap.add_argument("--confs", default="hardnet,sosnet")
    ap.add_argument("--commit", default="", help="base commit the lines are stamped with")
    ap.add_argument("--hip-only", action="store_true", help="time the HIP path alone (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dog_bench.jsonl"))
    args = ap.parse_args()
    import dog_reference as rr
    import sift_reference as sr
    from imcui_hip import backend
    from imcui_hip.hloc import extract_features as ef
    from imcui_hip.hloc.extractors.dog import DoG
    from imcui_hip.synth_weights import hardnet_synth_state, sosnet_synth_state

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    lines = []
    hip = backend.PatchDescHIP()

    for name in args.confs.split(","):
        sd = (hardnet_synth_state if name == "hardnet" else sosnet_synth_state)(0)
        model = DoG({**ef.confs[name]["model"], "state_dict": sd}).eval().to(dev)
        net = rr.build(name, sd).to(dev)

        # the last layer alone: 1024 rows, the forward's own launches
        x = torch.relu(torch.randn(1024, 8, 8, 128, device=dev))
        hip.layer_probe("final", x, name, model.packed)
        ms = median_ms(lambda: hip.layer_probe("final", x, name, model.packed), args.reps)
        lines.append({"commit": args.commit, "conf": name, "row": "layer 7 alone (probe: the batched K-group launch + fold, host launches included)", "rows": 1024, "hip_us": 1e3 * ms,
                      "floor_us_at_6.29TBps": FINAL_FLOOR_BYTES / 6.29e12 * 1e6, "model_gflop": 2.0 * 1024 * 8192 * 128 / 1e9,
                      "executed_split_tflops": 3 * 2.0 * 1024 * 8192 * 128 / (ms * 1e-3) / 1e12})  # fmt: skip

        for spec in args.rows.split(","):
            hw, b = spec.split(":")
            h, w = map(int, hw.split("x"))
            B = int(b)
            img = torch.from_numpy(np.stack([sr.seeded_image(h, w, seed=s) for s in range(B)]))[:, None].to(dev)
            det = model._sift.forward(img, model.sift_conf)
            counts = det["num_keypoints"].tolist()
            kp, sc, od, cnt = det["keypoints"], det["scales"] * 0.5, torch.rad2deg(det["oris"]), det["num_keypoints"]

            def run_detect():
                return model._sift.forward(img, model.sift_conf)

            def run_hip():
                return hip.forward(model.packed, img, kp, sc, od, cnt, name, mr_size=12.0)["descriptors"]

            def run_torch():
                with torch.no_grad():
                    return [rr.forward(name, None, img[i], kp[i, :n], sc[i, :n], od[i, :n], net=net) for i, n in enumerate(counts)]

            runs = (("detect", run_detect), ("hip", run_hip)) if args.hip_only else (("detect", run_detect), ("hip", run_hip), ("torch", run_torch))
            for _, f in runs:  # warm-up (MIOpen picks its kernels here)
                f()
                f()
            torch.cuda.synchronize()
            t = {k: [] for k, _ in runs}
            for _ in range(args.reps):
                for k, f in runs:
                    t[k].append(median_ms(f, 1))
            med = {k: sorted(v)[len(v) // 2] * 1e-3 for k, v in t.items()}
            npatch = sum(counts)
            rec = {"commit": args.commit, "conf": name, "size": f"{h}x{w}", "batch": B, "keypoints": counts, "detect_ms": 1e3 * med["detect"], "hip_desc_ms": 1e3 * med["hip"],
                   "hip_patches_per_s": npatch / med["hip"], "model_gflop_per_patch": FLOP_PER_PATCH / 1e9, "model_tflops": FLOP_PER_PATCH * npatch / med["hip"] / 1e12,
                   "executed_split_tflops": 3 * FLOP_PER_PATCH * npatch / med["hip"] / 1e12}  # fmt: skip
            if "torch" in med:
                a, b_ = run_hip(), run_torch()
                err = max((a[i, :n] - b_[i]).abs().max().item() for i, n in enumerate(counts) if n)
                rec.update(torch_desc_ms=1e3 * med["torch"], speedup=med["torch"] / med["hip"], max_abs_diff_vs_torch=err)
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
