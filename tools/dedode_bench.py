"""DeDoDe extractor throughput on one MI355X: the HIP path (split arithmetic, one batched `forward_batched` call, no host
synchronisation) vs the torch restatement (tests/dedode_reference.py, upstream's library form of the detection arithmetic) run by
PyTorch-ROCm in fp32 on the same GPU (MIOpen convolutions), one image per call, as imcui/hloc/extractors/dedode.py runs it -- what a user
of the `dedode` zoo entry gets without this backend.  Alternated, after warm-up; the median of `--reps` calls; one JSON line per row,
appended to profiles/dedode_bench.jsonl.

    python tools/dedode_bench.py [--reps 7] [--rows 768x768:4,768x768:1,480x640:8] [--commit <base commit>] [--hip-only]

One MODEL, not a measurement, goes with every row: 2 x taps x cin x cout per output pixel of each layer at its resolution, read from the
packed widths (encoders, the refiners' 1x1 layers, the depth-wise 5x5 layers; the descriptor's last out_conv counted at the key-points).
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


def model_flop(backend, dims, h, w, k):
    """FLOP per image: (encoders, refiner 1x1 layers, depth-wise layers)."""
    enc = pw = dw = 0.0
    for m, name in enumerate(backend.DEDODE_MODELS):
        px, cin = h * w, 3
        for v in backend.DEDODE_ENCODERS[name]:
            if v == "M":
                px //= 4
            else:
                enc += 2.0 * 9 * cin * v * px
                cin = v
        for i, s in enumerate(backend.DEDODE_SCALES):
            rin, hid, out, n = dims[(m * 4 + i) * 4 : (m * 4 + i) * 4 + 4]
            px = (h // s) * (w // s)
            pw += 2.0 * px * (rin * hid + hid * hid + n * hid * hid)
            dw += 2.0 * px * n * 25 * hid
            pw += 2.0 * hid * ((1 if m == 0 else 256) * (px if m == 0 else k) if s == 1 else out * px)
    return enc, pw, dw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="768x768:4,768x768:1,480x640:8")
    ap.add_argument("--max-keypoints", type=int, default=5000)
    ap.add_argument("--commit", default="", help="base commit the lines are stamped with")
    ap.add_argument("--hip-only", action="store_true", help="time the HIP path alone (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedode_bench.jsonl"))
    args = ap.parse_args()
    import dedode_reference as rr
    from imcui_hip import backend
    from imcui_hip.hloc.extractors.dedode import DeDoDe
    from imcui_hip.synth_weights import dedode_state_dicts
    from test_dedode_cpu import image

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    det, desc = dedode_state_dicts(0)
    hip = DeDoDe({"max_keypoints": args.max_keypoints, "state_dict_detector": det, "state_dict_descriptor": desc}).eval().to(dev)
    det_dev, desc_dev = ({k: v.to(dev) for k, v in sd.items()} for sd in (det, desc))
    conf = {"max_keypoints": args.max_keypoints}

    for spec in args.rows.split(","):
        hw, b = spec.split(":")
        h, w = map(int, hw.split("x"))
        B = int(b)
        x = torch.cat([image(h, w, 10 + i) for i in range(B)]).to(dev)
        enc, pw, dw = model_flop(backend, hip.dims, h, w, args.max_keypoints)

        def run_hip(x):
            return hip.forward_batched(x)["num_keypoints"]

        def run_torch(x):
            with torch.no_grad():
                return [rr.extract(det_dev, desc_dev, x[i : i + 1], conf, form=rr.scores_library)["scores"] for i in range(x.shape[0])]

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
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        flop = enc + pw + dw
        rec = {"commit": args.commit, "size": f"{h}x{w}", "batch": B, "max_keypoints": args.max_keypoints, "hip_ms": 1e3 * med["hip"],
               "hip_images_per_s": B / med["hip"], "model_gflop_per_image": flop / 1e9, "model_gflop_encoders": enc / 1e9, "model_gflop_1x1": pw / 1e9,
               "model_gflop_depthwise": dw / 1e9, "model_tflops": flop * B / med["hip"] / 1e12}  # fmt: skip
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
