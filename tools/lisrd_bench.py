"""LISRD timings on one MI355X: the HIP path (split arithmetic, no host synchronisation inside a call) vs the torch restatement
(tests/lisrd_reference.py and the wrapper's formulas restated there) run by PyTorch-ROCm in fp32 on the same GPU.  Alternated, after
warm-up; the median of `--reps` calls; one JSON line per row, appended to profiles/lisrd_bench.jsonl.

    python tools/lisrd_bench.py [--reps 7] [--size 480x640] [--keypoints 2048] [--commit <base commit>] [--out <file>]

Rows:
  describe   one image of --size with --keypoints key-points: `LisrdHIP.describe` against the restated network + `extract_descriptors`
  match      --keypoints x --keypoints key-points (random unit vectors, Dm = 1024): `backend.lisrd_match` against the MATERIALISED einsum
             form of `_lisrd_matcher` + `_compute_confidence` (two [N, 4, M] tensors).  Modelled work: 2 N M 4 (128 + 1024) FLOP.
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
import torch.nn.functional as F  # noqa: E402


def once_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternate(runs, reps):
    for _, f in runs:  # warm-up (MIOpen / hipBLASLt pick their kernels here)
        f()
        f()
    t = {name: [] for name, _ in runs}
    for _ in range(reps):
        for name, f in runs:
            t[name].append(once_ms(f))
    return {k: sorted(v)[len(v) // 2] for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", default="480x640")
    ap.add_argument("--keypoints", type=int, default=2048)
    ap.add_argument("--commit", default="", help="base commit the lines are stamped with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lisrd_bench.jsonl"))
    args = ap.parse_args()
    import lisrd_reference as R
    from imcui_hip import backend
    from imcui_hip.synth_weights import lisrd_synth_state

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    h, w = map(int, args.size.split("x"))
    K = args.keypoints
    g = torch.Generator().manual_seed(0)
    recs = []

    # ---- describe
    sd = lisrd_synth_state(0)
    packed = backend.pack_lisrd(sd).to(dev)
    impl = backend.LisrdHIP()
    net = R.LisrdNet().eval().to(dev)
    net.load_state_dict(sd)
    img = torch.rand(1, 3, h, w, generator=g).to(dev)
    kp = (torch.rand(1, K, 2, generator=g) * torch.tensor([w - 1.0, h - 1.0])).to(dev)
    cnt = torch.tensor([K], dtype=torch.int32, device=dev)

    def hip_describe():
        return impl.describe(packed, img, kp, cnt)

    def torch_describe():
        with torch.no_grad():
            out = net(img * 255.0)
            kpr = kp[0][:, [1, 0]]
            grid = (kpr * 2.0 / torch.tensor((h, w), dtype=torch.float32, device=dev) - 1.0)[..., [1, 0]].view(-1, K, 1, 2)
            pick = lambda maps: torch.stack([F.normalize(F.grid_sample(maps[v], grid, align_corners=False), dim=1)[0, :, :, 0].t() for v in R.VARIANCES], dim=1)
            return pick(out["descriptors"]), pick(out["meta_descriptors"])

    med = alternate((("hip", hip_describe), ("torch", torch_describe)), args.reps)
    recs.append({"commit": args.commit, "row": "describe", "size": f"{h}x{w}", "keypoints": K, "hip_ms": med["hip"], "torch_fp32_ms": med["torch"],
                 "speedup": med["torch"] / med["hip"]})  # fmt: skip

    # ---- match
    unit = lambda *s: F.normalize(torch.randn(*s, generator=g), dim=-1).to(dev)
    d0, m0, d1, m1 = unit(1, K, 4, 128), unit(1, K, 4, 1024), unit(1, K, 4, 128), unit(1, K, 4, 1024)

    def hip_match():
        return backend.lisrd_match(d0, m0, d1, m1)

    def torch_match():  # `_lisrd_matcher` and `_compute_confidence` as upstream writes them: both [N, 4, M] tensors exist
        a, b, c, e = d0[0], d1[0], m0[0], m1[0]
        wts = F.softmax(torch.einsum("nid,mid->nim", c, e), dim=1)
        sims = torch.sum(torch.einsum("nid,mid->nim", a, b) * wts, dim=1)
        nn12, nn21 = torch.max(sims, dim=1)[1], torch.max(sims, dim=0)[1]
        ids = torch.arange(K, device=dev)
        mask = ids == nn21[nn12]
        i0, i1 = ids[mask], nn12[mask]
        nz = lambda t: F.normalize(t, dim=2)
        return torch.sum(torch.sum(nz(a[i0]) * nz(b[i1]), dim=2) * F.softmax(torch.sum(nz(c[i0]) * nz(e[i1]), dim=2), dim=1), dim=1)

    med = alternate((("hip", hip_match), ("torch", torch_match)), args.reps)
    flop = 2.0 * K * K * 4 * (128 + 1024)
    recs.append({"commit": args.commit, "row": "match", "keypoints": f"{K}x{K}", "meta_width": 1024, "hip_ms": med["hip"], "torch_fp32_ms": med["torch"],
                 "speedup": med["torch"] / med["hip"], "modelled_gflop": flop / 1e9, "hip_modelled_tflops": flop / med["hip"] / 1e9})  # fmt: skip
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fd:
        for rec in recs:
            line = json.dumps(rec)
            print(line, flush=True)
            fd.write(line + "\n")


if __name__ == "__main__":
    main()
