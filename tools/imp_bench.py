"""IMP (`sfd2+imp`) timings on one MI355X: the HIP path (split arithmetic, B pairs per `forward_batched` call, no host synchronisation
inside a call) vs the restatement tests/imp_reference.py run by PyTorch-ROCm in fp32 on the same GPU, one pair per call.  Alternated,
after warm-up; the median of `--reps` calls; one JSON line per row, appended to profiles/imp_bench.jsonl.

    python tools/imp_bench.py [--reps 7] [--rows 1024x16,2048x8,4096x2,2048x1] [--commit <base commit>] [--out <file>] [--no-torch]
    python tools/imp_bench.py --trace        one `rocprofv3 --kernel-trace --stats` run of the 2048 x 8 row, in a process of its own

Per row (N x N key-points, B pairs, 20 rounds):
  hip_ms / torch_fp32_ms / speedup   the whole call; the restatement's time is the sum over its B calls
  rounds_ms                          the 20 Sinkhorn rounds alone: the assignment probe at 20 rounds minus the probe at 0 rounds
  rounds_floor_ms                    the bytes the rounds must move (20 x B x N x N x 4: the matrix once per round) at the 6.29 TB/s copy figure
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "image-matching-webui_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

COPY_TBPS = 6.29
ROUNDS = 20


def once_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternate(runs, reps):
    for _, f in runs:
        f()
        f()
    t = {name: [] for name, _ in runs}
    for _ in range(reps):
        for name, f in runs:
            t[name].append(once_ms(f))
    return {k: sorted(v)[len(v) // 2] for k, v in t.items()}


def trace(args):
    """One kernel-trace run of the 2048 x 8 row (HIP path only) in a child process; prints the kernel shares."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--rows", "2048x8", "--reps", "3",
               "--no-torch", "--out", os.path.join(tmp, "ignored.jsonl")]  # fmt: skip
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"rocprofv3 failed ({r.returncode}):\n{r.stderr[-2000:]}")
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        with open(files[0]) as fd:
            rows = list(csv.DictReader(fd))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    shares = sorted(((float(r["TotalDurationNs"]) / total, r["Name"], int(r["Calls"])) for r in rows), reverse=True)[:12]
    rec = {"commit": args.commit, "row": "trace 2048x2048x8", "kernel_shares": [{"kernel": n[:60], "share": round(s, 4), "calls": c} for s, n, c in shares]}
    line = json.dumps(rec)
    print(line)
    with open(args.out, "a") as fd:
        fd.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", default="1024x16,2048x8,4096x2,2048x1")
    ap.add_argument("--commit", default="", help="base commit the lines are stamped with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imp_bench.jsonl"))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if args.trace:
        return trace(args)
    import imp_reference as R
    from imcui_hip import backend
    from imcui_hip.hloc.matchers.imp import IMP
    from imcui_hip.synth_weights import imp_synth_state

    dev = torch.device("cuda:0")
    backend.set_precision(dev, 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    sd = imp_synth_state(0)
    model = IMP({"state_dict": sd, "sinkhorn_iterations": ROUNDS}).eval().to(dev)
    net = R.oracle(sd, ROUNDS, double=False).to(dev)
    probe = backend.IMPHIP()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for row in args.rows.split(","):
        N, B = map(int, row.split("x"))
        ds = [R.problem(500 + b, N, N, N // 4) for b in range(B)]
        cat = lambda k: torch.cat([d[k] for d in ds]).to(dev)
        t = [cat(k) for k in ("keypoints0", "keypoints1", "scores0", "scores1", "descriptors0", "descriptors1")]
        cnt = torch.full((B,), N, dtype=torch.int32, device=dev)
        gpu = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items() if k != "partner"} for d in ds]

        def hip():
            return model.forward_batched(*t, cnt, cnt, (640, 480), (640, 480))

        def torch_fp32():
            return [net.produce_matches(d) for d in gpu]

        runs = (("hip", hip),) if args.no_torch else (("hip", hip), ("torch", torch_fp32))
        med = alternate(runs, args.reps)
        sc = torch.randn(B, N, N, device=dev)
        pr = alternate((("r20", lambda: probe.ot_probe(sc, cnt, cnt, 1.0, ROUNDS)), ("r0", lambda: probe.ot_probe(sc, cnt, cnt, 1.0, 0))), args.reps)
        del sc
        floor = ROUNDS * B * N * N * 4 / (COPY_TBPS * 1e12) * 1e3
        rec = {"commit": args.commit, "row": f"{N}x{N}x{B}", "rounds": ROUNDS, "hip_ms": med["hip"], "rounds_ms": pr["r20"] - pr["r0"], "rounds_floor_ms": floor,
               "rounds_share_of_floor": floor / max(pr["r20"] - pr["r0"], 1e-9)}  # fmt: skip
        if not args.no_torch:
            rec.update({"torch_fp32_ms": med["torch"], "speedup": med["torch"] / med["hip"]})
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as fd:
            fd.write(line + "\n")


if __name__ == "__main__":
    main()
