"""What Bob-side reconciliation costs: on the golden N = 10240 code at QBER 0.02
with 4096 frames (keys from keygen, syndromes from calculate_syndrome), three
calls timed warm with HIP events, alternating, REPS times each:

  (a) reconcile(H, bob, syndrome, q)               the received-syndrome entry
  (b) qkd_ldpc(H, alice, bob, q, want_bits=True)   both keys (the reference's harness)
  (c) sum_product_decoding(H, llr, syndrome)       +-log_p LLRs: what a caller holding
                                                   only a syndrome had to do before

Writes profiles/reconcile_bench.json: per call the median and the min-max spread
of its reps, and the ratios (a)/(b) and (c)/(a). --headline adds the step times
of plain bench.py runs of this build and of the parent's (JSON result lines
collected by the caller, alternating, on the same card). Reads nothing outside
the repository.

  python tools/reconcile_bench.py [--reps 20] [--frames 4096] [--out profiles/reconcile_bench.json]
         [--headline this=run1.json,run2.json,run3.json parent=run1.json,...]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qkd_ldpc_amd as Q  # noqa: E402


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "spread_ms": max(ms) - min(ms), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--qber", type=float, default=0.02)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconcile_bench.json"))
    ap.add_argument("--headline", nargs="*", default=[], metavar="NAME=FILE,FILE,...",
                    help="bench.py result files of a build (their last line is the JSON result)")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")

    g = np.load(os.path.join(ROOT, "tests", "golden", "code_n10240.npz"))
    H = Q.HMatrix.from_check_lists(int(g["dims"][0]), g["chk_off"], g["chk_idx"])
    ws = Q.Workspace(H)
    seeds = torch.from_numpy(Q.make_seeds(777, args.frames).view(np.int64)).cuda()
    alice, bob, q = Q.keygen(H, seeds, args.qber)
    q = float(q[0])
    syn = Q.calculate_syndrome(H, alice)
    lp = math.log((1 - q) / q)
    # (the 8 bytes per position a caller of the LLR entry has to build and the decoder to read)
    llr = torch.where(bob != 0, torch.tensor(-lp, dtype=torch.float64, device="cuda"),
                      torch.tensor(lp, dtype=torch.float64, device="cuda"))
    calls = {
        "reconcile": lambda: Q.reconcile(H, bob, syn, q, workspace=ws),
        "qkd_ldpc_want_bits": lambda: Q.qkd_ldpc(H, alice, bob, q, want_bits=True, workspace=ws),
        "sum_product_decoding_llr": lambda: Q.sum_product_decoding(H, llr, syn, workspace=ws),
    }
    out = {}
    for name, fn in calls.items():              # warm: allocations, tables, the speculation policy
        for _ in range(3):
            out[name] = fn()
    torch.cuda.synchronize()
    ra, rb, rc = (out[k] for k in calls)
    same = bool(torch.equal(ra.bits, rb.bits) and torch.equal(ra.iterations, rb.iterations)
                and torch.equal(ra.bits, rc.bits) and torch.equal(ra.iterations, rc.iterations))
    ms = {k: [] for k in calls}
    for _ in range(args.reps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    res = {"code": "golden N=10240 M=5231", "frames": args.frames, "qber": q,
           "device": torch.cuda.get_device_name(0), "outputs_equal": same,
           "llr_bytes": llr.numel() * 8,
           "calls": {k: summary(v) for k, v in ms.items()}}
    a, b, c = (res["calls"][k]["median_ms"] for k in calls)
    res["ratio_reconcile_over_qkd_ldpc"] = a / b
    res["ratio_llr_over_reconcile"] = c / a
    res["reconcile_within_qkd_ldpc_spread"] = bool(a <= b + res["calls"]["qkd_ldpc_want_bits"]["spread_ms"])
    if args.headline:
        head = {}
        for item in args.headline:
            name, _, files = item.partition("=")
            steps = []
            for f in files.split(","):
                with open(f) as fh:
                    steps.append(json.loads(fh.read().strip().splitlines()[-1])["ms_per_step"])
            head[name] = {"ms_per_step": steps, "median_ms": statistics.median(steps),
                          "spread_ms": max(steps) - min(steps)}
        if "this" in head and "parent" in head:
            head["agree_within_parent_spread"] = bool(
                abs(head["this"]["median_ms"] - head["parent"]["median_ms"]) <= head["parent"]["spread_ms"])
        res["headline_bench"] = head
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
