"""What key verification costs: on the golden N = 10240 code at QBER 0.02 with
4096 frames (keys from keygen, syndromes from calculate_syndrome, Alice's tags
from verify_tags), four calls timed warm with HIP events, alternating, REPS
times each, on one build:

  (a) reconcile(H, bob, syndrome, q)                       no verification
  (b) reconcile(..., hash_seed=, alice_tags=)              tags from the unpack kernel (fused)
  (c) reconcile(...) then verify_tags(H, its bits, ...)    the same tags from a second kernel
  (d) verify_tags(H, alice, ...)                           Alice's half alone, with the
                                                           effective GB/s of its F * N key bytes

Writes profiles/verify_bench.json: per call the median and the min-max spread of
its reps, (b) - (a), (c) - (a), and whether (b) stays within (c) plus the run's
spread (the yardstick for keeping the fused form). --headline adds the step
times of plain bench.py runs of this build and of the parent's (JSON result
lines collected by the caller, alternating, on the same card). Reads nothing
outside the repository.

  python tools/verify_bench.py [--reps 20] [--frames 4096] [--out profiles/verify_bench.json]
         [--headline this=run1.json,run2.json,run3.json parent=run1.json,...]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qkd_ldpc_amd as Q  # noqa: E402

SEED = 0x5EEDC0DE2026


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "spread_ms": max(ms) - min(ms), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--qber", type=float, default=0.02)
    ap.add_argument("--tag-bits", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_bench.json"))
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
    t = args.tag_bits
    at = Q.verify_tags(H, alice, hash_seed=SEED, tag_bits=t)

    def separate():
        r = Q.reconcile(H, bob, syn, q, workspace=ws)
        return r, Q.verify_tags(H, r.bits, hash_seed=SEED, tag_bits=t)

    calls = {
        "reconcile": lambda: Q.reconcile(H, bob, syn, q, workspace=ws),
        "reconcile_verify": lambda: Q.reconcile(H, bob, syn, q, workspace=ws, hash_seed=SEED, tag_bits=t,
                                                alice_tags=at),
        "reconcile_then_verify_tags": separate,
        "verify_tags_alice": lambda: Q.verify_tags(H, alice, hash_seed=SEED, tag_bits=t),
    }
    out = {}
    for name, fn in calls.items():              # warm: allocations, tables, the speculation policy
        for _ in range(3):
            out[name] = fn()
    torch.cuda.synchronize()
    ra, rb, (rc, tc) = out["reconcile"], out["reconcile_verify"], out["reconcile_then_verify_tags"]
    same = bool(torch.equal(ra.bits, rb.bits) and torch.equal(ra.iterations, rb.iterations)
                and torch.equal(ra.corrected, rb.corrected) and torch.equal(ra.bits, rc.bits)
                and torch.equal(rb.tags, tc) and torch.equal(out["verify_tags_alice"], at))
    verified = int(rb.verified.sum())
    keys_equal = int((rb.bits == alice).all(dim=1).sum())
    ms = {k: [] for k in calls}
    for _ in range(args.reps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    res = {"code": "golden N=10240 M=5231", "frames": args.frames, "qber": q, "tag_bits": t,
           "device": torch.cuda.get_device_name(0), "outputs_equal": same,
           "frames_verified": verified, "frames_equal_to_alice": keys_equal,
           "calls": {k: summary(v) for k, v in ms.items()}}
    a, b, c, d = (res["calls"][k]["median_ms"] for k in calls)
    spread = max(res["calls"][k]["spread_ms"] for k in ("reconcile", "reconcile_verify", "reconcile_then_verify_tags"))
    res["verify_cost_fused_ms"] = b - a
    res["verify_cost_separate_ms"] = c - a
    res["run_spread_ms"] = spread
    res["fused_within_separate_plus_spread"] = bool(b <= c + spread)
    # (d): the key bytes it has to read, over its call time (launch included)
    key_bytes = alice.numel()
    res["verify_tags_key_bytes"] = key_bytes
    res["verify_tags_effective_GBps"] = key_bytes / (d * 1e-3) / 1e9
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
