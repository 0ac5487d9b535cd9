"""What the reveal rounds of blind reconciliation cost on the device against a host loop,
on one build.

4096 frames of the golden N = 10240 code at QBER 0.07, the first 1024 positions of
adapt_positions(seed 5) punctured, none shortened, 256 more bits revealed per round, at
most 5 rounds (payload and fill from a seeded generator, Bob's payload through a binary
symmetric channel at the QBER, frames from adapt_embed, syndromes from
calculate_syndrome). Timed warm with HIP events, alternating, REPS times each:

  blind        one reconcile_blind call: every round's bookkeeping, class bytes and decode
               on the stream, no trip to the host between rounds
  host_loop    the route without it: per round the host reads which frames are open,
               builds the binary64 LLRs of those frames with torch (revealed bits as
               -+known_llr), calls sum_product_decoding(erasures=True) on them, scatters
               the results and advances the counts
  all_skipped  a reconcile_blind call in which every frame is skipped: the launch floor
               of the rounds (no frame is decoded)

Before timing, the two routes are compared (decisions, iterations, flags, rounds and
revealed counts must be equal). Writes profiles/blind_bench.json: per call the median and
min-max spread of its reps, what the rounds did, and the one condition: the device loop
is not slower than the host loop in this record. Reads nothing outside the repository.

  python tools/blind_bench.py [--reps 20] [--frames 4096] [--out profiles/blind_bench.json]
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

KNOWN = 100.0


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "spread_ms": max(ms) - min(ms), "reps": len(ms)}


def timed(calls, reps):
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {k: summary(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--qber", type=float, default=0.07)
    ap.add_argument("--punctured", type=int, default=1024)
    ap.add_argument("--step", type=int, default=256)
    ap.add_argument("--max-rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blind_bench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")

    g = np.load(os.path.join(ROOT, "tests", "golden", "code_n10240.npz"))
    n = int(g["dims"][0])
    H = Q.HMatrix.from_check_lists(n, g["chk_off"], g["chk_idx"])
    ws = Q.Workspace(H)
    q, F, p, step, rounds_max = args.qber, args.frames, args.punctured, args.step, args.max_rounds
    lp_t = torch.tensor(math.log((1.0 - q) / q), dtype=torch.float64, device="cuda")
    known_t = torch.tensor(KNOWN, dtype=torch.float64, device="cuda")
    zero_t = torch.tensor(0.0, dtype=torch.float64, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261021)
    plan = Q.AdaptPlan.choose(H, p, p, 5)
    npay = plan.n_payload
    payload = torch.randint(0, 2, (F, npay), dtype=torch.uint8, device="cuda", generator=gen)
    fill = torch.randint(0, 2, (F, p), dtype=torch.uint8, device="cuda", generator=gen)
    flips = (torch.rand((F, npay), device="cuda", generator=gen) < q).to(torch.uint8)
    bob = (payload ^ flips).contiguous()
    syn = Q.calculate_syndrome(H, Q.adapt_embed(plan, payload, fill))
    pay_pos = torch.from_numpy(np.setdiff1d(np.arange(n), plan.punctured.astype(np.int64))).cuda()
    pu_pos = torch.from_numpy(plan.punctured.astype(np.int64)).cuda()
    rank = torch.arange(p, device="cuda")
    all_skip = torch.ones(F, dtype=torch.uint8, device="cuda")

    def blind(skip=None):
        return Q.reconcile_blind(H, plan, bob, syn, q, fill, None, skip, step, rounds_max, KNOWN,
                                 workspace=ws, want_frames=True)

    def host_loop():
        frames = torch.empty((F, n), dtype=torch.uint8, device="cuda")
        iters = torch.empty(F, dtype=torch.int32, device="cuda")
        ok = torch.empty(F, dtype=torch.uint8, device="cuda")
        nrev = torch.zeros(F, dtype=torch.int64, device="cuda")
        rounds = torch.zeros(F, dtype=torch.int32, device="cuda")
        live = torch.ones(F, dtype=torch.bool, device="cuda")
        for t in range(rounds_max):
            idx = live.nonzero().squeeze(1)              # (the host learns how many: a synchronisation)
            if idx.numel() == 0:
                break
            llr = torch.zeros((idx.numel(), n), dtype=torch.float64, device="cuda")
            llr[:, pay_pos] = torch.where(bob[idx] != 0, -lp_t, lp_t)
            known = torch.where((fill[idx] & 1) != 0, -known_t, known_t)
            llr[:, pu_pos] = torch.where(rank[None, :] < nrev[idx, None], known, zero_t)
            r = Q.sum_product_decoding(H, llr, syn[idx].contiguous(), workspace=ws, erasures=True)
            frames[idx] = r.bits
            iters[idx] = r.iterations
            ok[idx] = r.syndromes_match
            rounds[idx] += 1
            failed = (r.syndromes_match == 0) & (nrev[idx] < p)
            live = torch.zeros(F, dtype=torch.bool, device="cuda")
            live[idx[failed]] = True
            if t + 1 < rounds_max:
                nrev[idx[failed]] = torch.clamp(nrev[idx[failed]] + step, max=p)
        return frames, iters, ok, nrev, rounds

    # the two routes agree
    rb = blind()
    hf, hi, hk, hn, hr = host_loop()
    torch.cuda.synchronize()
    same = bool(torch.equal(rb.frames, hf) and torch.equal(rb.iterations, hi) and torch.equal(rb.syndromes_match, hk)
                and torch.equal(rb.n_revealed.long(), hn) and torch.equal(rb.rounds, hr))
    assert same, "reconcile_blind and the host loop disagree"
    okf = rb.syndromes_match != 0
    rounds_np = rb.rounds.cpu().numpy()
    what = {"outputs_equal": same,
            "frames_converged": int(okf.sum()),
            "frames_correct": int((rb.bits == payload).all(dim=1).sum()),
            "frames_by_rounds": {str(k): int((rounds_np == k).sum()) for k in range(1, rounds_max + 1)},
            "frame_decodes": int(rounds_np.sum()),
            "mean_revealed": float(rb.n_revealed.double().mean()),
            "mean_leak_bits": float(rb.leak_bits.double().mean()),
            "leak_per_key_bit": float(rb.leak_bits.double().mean()) / npay}

    calls = {"blind": blind, "host_loop": host_loop, "all_skipped": lambda: blind(all_skip)}
    for fn in calls.values():                   # warm: code objects, allocations
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    res = {"code": "golden N=10240 M=5231", "device": torch.cuda.get_device_name(0), "qber": q, "frames": F,
           "punctured": p, "shortened": 0, "step": step, "max_rounds": rounds_max, "known_llr": KNOWN,
           "rounds": what, "calls": timed(calls, args.reps)}
    c = res["calls"]
    res["blind_over_host_loop"] = c["blind"]["median_ms"] / c["host_loop"]["median_ms"]
    res["condition_met"] = bool(c["blind"]["median_ms"] <= c["host_loop"]["median_ms"])
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    if not res["condition_met"]:
        sys.exit("the device loop is slower than the host loop in this record")


if __name__ == "__main__":
    main()
