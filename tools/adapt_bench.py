"""What rate-adaptive reconciliation costs against its neighbours, on one build.

4096 frames of the golden N = 10240 code at QBER 0.02 (payload and fill from a seeded
generator, Bob's payload through a binary symmetric channel at the QBER, frames from
adapt_embed, syndromes from calculate_syndrome). Timed warm with HIP events,
alternating, REPS times each:

  reconcile             reconcile(H, bob, syndrome, q)                 folded first iteration,
                                                                       tables, speculation
  adaptive_p0_s0        reconcile_adaptive, p = s = 0                  the class-byte mode, exact
  adaptive_p1024_s0     reconcile_adaptive, p = 1024                   iterations only
  adaptive_p0_s1024     reconcile_adaptive, s = 1024
  llr_route_<shape>     the binary64 LLRs of the same frames built on the device (torch),
                        then sum_product_decoding(erasures=True)       what the mode replaces
  llr_decode_<shape>    that decode alone, the LLRs already in memory

Before timing, reconcile_adaptive and the LLR route are compared on every shape (bits,
iterations and flags must be equal), and p = s = 0 with reconcile. Writes
profiles/adapt_bench.json: per call the median and min-max spread of its reps, the
frames each shape converged, and the one condition this mode has to meet: each adaptive
call is faster than the LLR route of its shape in the same run. Reads nothing outside
the repository.

  python tools/adapt_bench.py [--reps 20] [--frames 4096] [--out profiles/adapt_bench.json]
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

SHAPES = ((0, 0), (1024, 0), (0, 1024))
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
    ap.add_argument("--qber", type=float, default=0.02)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapt_bench.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")

    g = np.load(os.path.join(ROOT, "tests", "golden", "code_n10240.npz"))
    n = int(g["dims"][0])
    H = Q.HMatrix.from_check_lists(n, g["chk_off"], g["chk_idx"])
    ws = Q.Workspace(H)
    q, F = args.qber, args.frames
    lp = math.log((1.0 - q) / q)
    pos_lp = torch.tensor(lp, dtype=torch.float64, device="cuda")
    neg_lp = torch.tensor(-lp, dtype=torch.float64, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261020)

    calls, shapes = {}, {}
    for p, s in SHAPES:
        tag = f"p{p}_s{s}"
        plan = Q.AdaptPlan.choose(H, p + s, p, 5)
        npay = plan.n_payload
        payload = torch.randint(0, 2, (F, npay), dtype=torch.uint8, device="cuda", generator=gen)
        fill = torch.randint(0, 2, (F, p), dtype=torch.uint8, device="cuda", generator=gen) if p else None
        flips = (torch.rand((F, npay), device="cuda", generator=gen) < q).to(torch.uint8)
        bob = (payload ^ flips).contiguous()
        syn = Q.calculate_syndrome(H, Q.adapt_embed(plan, payload, fill))
        taken = np.concatenate([plan.punctured, plan.shortened]).astype(np.int64)
        pay_pos = torch.from_numpy(np.setdiff1d(np.arange(n), taken)).cuda()
        sh_pos = torch.from_numpy(plan.shortened.astype(np.int64)).cuda()

        def build_llr(bob=bob, pay_pos=pay_pos, sh_pos=sh_pos):
            llr = torch.zeros((F, n), dtype=torch.float64, device="cuda")
            llr[:, pay_pos] = torch.where(bob != 0, neg_lp, pos_lp)
            llr[:, sh_pos] = KNOWN
            return llr

        llr0 = build_llr()
        adaptive = lambda plan=plan, bob=bob, syn=syn: Q.reconcile_adaptive(      # noqa: E731
            H, plan, bob, syn, q, KNOWN, workspace=ws, want_frames=True)
        route = lambda syn=syn, build_llr=build_llr: Q.sum_product_decoding(      # noqa: E731
            H, build_llr(), syn, workspace=ws, erasures=True)
        decode = lambda syn=syn, llr0=llr0: Q.sum_product_decoding(               # noqa: E731
            H, llr0, syn, workspace=ws, erasures=True)
        calls[f"adaptive_{tag}"] = adaptive
        calls[f"llr_route_{tag}"] = route
        calls[f"llr_decode_{tag}"] = decode
        # the two routes agree, and the frames decode to Alice's payload
        ra, rl = adaptive(), route()
        torch.cuda.synchronize()
        same = bool(torch.equal(ra.frames, rl.bits) and torch.equal(ra.iterations, rl.iterations)
                    and torch.equal(ra.syndromes_match, rl.syndromes_match))
        assert same, f"reconcile_adaptive and the LLR route disagree at {tag}"
        shapes[tag] = {"p": p, "s": s, "n_payload": npay, "outputs_equal": same,
                       "frames_converged": int(ra.syndromes_match.sum()),
                       "frames_correct": int((ra.bits == payload).all(dim=1).sum()),
                       "mean_iterations": float(ra.iterations.double().mean()),
                       "disclosed_per_key_bit": H.num_check_nodes / npay}
        if p == 0 and s == 0:
            calls = {"reconcile": (lambda bob=bob, syn=syn: Q.reconcile(H, bob, syn, q, workspace=ws)), **calls}
            rr = calls["reconcile"]()
            torch.cuda.synchronize()
            assert torch.equal(rr.bits, ra.bits) and torch.equal(rr.iterations, ra.iterations)

    for fn in calls.values():                   # warm: code objects, allocations, the speculation policy
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {"code": "golden N=10240 M=5231", "device": torch.cuda.get_device_name(0), "qber": q, "frames": F,
           "known_llr": KNOWN, "shapes": shapes, "calls": timed(calls, args.reps)}
    c = res["calls"]
    med = lambda k: c[k]["median_ms"]           # noqa: E731
    res["adaptive_faster_than_llr_route"] = {
        tag: bool(med(f"adaptive_{tag}") < med(f"llr_route_{tag}")) for tag in shapes}
    res["condition_met"] = all(res["adaptive_faster_than_llr_route"].values())
    res["adaptive_over_reconcile"] = med("adaptive_p0_s0") / med("reconcile")
    res["llr_bytes_avoided_per_bit_phase"] = F * n * 8 - F * n
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    if not res["condition_met"]:
        sys.exit("reconcile_adaptive is not faster than the LLR route: the mode has no reason to exist")


if __name__ == "__main__":
    main()
