"""What key verification costs inside rate-adaptive and blind reconciliation, on one build.

4096 frames of the golden N = 10240 code, the first 1024 positions of adapt_positions(seed
5) punctured, none shortened (payload and fill from a seeded generator, Bob's payload
through a binary symmetric channel at the QBER, frames from adapt_embed, syndromes from
calculate_syndrome, Alice's tags from verify_tags on the plan). Timed warm with HIP events,
REPS times each, the three adaptive calls alternating with each other and then the two blind
calls with each other:

  adaptive            reconcile_adaptive at QBER 0.02                     (a) no verification
  adaptive_then_tag   reconcile_adaptive, then the 64-bit tag of the      (b) the route without
                      payload through privacy_amplify(n_in = n_payload,       the fused call: one
                      out_bits = 64) under the same key string                more read of F x
                                                                              n_payload bytes
  adaptive_verify     reconcile_adaptive(alice_tags=)                     (c) the tag taken by the
                                                                              decoder kernel
  blind               reconcile_blind at QBER 0.07, 256 bits a round, at most 5 rounds
                      (tools/blind_bench.py's shape)
  blind_verify        the same with alice_tags=: closed by verified

Before timing, (b)'s tags and (c)'s are compared with each other and with Alice's on the
frames that decode to her payload, (c)'s other outputs with (a)'s, and the verifying blind
call's with the plain one's. Writes profiles/adapt_verify_bench.json: per call the median
and min-max spread of its reps and the condition: (c) is not slower than (b) beyond the
spread of the alternating reps. Reads nothing outside the repository.

  python tools/adapt_verify_bench.py [--reps 20] [--frames 4096] [--out profiles/adapt_verify_bench.json]
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

KNOWN = 100.0
SEED = 12345


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
    ap.add_argument("--blind-qber", type=float, default=0.07)
    ap.add_argument("--punctured", type=int, default=1024)
    ap.add_argument("--step", type=int, default=256)
    ap.add_argument("--max-rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapt_verify_bench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")

    g = np.load(os.path.join(ROOT, "tests", "golden", "code_n10240.npz"))
    n = int(g["dims"][0])
    H = Q.HMatrix.from_check_lists(n, g["chk_off"], g["chk_idx"])
    ws = Q.Workspace(H)
    F, p = args.frames, args.punctured
    plan = Q.AdaptPlan.choose(H, p, p, 5)
    npay = plan.n_payload
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261022)
    payload = torch.randint(0, 2, (F, npay), dtype=torch.uint8, device="cuda", generator=gen)
    fill = torch.randint(0, 2, (F, p), dtype=torch.uint8, device="cuda", generator=gen)
    syn = Q.calculate_syndrome(H, Q.adapt_embed(plan, payload, fill))
    bob = {}
    for q in (args.qber, args.blind_qber):
        flips = (torch.rand((F, npay), device="cuda", generator=gen) < q).to(torch.uint8)
        bob[q] = (payload ^ flips).contiguous()
    # one key string for the tag and for privacy_amplify(out_bits = 64): the same words
    words = torch.from_numpy(Q.verify_expand_key(SEED, npay).view(np.int64)).cuda()
    assert Q.privacy_key_words(npay, 64) == words.numel()
    at = Q.verify_tags(plan, payload, hash_words=words)

    qa, qb = args.qber, args.blind_qber

    def adaptive():
        return Q.reconcile_adaptive(H, plan, bob[qa], syn, qa, KNOWN, workspace=ws)

    def adaptive_then_tag():
        r = adaptive()
        return r, Q.privacy_amplify(r.bits, 64, hash_words=words)

    def adaptive_verify():
        return Q.reconcile_adaptive(H, plan, bob[qa], syn, qa, KNOWN, workspace=ws, hash_words=words, alice_tags=at)

    def blind(**kw):
        return Q.reconcile_blind(H, plan, bob[qb], syn, qb, fill, None, None, args.step, args.max_rounds, KNOWN,
                                 workspace=ws, **kw)

    def blind_verify():
        return blind(hash_words=words, alice_tags=at)

    # the routes agree
    ra, (rb, tb), rc = adaptive(), adaptive_then_tag(), adaptive_verify()
    pb, pv = blind(), blind_verify()
    torch.cuda.synchronize()
    for name in ("iterations", "syndromes_match", "bits", "corrected"):
        assert torch.equal(getattr(ra, name), getattr(rc, name)), f"adaptive and adaptive_verify disagree on {name}"
    assert torch.equal(tb[:, 0], rc.tags), "the fused tag is not privacy_amplify's"
    right = (rc.bits == payload).all(dim=1)
    assert torch.equal(rc.verified != 0, right & (rc.syndromes_match != 0))
    assert torch.equal(rc.tags[right], at[right])
    honest = bool(torch.equal(pv.verified, pv.syndromes_match))
    if honest:                                  # (no frame matched on a wrong word: the plain call's outputs)
        for name in ("iterations", "syndromes_match", "bits", "corrected", "rounds", "n_revealed"):
            assert torch.equal(getattr(pb, name), getattr(pv, name)), f"blind and blind_verify disagree on {name}"
    what = {"adaptive": {"frames_converged": int((rc.syndromes_match != 0).sum()),
                         "frames_verified": int((rc.verified != 0).sum()),
                         "mean_iterations": float(rc.iterations.double().mean())},
            "blind": {"frames_converged": int((pv.syndromes_match != 0).sum()),
                      "frames_verified": int((pv.verified != 0).sum()),
                      "matched_on_a_wrong_word": int(((pv.syndromes_match != 0) & (pv.verified == 0)).sum()),
                      "frame_decodes": int(pv.rounds.sum()), "frame_decodes_plain": int(pb.rounds.sum()),
                      "mean_revealed": float(pv.n_revealed.double().mean())}}

    # two alternating groups, each compared within itself (with all five calls in one rotation
    # the adaptive call that followed the two 90 ms blind calls read 7.73 ms, against 7.14 ms for
    # the same call in tools/adapt_bench.py and 7.17 ms for the fused call two places later)
    groups = ({"adaptive": adaptive, "adaptive_then_tag": adaptive_then_tag, "adaptive_verify": adaptive_verify},
              {"blind": blind, "blind_verify": blind_verify})
    for calls in groups:                        # warm: code objects, allocations
        for fn in calls.values():
            for _ in range(3):
                fn()
    torch.cuda.synchronize()
    res = {"code": "golden N=10240 M=5231", "device": torch.cuda.get_device_name(0), "frames": F, "punctured": p,
           "shortened": 0, "n_payload": npay, "qber": qa, "blind_qber": qb, "step": args.step,
           "max_rounds": args.max_rounds, "known_llr": KNOWN, "tag_bits": 64, "outputs": what,
           "calls": {**timed(groups[0], args.reps), **timed(groups[1], args.reps)}}
    c = res["calls"]
    med = lambda k: c[k]["median_ms"]           # noqa: E731
    spread = max(c["adaptive_then_tag"]["spread_ms"], c["adaptive_verify"]["spread_ms"])
    res["verify_over_then_tag"] = med("adaptive_verify") / med("adaptive_then_tag")
    res["verify_over_adaptive"] = med("adaptive_verify") / med("adaptive")
    res["blind_verify_over_blind"] = med("blind_verify") / med("blind")
    res["tag_payload_bytes_not_reread"] = F * npay
    res["condition_met"] = bool(med("adaptive_verify") - med("adaptive_then_tag") <= spread)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    if not res["condition_met"]:
        sys.exit("the fused call is slower than reconcile_adaptive followed by privacy_amplify")


if __name__ == "__main__":
    main()
