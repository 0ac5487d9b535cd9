"""What privacy amplification costs, per kernel form, on one build.

Config-2 case: the golden N = 10240 code at QBER 0.02 with 4096 frames (keys from
keygen, syndromes from calculate_syndrome), n_in = 10240, out_bits = 4096. Timed
warm with HIP events, alternating, REPS times each:

  reconcile        reconcile(H, bob, syndrome, q)           the decoder the chain waits for
  table            privacy_amplify(bits, 4096, ...)         QKD_PRIVACY_KERNEL=table
  table1/2/4       the same with 1, 2, 4 outputs per lane   (the tile sizes table chooses from)
  direct           the same                                 QKD_PRIVACY_KERNEL=direct
  default          the same with the option unset           the shipped form

Long-block case: the first 4000 of those frames viewed as 40 blocks of
n_in = 102,400 bits, out_bits = 40,960: table and direct (recorded, not judged).

Before timing, the forms' outputs are compared (they must be equal). Writes
profiles/privacy_bench.json: per call the median and the min-max spread of its reps,
whether the default form stays within reconcile's time, and whether it is the faster
of table and direct. Reads nothing outside the repository.

  python tools/privacy_bench.py [--reps 20] [--frames 4096] [--out profiles/privacy_bench.json]
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

SEED = 0x9A17ACE5EED2026
FORMS = ("table", "table1", "table2", "table4", "direct", None)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "spread_ms": max(ms) - min(ms), "reps": len(ms)}


def amplify(form, keys, out_bits):
    Q.set_debug_option("QKD_PRIVACY_KERNEL", form)
    try:
        return Q.privacy_amplify(keys, out_bits, hash_seed=SEED)
    finally:
        Q.set_debug_option("QKD_PRIVACY_KERNEL", None)


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
    ap.add_argument("--out-bits", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "privacy_bench.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")

    g = np.load(os.path.join(ROOT, "tests", "golden", "code_n10240.npz"))
    n = int(g["dims"][0])
    H = Q.HMatrix.from_check_lists(n, g["chk_off"], g["chk_idx"])
    ws = Q.Workspace(H)
    seeds = torch.from_numpy(Q.make_seeds(777, args.frames).view(np.int64)).cuda()
    alice, bob, q = Q.keygen(H, seeds, args.qber)
    q = float(q[0])
    syn = Q.calculate_syndrome(H, alice)
    bits = Q.reconcile(H, bob, syn, q, workspace=ws).bits
    L = args.out_bits

    name = lambda f: "default" if f is None else f          # noqa: E731
    calls = {"reconcile": lambda: Q.reconcile(H, bob, syn, q, workspace=ws)}
    for f in FORMS:
        calls[name(f)] = (lambda f=f: amplify(f, bits, L))
    outs = {}
    for k, fn in calls.items():                 # warm: code objects, allocations, the speculation policy
        for _ in range(3):
            outs[k] = fn()
    torch.cuda.synchronize()
    same = all(torch.equal(outs["direct"], outs[name(f)]) for f in FORMS)
    assert same, "the kernel forms disagree at the config-2 shape"
    res = {"code": "golden N=10240 M=5231", "device": torch.cuda.get_device_name(0), "qber": q,
           "config2": {"frames": args.frames, "n_in": n, "out_bits": L, "outputs_equal": same,
                       "calls": timed(calls, args.reps)}}
    c = res["config2"]["calls"]
    c2 = res["config2"]
    c2["default_within_reconcile"] = bool(c["default"]["median_ms"] <= c["reconcile"]["median_ms"])
    faster = "table" if c["table"]["median_ms"] <= c["direct"]["median_ms"] else "direct"
    c2["faster_form"] = faster
    # the shipped form: the one whose time the unset option reproduces (within the run's spread)
    c2["default_is_faster_form"] = bool(
        abs(c["default"]["median_ms"] - c[faster]["median_ms"])
        <= abs(c["default"]["median_ms"] - c["direct" if faster == "table" else "table"]["median_ms"]))
    c2["key_bytes"] = bits.numel()
    c2["lookups_table"] = ((args.frames + 31) // 32) * L * ((n + 7) // 8)

    # long blocks: B frames as one input
    B = 10
    blocks = min(40, args.frames // B)
    if blocks >= 1:
        long_keys = bits[:blocks * B].view(blocks, B * n)
        Ll = B * L
        lcalls = {name(f): (lambda f=f: amplify(f, long_keys, Ll)) for f in ("table", "direct")}
        louts = {}
        for k, fn in lcalls.items():
            for _ in range(3):
                louts[k] = fn()
        torch.cuda.synchronize()
        lsame = bool(torch.equal(louts["table"], louts["direct"]))
        assert lsame, "the kernel forms disagree at the long-block shape"
        res["long_block"] = {"blocks": blocks, "n_in": B * n, "out_bits": Ll, "outputs_equal": lsame,
                             "calls": timed(lcalls, args.reps)}
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
