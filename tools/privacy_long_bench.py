"""What long-block privacy amplification costs, on one build.

Timed warm with HIP events, the calls of a group alternating, REPS times each (a call
that takes longer than SLOW_MS gets SLOW_REPS), medians and min-max spreads:

  tiled      one block of 2^22 bits hashed to 2^21: privacy_amplify_long against the
             composition a caller can build from privacy_amplify alone (the XOR over 2^20-bit
             input chunks of 2^19-bit output tiles, each under its slice of the key string).
             The long form has to be the faster one; the factor is recorded.
  crossover  at and below the short form's limit, privacy_amplify_long against the table
             and direct kernels: (2^20, 2^19) with 1 and with 128 blocks, and
             (10240 * 32, 4096 * 32) with 128 blocks. Recorded for a later dispatch
             decision; nothing acts on it.
  headline   one block of n_in = 10^8, out_bits = 3.4 * 10^7 (a transform of 2^27 points):
             a call with one block and a call with two; their difference is a block, the
             rest of the first the per-call work (the twiddle table and the key string's
             transform). With the bytes each kernel moves, computed here from the shapes,
             and, when --kernel-trace names the directory of a rocprofv3 --kernel-trace run
             of `--trace-only`, each kernel's share of the block and its bytes per second
             against the HBM rate a copy reaches.

Before timing, outputs that must be equal are compared. Writes
profiles/privacy_long_bench.json. Reads nothing outside the repository.

  python tools/privacy_long_bench.py [--reps 20] [--kernel-trace DIR] [--out FILE]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
      python tools/privacy_long_bench.py --trace-only
"""
import argparse
import collections
import csv
import glob
import json
import os
import re
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qkd_ldpc_amd as Q  # noqa: E402

SEED = 0x10F6B10C5EED2026
M20 = 2**20
SLOW_MS, SLOW_REPS = 250.0, 5
HBM_COPY_TBS = 6.29          # what a float4 copy reaches on this part (of 8.0 TB/s nominal)
HEAD_N, HEAD_L = 10**8, 34 * 10**6
S_LOG2, MAX_COLS = 13, 6     # privacy_ntt.hip: kNttMaxLog2, kNttMaxCols


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "spread_ms": max(ms) - min(ms), "reps": len(ms)}


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(calls, reps):
    """Warm every call, then alternate them; a slow call stops at SLOW_REPS."""
    ms = {k: [] for k in calls}
    first = {}
    for name, fn in calls.items():
        for _ in range(2):
            first[name] = once(fn)
    for r in range(reps):
        for name, fn in calls.items():
            if first[name] > SLOW_MS and r >= SLOW_REPS:
                continue
            ms[name].append(once(fn))
    return {k: summary(v) for k, v in ms.items()}


def short_form(form, keys, out_bits, **kw):
    Q.set_debug_option("QKD_PRIVACY_KERNEL", form)
    try:
        return Q.privacy_amplify(keys, out_bits, **kw)
    finally:
        Q.set_debug_option("QKD_PRIVACY_KERNEL", None)


def tiled_hash(keys, L, words, chunk=M20, tile=2**19):
    """One long block from the short form: XOR over input chunks of output tiles."""
    n_in = keys.shape[1]
    out = torch.zeros(1, (L + 63) // 64, dtype=torch.int64, device=keys.device)
    for o0 in range(0, L, tile):
        lt = min(tile, L - o0)
        for p0 in range(0, n_in, chunk):
            nc = min(chunk, n_in - p0)
            w0 = (p0 + o0) // 64
            part = Q.privacy_amplify(keys[:, p0:p0 + nc], lt, hash_words=words[w0:w0 + Q.privacy_key_words(nc, lt)])
            out[:, o0 // 64:o0 // 64 + part.shape[1]] ^= part
    return out


def random_keys(rng, blocks, n_in):
    return torch.from_numpy(rng.integers(0, 2, (blocks, n_in), dtype=np.uint8)).cuda()


def random_words(rng, count):
    return torch.from_numpy(rng.integers(0, 2**64, count, dtype=np.uint64).view(np.int64)).cuda()


def passes(k):
    """privacy_ntt.hip's plan at S = 13: (strided passes, log2 of the block pass)."""
    sb = min(k, S_LOG2)
    rest = k - sb
    s_max = S_LOG2 - min(S_LOG2 // 2, MAX_COLS)
    return (rest + s_max - 1) // s_max if rest else 0, sb


def bytes_moved(n_in, L):
    """Bytes each kernel of one block reads and writes, from the shapes (the twiddle table,
    which stays in cache, not counted)."""
    k = 6
    while 2**k < n_in + L - 1:
        k += 1
    T, (n_strided, _) = 2**k, passes(k)
    per = {"ntt_unpack_x_kernel": n_in + 4 * T,
           "ntt_strided_kernel<false>": n_strided * 8 * T,
           "ntt_block_kernel<false>": 12 * T,                     # the block, the key string's transform, the block
           "ntt_strided_kernel<true>": n_strided * 8 * T,
           "ntt_pack_kernel": 4 * L + (L + 63) // 64 * 8}
    return {"log2_T": k, "strided_passes": n_strided, "per_kernel": per, "block_total": sum(per.values()),
            "per_call_total": 4 * T + n_strided * 8 * T + 8 * T}  # unpack the string, its passes


def kernel_shares(trace_dir, skip_calls, bm):
    """Per-kernel time of a block from a rocprofv3 kernel trace of --trace-only (calls of one
    block each): the dispatches of the first skip_calls calls dropped, the rest summed per
    kernel and divided by the calls left. The per-call kernels (table, key string) are told
    from a block's by their order: a call's first strided-forward and key-block dispatches."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"]
        if "ntt_" in name:
            rows.append((int(r["Start_Timestamp"]), name, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    calls, cur = [], None
    for _, name, ns in rows:
        if "ntt_table_kernel" in name:
            cur = []
            calls.append(cur)
        if cur is not None:
            cur.append((name, ns))
    calls = calls[skip_calls:]
    if not calls:
        raise SystemExit("the trace holds no warm call")
    n_strided = bm["strided_passes"]
    tot = collections.defaultdict(float)
    for call in calls:
        seen_fwd = 0
        for name, ns in call:
            short = re.search(r"ntt_\w+(<\w+>)?", name).group(0)
            if "ntt_strided_kernel<false>" in short:
                seen_fwd += 1
                if seen_fwd <= n_strided:
                    short += " (key string)"
            tot[short] += ns / 1e6 / len(calls)
    block_ms = sum(v for k, v in tot.items() if k in bm["per_kernel"])
    out = []
    for kname, ms in sorted(tot.items(), key=lambda kv: -kv[1]):
        row = {"kernel": kname, "ms_per_call": ms}
        if kname in bm["per_kernel"]:
            b = bm["per_kernel"][kname]
            row.update(share_of_block=ms / block_ms, bytes=b, tb_per_s=b / ms / 1e9,
                       of_hbm_copy_rate=b / ms / 1e9 / HBM_COPY_TBS)
        out.append(row)
    return {"warm_calls": len(calls), "block_kernels_ms": block_ms, "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace-only", action="store_true", help="six calls of the headline shape, nothing written")
    ap.add_argument("--kernel-trace", default=None, help="directory of a rocprofv3 --kernel-trace run of --trace-only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "privacy_long_bench.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    rng = np.random.default_rng(2026)

    # ---- headline ---------------------------------------------------------------------
    keys2 = random_keys(rng, 2, HEAD_N)
    words = random_words(rng, Q.privacy_long_key_words(HEAD_N, HEAD_L))
    scratch = torch.empty(Q.privacy_long_scratch_bytes(HEAD_N, HEAD_L), dtype=torch.uint8, device="cuda")
    head = {"one_block": lambda: Q.privacy_amplify_long(keys2[:1], HEAD_L, hash_words=words, scratch=scratch),
            "two_blocks": lambda: Q.privacy_amplify_long(keys2, HEAD_L, hash_words=words, scratch=scratch)}
    if args.trace_only:
        for _ in range(6):
            head["one_block"]()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "slow_call_ms": SLOW_MS, "slow_call_reps": SLOW_REPS}
    a, b = head["one_block"](), head["two_blocks"]()
    assert torch.equal(a[0], b[0]) and not torch.equal(b[0], b[1])
    bm = bytes_moved(HEAD_N, HEAD_L)
    t = timed(head, args.reps)
    block_ms = t["two_blocks"]["median_ms"] - t["one_block"]["median_ms"]
    res["headline"] = {"n_in": HEAD_N, "out_bits": HEAD_L, "calls": t, "ms_per_block": block_ms,
                       "ms_per_call_once": t["one_block"]["median_ms"] - block_ms,
                       "input_gbit_per_s": HEAD_N / block_ms / 1e6, "bytes_moved": bm,
                       "block_tb_per_s": bm["block_total"] / block_ms / 1e9,
                       "block_of_hbm_copy_rate": bm["block_total"] / block_ms / 1e9 / HBM_COPY_TBS,
                       "hbm_copy_tb_per_s": HBM_COPY_TBS}
    if args.kernel_trace:
        res["headline"]["kernel_trace"] = kernel_shares(args.kernel_trace, 2, bm)
    del keys2, words, scratch, head, a, b
    torch.cuda.empty_cache()

    # ---- the tiled baseline -----------------------------------------------------------
    n_in, L = 4 * M20, 2 * M20
    keys = random_keys(rng, 1, n_in)
    words = random_words(rng, Q.privacy_long_key_words(n_in, L))
    scratch = torch.empty(Q.privacy_long_scratch_bytes(n_in, L), dtype=torch.uint8, device="cuda")
    calls = {"long": lambda: Q.privacy_amplify_long(keys, L, hash_words=words, scratch=scratch),
             "tiled_short_form": lambda: tiled_hash(keys, L, words)}
    same = bool(torch.equal(calls["long"](), calls["tiled_short_form"]()))
    assert same, "the long form and the tiled composition disagree"
    t = timed(calls, args.reps)
    res["tiled"] = {"n_in": n_in, "out_bits": L, "outputs_equal": same, "calls": t,
                    "short_form_calls": (n_in // M20) * (L // 2**19),
                    "long_is_faster": bool(t["long"]["median_ms"] < t["tiled_short_form"]["median_ms"]),
                    "factor": t["tiled_short_form"]["median_ms"] / t["long"]["median_ms"]}
    del keys, words, scratch, calls
    torch.cuda.empty_cache()

    # ---- the crossover ----------------------------------------------------------------
    res["crossover"] = []
    for n_in, L, blocks in ((M20, 2**19, 1), (M20, 2**19, 128), (10240 * 32, 4096 * 32, 128)):
        keys = random_keys(rng, blocks, n_in)
        scratch = torch.empty(Q.privacy_long_scratch_bytes(n_in, L), dtype=torch.uint8, device="cuda")
        calls = {"long": lambda: Q.privacy_amplify_long(keys, L, hash_seed=SEED, scratch=scratch),
                 "table": lambda: short_form("table", keys, L, hash_seed=SEED),
                 "direct": lambda: short_form("direct", keys, L, hash_seed=SEED)}
        outs = {k: fn() for k, fn in calls.items()}
        same = bool(torch.equal(outs["long"], outs["table"]) and torch.equal(outs["long"], outs["direct"]))
        assert same, f"the forms disagree at {(n_in, L, blocks)}"
        t = timed(calls, args.reps)
        fastest = min(t, key=lambda k: t[k]["median_ms"])
        res["crossover"].append({"n_in": n_in, "out_bits": L, "blocks": blocks, "outputs_equal": same, "calls": t,
                                 "fastest": fastest})
        del keys, scratch, calls, outs
        torch.cuda.empty_cache()

    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
