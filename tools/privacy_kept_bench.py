"""What hashing only the kept frames of a block costs, on one build.

One block of B = 9765 frames of N = 10240 bits (99,993,600 bits) hashed to 3.4 * 10^7 bits,
5 % of the frames dropped (a transform of 2^27 points). Three calls, alternating, REPS times
each after two warm calls, timed by a host clock around the call and the device
synchronisation that ends it (so that a synchronisation a route forces is counted), medians
and min-max spreads:

  kept            (a) privacy_amplify_kept on the frames and the flags
  torch_compact   (b) what a caller had to do before: frames[keep.bool()] (a host
                  synchronisation: the shape depends on device data), zero-pad to [1, B * N],
                  privacy_amplify_long
  long_compacted  (c) privacy_amplify_long alone on a block compacted beforehand

Before timing, the three outputs are compared: they must be equal. The expected relation is
(a) <= (b), and (a) - (c) no more than one extra pass over the input bytes; the record says
whether each holds. When --kernel-trace names the directory of a rocprofv3 --kernel-trace run
of `--trace-only`, the record also holds the time per dispatch of the input stages
(ntt_unpack_x_kernel of (c), ntt_gather_x_kernel of (a)) and of the scan, and
ntt_unpack_x_kernel's share of (c): the margin (a) may take over (c).

Writes profiles/privacy_kept_bench.json. Reads nothing outside the repository.

  python tools/privacy_kept_bench.py [--reps 20] [--kernel-trace DIR] [--out FILE]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
      python tools/privacy_kept_bench.py --trace-only
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qkd_ldpc_amd as Q  # noqa: E402

FRAME_BITS, FRAMES, OUT_BITS, DROPPED = 10240, 9765, 34 * 10**6, 0.05
HBM_COPY_TBS = 6.29          # what a float4 copy reaches on this part (of 8.0 TB/s nominal)
TRACE_CALLS, TRACE_WARM = 6, 2
TRACED = ("ntt_unpack_x_kernel", "ntt_gather_x_kernel", "kept_scan_kernel")


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "spread_ms": max(ms) - min(ms), "reps": len(ms)}


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed(calls, reps):
    """Warm every call twice, then alternate them."""
    for fn in calls.values():
        for _ in range(2):
            once(fn)
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            ms[name].append(once(fn))
    return {k: summary(v) for k, v in ms.items()}


def kernel_times(trace_dir):
    """Mean time per dispatch of the input stages and the scan from a rocprofv3 kernel trace
    of --trace-only, the first TRACE_WARM dispatches of each kernel dropped."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    seen = {k: [] for k in TRACED}
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
                  for r in csv.DictReader(open(files[0])))
    for _, name, ns in rows:
        for k in TRACED:
            if k in name:
                seen[k].append(ns / 1e6)
    out = {}
    for k, v in seen.items():
        warm = v[TRACE_WARM:]
        if warm:
            out[k] = {"ms_per_dispatch": statistics.mean(warm), "dispatches": len(warm)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace-only", action="store_true",
                    help="six calls of (c), then six of (a), nothing written")
    ap.add_argument("--kernel-trace", default=None, help="directory of a rocprofv3 --kernel-trace run of --trace-only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "privacy_kept_bench.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    rng = np.random.default_rng(2026)
    n_in = FRAMES * FRAME_BITS
    frames = torch.from_numpy(rng.integers(0, 2, (FRAMES, FRAME_BITS), dtype=np.uint8)).cuda()
    keep_np = (rng.random(FRAMES) >= DROPPED).astype(np.uint8)
    keep = torch.from_numpy(keep_np).cuda()
    words = torch.from_numpy(rng.integers(0, 2**64, Q.privacy_long_key_words(n_in, OUT_BITS), dtype=np.uint64)
                             .view(np.int64)).cuda()
    scratch = torch.empty(Q.privacy_kept_scratch_bytes(FRAME_BITS, FRAMES, OUT_BITS, 1), dtype=torch.uint8, device="cuda")
    assert scratch.numel() >= Q.privacy_long_scratch_bytes(n_in, OUT_BITS)

    def torch_compact():
        sel = frames[keep.bool()]
        block = torch.zeros(1, n_in, dtype=torch.uint8, device="cuda")
        block[0, :sel.numel()] = sel.view(-1)
        return Q.privacy_amplify_long(block, OUT_BITS, hash_words=words, scratch=scratch)

    compacted = torch.zeros(1, n_in, dtype=torch.uint8, device="cuda")
    sel = frames[keep.bool()]
    compacted[0, :sel.numel()] = sel.view(-1)
    kept_frames = int(sel.shape[0])
    del sel
    calls = {"kept": lambda: Q.privacy_amplify_kept(frames, keep, OUT_BITS, hash_words=words, scratch=scratch),
             "torch_compact": torch_compact,
             "long_compacted": lambda: Q.privacy_amplify_long(compacted, OUT_BITS, hash_words=words, scratch=scratch)}
    if args.trace_only:
        for name in ("long_compacted", "kept"):
            for _ in range(TRACE_CALLS):
                calls[name]()
        torch.cuda.synchronize()
        return

    out_a, kept = calls["kept"]()
    same = bool(torch.equal(out_a, calls["torch_compact"]()) and torch.equal(out_a, calls["long_compacted"]()))
    assert same, "the three routes disagree"
    assert kept.cpu().tolist() == [kept_frames] == [int(keep_np.sum())]
    t = timed(calls, args.reps)
    a, b, c = (t[k]["median_ms"] for k in ("kept", "torch_compact", "long_compacted"))
    input_pass_ms = n_in / (HBM_COPY_TBS * 1e9)               # the input bytes once, at the copy rate
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "timing": "host clock around call + synchronize",
           "frame_bits": FRAME_BITS, "frames_per_block": FRAMES, "n_in": n_in, "out_bits": OUT_BITS,
           "frames_kept": kept_frames, "frames_dropped": FRAMES - kept_frames, "outputs_equal": same, "calls": t,
           "kept_minus_torch_compact_ms": a - b, "kept_le_torch_compact": bool(a <= b), "torch_compact_over_kept": b / a,
           "kept_minus_long_compacted_ms": a - c, "kept_within_one_input_pass_of_long_compacted": bool(a - c <= input_pass_ms),
           "input_bytes_once_at_copy_rate_ms": input_pass_ms, "hbm_copy_tb_per_s": HBM_COPY_TBS}
    if args.kernel_trace:
        kt = kernel_times(args.kernel_trace)
        res["kernel_trace"] = kt
        if "ntt_unpack_x_kernel" in kt:
            margin = kt["ntt_unpack_x_kernel"]["ms_per_dispatch"]
            res["unpack_x_share_of_long_compacted"] = margin / c
            res["margin_over_long_compacted_ms"] = margin
            res["kept_within_margin_of_long_compacted"] = bool(a - c <= margin)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
