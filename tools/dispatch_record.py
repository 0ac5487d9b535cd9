"""Record which kernels the decode entries dispatch, case by case:

    python tools/dispatch_record.py OUT.json [--only NAME ...]

Every case runs in a fresh child process under `rocprofv3 --kernel-trace`
(nothing else traced, no counters) with its own time limit; the child (`--case
NAME FILE`) makes one call of the public API on a small code and writes
qkd_debug_check_lanes' three numbers to FILE. Per case the output keeps the
ordered list of (kernel name, grid, block, LDS bytes), durations dropped, the
check-lane numbers, and `choice`: the case as the arguments of
tests/native/launch_choice_check.cpp, which tests/test_launch_choice.py feeds
to choose_decode. The first error ends the run.

QKD_AMD_LIB names another build of the library (an A/B against the parent)."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# frames per call: past the 256 CUs' resident workgroups, so the grids recorded
# are the occupancy's, not the frame count's; FRAMES: the cases with another
# count (the interleaved decoder takes 16 frames per workgroup)
F = 600
FRAMES = {"keys_ilv1": 8192, "trace": 1}
SC = 0x1000000
# name -> (code (tests/test_code_layout.py codes()), entry, entry arguments, debug options, choice arguments)
KEYS = "mode=1 first_table=auto tab2=auto"
CASES = {
    "keys_b6": ("golden_n10240", "keys", {}, {}, KEYS + " spec_cap=8"),
    "keys_b4": ("check_lanes_4", "keys", {}, {}, KEYS + " spec_cap=8"),
    "keys_b64": ("check_degree_17", "keys", {}, {}, KEYS + " spec_cap=8"),
    "keys_dv4": ("bit_degree_4", "keys", {}, {}, KEYS + " spec_cap=8"),
    "keys_lanes0": ("golden_n10240", "keys", {}, {"QKD_CHECK_LANES": 0}, KEYS + " spec_cap=8 check_lanes=0"),
    "keys_lanes1": ("check_lanes_4", "keys", {}, {"QKD_CHECK_LANES": 1}, KEYS + " spec_cap=8 check_lanes=1"),
    "keys_lanes2": ("golden_n10240", "keys", {}, {"QKD_CHECK_LANES": 2}, KEYS + " spec_cap=8 check_lanes=2"),
    "keys_nofold": ("golden_n10240", "keys", {}, {"QKD_FOLD_TABLE": 0}, KEYS + " spec_cap=8 fold_table=0"),
    "keys_always": ("golden_n10240", "keys", {}, {"QKD_SPEC_POLICY": "always"}, KEYS + " spec_cap=8 spec_always=1"),
    "keys_ckpt": ("golden_n10240", "keys", {}, {"QKD_SPEC_CKPT": 1}, KEYS + " spec_cap=8 ckpt_unsat=128"),
    "keys_cap0": ("golden_n10240", "keys", {}, {"QKD_SPEC_CAP": 0}, KEYS + " spec_cap=0"),
    "keys_noclamp": ("golden_n10240", "keys", {"threshold_enabled": False}, {}, KEYS + " flags=0 spec_cap=0"),
    "keys_bits": ("golden_n10240", "keys", {"want_bits": True}, {}, KEYS + " spec_cap=8 bits_out=1"),
    "keys_pad": ("golden_n10240", "keys", {}, {"QKD_C2B_PAD": 64}, KEYS + " spec_cap=8 c2b_pad=64"),
    "keys_budget": ("golden_n10240", "keys", {}, {"QKD_SPLIT_BUDGET": 23000}, KEYS + " spec_cap=8 budget=23000"),
    "keys_classic": ("golden_n10240", "keys", {}, {"QKD_DECODE_KERNEL": "classic"}, KEYS + " spec_cap=8 classic=1"),
    "keys_ilv1": ("golden_n10240", "keys", {}, {"QKD_ILV": 1}, KEYS + " spec_cap=8 ilv=1"),
    "keys_ilv0": ("golden_n10240", "keys", {}, {"QKD_ILV": 0}, KEYS + " spec_cap=8 ilv=0"),
    "f32": ("golden_n10240", "keys", {"variant": "sp_f32"}, {}, KEYS + " flags=17"),
    "f32_budget": ("golden_n10240", "keys", {"variant": "sp_f32"}, {"QKD_SPLIT_BUDGET": 60000},
                   KEYS + " flags=17 budget=60000"),
    "ms_split": ("golden_n10240", "keys", {"variant": "minsum"}, {}, KEYS + " flags=33"),
    "ms_lds": ("golden_n10240", "keys", {"variant": "minsum"}, {"QKD_MINSUM_STORE": "lds"}, KEYS + " flags=33 ms_lds=1"),
    "ms_lds17": ("check_degree_17", "keys", {"variant": "minsum"}, {}, KEYS + " flags=33"),
    "ms_global": ("golden_n10240", "keys", {"variant": "minsum"}, {"QKD_MINSUM_STORE": "global"},
                  KEYS + " flags=33 ms_global=1"),
    "ms_split_sc": ("golden_n10240", "keys", {"variant": "minsum", "minsum_self_correct": True}, {},
                    KEYS + " flags=%d" % (33 | SC)),
    "ms_lds_sc": ("golden_n10240", "keys", {"variant": "minsum", "minsum_self_correct": True},
                  {"QKD_MINSUM_STORE": "lds"}, KEYS + " flags=%d ms_lds=1" % (33 | SC)),
    "llr": ("golden_n10240", "llr", {}, {}, "mode=0 spec_cap=8 bits_out=1"),
    "llr_noclamp": ("golden_n10240", "llr", {"threshold_enabled": False}, {}, "mode=0 flags=0 bits_out=1"),
    "llr_era": ("golden_n10240", "llr", {"erasures": True}, {}, "mode=0 flags=3 spec_cap=8 bits_out=1"),
    "trace": ("check_lanes_4", "trace", {}, {}, "mode=0 trace=1 bits_out=0"),
    "reconcile": ("golden_n10240", "reconcile", {}, {}, KEYS + " spec_cap=8 bits_out=1"),
    "reconcile_classic": ("check_lanes_4", "reconcile", {}, {"QKD_DECODE_KERNEL": "classic"},
                          KEYS + " spec_cap=8 bits_out=1 classic=1"),
    "reconcile_verify": ("golden_n10240", "reconcile", {"hash_seed": 7, "want_tags": True}, {},
                         KEYS + " spec_cap=8 bits_out=1"),
    "class": ("golden_n10240", "adaptive", {}, {}, "mode=2 adapt=1"),
    "class_noclamp": ("golden_n10240", "adaptive", {"threshold_enabled": False}, {}, "mode=2 adapt=1 flags=0"),
    "class_verify": ("golden_n10240", "adaptive", {"hash_seed": 7, "want_tags": True}, {}, "mode=2 adapt=1 vfy=1"),
    "class_classic": ("check_lanes_4", "adaptive", {}, {"QKD_DECODE_KERNEL": "classic"}, "mode=2 adapt=1 classic=1"),
    "class_verify_classic": ("check_lanes_4", "adaptive", {"hash_seed": 7, "want_tags": True},
                             {"QKD_DECODE_KERNEL": "classic"}, "mode=2 adapt=1 vfy=1 classic=1"),
    "blind": ("golden_n10240", "blind", {}, {}, "mode=2 adapt=1"),
    "blind_verify": ("check_lanes_4", "blind", {"hash_seed": 7, "want_tags": True}, {}, "mode=2 adapt=1 vfy=1"),
    "llr_classic": ("check_lanes_4", "llr", {}, {"QKD_DECODE_KERNEL": "classic"}, "mode=0 spec_cap=8 bits_out=1 classic=1"),
}


def child(name, out):
    import numpy as np
    import torch

    import qkd_ldpc_amd as Q
    from tests.test_code_layout import codes

    code, entry, kw, opts, _ = CASES[name]
    n, m, off, idx = codes()[code]
    H = Q.HMatrix.from_check_lists(n, off, idx)
    ws = Q.Workspace(H)
    for k, v in opts.items():
        Q.set_debug_option(k, v, ws)
    rs = np.random.RandomState(5)
    frames = FRAMES.get(name, F)
    alice = rs.randint(0, 2, (frames, n)).astype(np.uint8)
    bob = alice ^ (rs.random_sample((frames, n)) < 0.02).astype(np.uint8)
    a, b = torch.from_numpy(alice).cuda(), torch.from_numpy(bob).cuda()
    if entry == "keys":
        Q.qkd_ldpc(H, a, b, 0.02, workspace=ws, **kw)
    elif entry == "reconcile":
        Q.reconcile(H, b, Q.calculate_syndrome(H, a), 0.02, workspace=ws, **kw)
    elif entry == "trace":
        syn = Q.calculate_syndrome(H, a).cpu().numpy()[0]
        Q.trace_decode(H, np.where(bob[0] == 0, 3.9, -3.9), syn, max_iterations=5)
    elif entry in ("adaptive", "blind"):
        p = 64
        plan = Q.AdaptPlan.choose(H, p, p, 5)
        pay = torch.from_numpy(alice[:, :plan.n_payload].copy()).cuda()
        bpay = torch.from_numpy(alice[:, :plan.n_payload] ^ (alice ^ bob)[:, :plan.n_payload]).cuda()
        fill = torch.from_numpy(alice[:, n - p:].copy()).cuda()
        syn = Q.calculate_syndrome(H, Q.adapt_embed(plan, pay, fill))
        if entry == "adaptive":
            Q.reconcile_adaptive(H, plan, bpay, syn, 0.02, workspace=ws, **kw)
        else:
            Q.reconcile_blind(H, plan, bpay, syn, 0.02, fill, None, None, 32, 2, workspace=ws, **kw)
    else:
        syn = Q.calculate_syndrome(H, a)
        llr = torch.from_numpy(np.where(bob == 0, 3.9, -3.9)).cuda()
        Q.sum_product_decoding(H, llr, syn, workspace=ws, **kw)
    torch.cuda.synchronize()
    with open(out, "w") as f:
        json.dump(list(Q.check_lanes(ws)), f)


def first(row, *names):
    for k in names:
        if k in row:
            return int(row[k])
    raise KeyError(names)


def record(name, tmp):
    d = os.path.join(tmp, name)
    lanes = os.path.join(tmp, name + ".json")
    cmd = ["timeout", "-k", "10", "120", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--case", name, lanes]
    rc = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.DEVNULL).returncode
    if rc == 1:                      # the case's own Python error: reported, the run goes on
        return {"error": "exit status 1"}
    if rc != 0:                      # anything else (a fault, a time limit) ends the run
        raise SystemExit("%s: exit status %d" % (name, rc))
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # (the dispatch's LDS: whichever column of this rocprofv3 carries it)
    lds = [k for k in (rows[0] if rows else {}) if "LDS" in k.upper() or "GROUP_SEGMENT" in k.upper()]
    kernels = [[r["Kernel_Name"], first(r, "Grid_Size_X", "Grid_Size"), first(r, "Workgroup_Size_X", "Workgroup_Size"),
                max(int(r[k]) for k in lds)] for r in rows if "qkd::" in r["Kernel_Name"]]
    if name == next(iter(CASES)):
        print("columns:", ",".join(rows[0]), flush=True)
    return {"code": CASES[name][0], "entry": CASES[name][1], "n_frames": FRAMES.get(name, F),
            "choice": CASES[name][4], "kernels": kernels, "check_lanes": json.load(open(lanes))}


def main():
    if sys.argv[1] == "--case":
        return child(sys.argv[2], sys.argv[3])
    names = sys.argv[sys.argv.index("--only") + 1:] if "--only" in sys.argv else list(CASES)
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in names:
            res[name] = record(name, tmp)
            print(name, len(res[name].get("kernels", ())), "kernels", res[name].get("error", ""), flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
