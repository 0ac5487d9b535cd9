"""The decode launch's decision (csrc/qkd_launch.h choose_decode) on the CPU,
through a g++ build of the header (tests/native/launch_choice_check.cpp).

(a) Against the commit before the decision was split from the launch:
tests/golden/decode_dispatch_parent.json holds, for the cases the public API
reaches on small codes, the kernels that commit dispatched on an MI355X
(tools/dispatch_record.py under rocprofv3 --kernel-trace: name, grid, block, LDS
bytes, in order) and qkd_debug_check_lanes' numbers. choose_decode must name the
same kernel instantiations with the same LDS bytes and check-lane numbers.
(Grids need the device's occupancy: profiles/launch_choice_ab.txt compares them
on the GPU, with profiles/launch_choice_dispatch.json this change's recording.)

(b) Branch by branch, with expectations read off that commit's launch_decode,
on the same small codes and on synthetic facts for what no small code reaches
(long codes, dead slot words, the interleaved decoder's thresholds)."""
import json
import os
import re
import subprocess

import pytest

from test_code_layout import codes, write_code

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native", "launch_choice_check.cpp")
GOLDEN = os.path.join(HERE, "golden", "decode_dispatch_parent.json")

K_LDS_MAX = 160 * 1024
K_C2B_PAD = 64
K_MAX_BITS_SPLIT = 64 * 1024
SC = 0x1000000
UNSUPPORTED = 8
ERA_TEXT = "the erasure rule: binary64 variant, LLR or class entry, no trace"
SC_TEXT = ("self-corrected min-sum needs the split or the LDS-state min-sum kernel (check degree <= 32, its state "
           "in LDS)")

KEYS = "mode=1 first_table=auto tab2=auto spec_cap=8"
# synthetic facts (code "-"): every CodeFacts field given
BIG = ("n=40000 n_pad=40064 m=20000 max_dv=3 max_dc=6 n_pat=0 n_tasks=1900 cl_dc=6 ilv_rs=8 has_bit_code=1 "
       "has_ilv_slots=1 cu_count=256 mode=1 first_table=1 tab2=0 spec_cap=8")
LONG = ("n=100000 n_pad=100032 m=50000 max_dv=3 max_dc=6 n_pat=0 n_tasks=4700 cl_dc=6 ilv_rs=8 has_bit_code=1 "
        "has_ilv_slots=1 cu_count=256 first_table=1 tab2=0 spec_cap=8 n_frames=4096")

# name -> (code, arguments, expected fields)
CASES = {
    # keys, binary64, clamp: speculation with check lanes and the fold table
    "b6": ("golden_n10240", KEYS, dict(path=1, rule=0, bucket=6, spec=1, ckpt=0, cl_form=1, cl_tasks=80, cl_rem_tasks=10,
                                       ftab_entries=512, decoder="split:1,0,6,1,0,1,0,0,0,0,0,0",
                                       handoff="split:1,0,6,1,0,0,0,0,0,0,0,0", need_plan=1, win_count=4,
                                       # 30912 - 17472 slots = 210 x 64: even, so one more pad
                                       c2b_stride=211 * 64)),
    "b4": ("check_lanes_4", KEYS, dict(path=1, bucket=4, spec=1, cl_form=1, decoder="split:1,0,4,1,0,1,0,0,0,0,0,0")),
    # no packed bit words: no speculation, no check lanes
    "b64": ("check_degree_17", KEYS, dict(path=1, bucket=64, spec=0, cl_form=0, ftab_entries=0, win_count=0,
                                          decoder="split:1,0,64,1,0,0,0,0,0,0,0,0")),
    # speculation on, but no check lanes at buckets 8 and 16 (the code's plans are for bucket 6)
    "b8_spec": ("golden_n10240", KEYS + " max_dc=8", dict(path=1, bucket=8, spec=1, ckpt=0, cl_form=0, cl_split=0,
                                                          cl_tasks=0, cl_rem_tasks=490, ftab_entries=512,
                                                          decoder="split:1,0,8,1,0,1,0,0,0,0,0,0")),
    "b16_spec": ("golden_n10240", KEYS + " max_dc=16 ilv_rs=16 check_lanes=2",
                 dict(path=1, bucket=16, spec=1, cl_form=0, cl_split=0, decoder="split:1,0,16,1,0,1,0,0,0,0,0,0")),
    "b16_ilv": ("golden_n10240", KEYS + " max_dc=16 ilv_rs=16 ilv=1",
                dict(path=2, bucket=16, ilv="ilv:0,0,16,0,0,0,0,0,0,16,0,0", handoff="split:1,0,16,1,0,0,0,0,0,0,0,0")),
    "lanes0": ("golden_n10240", KEYS + " check_lanes=0", dict(cl_form=0, cl_split=0, cl_tasks=0, cl_rem_tasks=490)),
    "lanes1": ("golden_n10240", KEYS + " check_lanes=1", dict(cl_form=1, cl_split=0x80000000 | 80 | 10 << 16)),
    "lanes2": ("golden_n10240", KEYS + " check_lanes=2", dict(cl_form=2, cl_rem_tasks=0)),
    "lanes9": ("golden_n10240", KEYS + " check_lanes=9", dict(cl_form=2)),
    "nofold": ("golden_n10240", KEYS + " fold_table=0", dict(ftab_entries=0, spec=1)),
    "fold1": ("golden_n10240", KEYS + " fold_table=1", dict(ftab_entries=512)),
    "always": ("golden_n10240", KEYS + " spec_always=1", dict(spec_always=1)),
    "ckpt": ("golden_n10240", KEYS + " ckpt_unsat=128", dict(spec=1, ckpt=1, need_ckpt=1, cl_form=0, ftab_entries=0,
                                                             decoder="split:1,0,6,1,0,2,0,0,0,0,0,0")),
    "cap0": ("golden_n10240", KEYS.replace("spec_cap=8", "spec_cap=0"), dict(spec=0, decoder="split:1,0,6,1,0,0,0,0,0,0,0,0")),
    "noclamp": ("golden_n10240", KEYS + " flags=0", dict(spec=0, decoder="split:1,0,6,0,0,0,0,0,0,0,0,0")),
    # kFoldTabMaxEntries = 1024, kFoldTabPat = 64
    "fold_max": ("golden_n10240", KEYS + " n_pat=16 tab2=384", dict(ftab_entries=1024)),
    "fold_over": ("golden_n10240", KEYS + " n_pat=17 tab2=384", dict(ftab_entries=0, spec=1)),
    # binary32: every slot in LDS, or the classic kernel
    "f32": ("golden_n10240", "mode=1 first_table=auto flags=17", dict(path=1, rule=1, esz=4, split_S=30912,
                                                                      decoder="split:1,1,6,1,0,0,0,0,0,0,0,0")),
    "f32_budget": ("golden_n10240", "mode=1 first_table=auto flags=17 budget=60000",
                   dict(path=0, rule=1, decoder="classic:1,1,6,1,0,0,0,0,0,0,0,0", need_c2b=1)),
    # min-sum
    "ms_split": ("golden_n10240", "mode=1 first_table=auto flags=33", dict(path=1, rule=5, split_S=30912,
                                                                           decoder="split:1,5,6,1,0,0,0,0,0,0,0,0")),
    "ms_lds_deg": ("check_degree_17", "mode=1 flags=33", dict(path=0, rule=3, bucket=32, need_c2b=0,
                                                              decoder="classic:1,3,32,1,0,0,0,0,0,0,0,0")),
    "ms_global_deg": ("check_degree_17", "mode=1 flags=33 max_dc=40", dict(path=0, rule=2, bucket=64, need_c2b=1)),
    "ms_lds": ("golden_n10240", "mode=1 first_table=auto flags=33 ms_lds=1", dict(path=0, rule=3, bucket=6)),
    "ms_global": ("golden_n10240", "mode=1 first_table=auto flags=33 ms_global=1", dict(path=0, rule=2, bucket=6)),
    "ms_split_sc": ("golden_n10240", "mode=1 first_table=auto flags=%d" % (33 | SC),
                    dict(path=1, rule=6, ftab_entries=2 * 490 + 160)),
    "ms_lds_sc": ("golden_n10240", "mode=1 first_table=auto ms_lds=1 flags=%d" % (33 | SC), dict(path=0, rule=4)),
    "ms_global_sc": ("golden_n10240", "mode=1 ms_global=1 flags=%d" % (33 | SC), dict(status=UNSUPPORTED, message=SC_TEXT)),
    "ms_deg_sc": ("check_degree_17", "mode=1 max_dc=40 flags=%d" % (33 | SC), dict(status=UNSUPPORTED, message=SC_TEXT)),
    # the classic kernel
    "classic": ("golden_n10240", KEYS + " classic=1", dict(path=0, rule=0, gt=0, decoder="classic:1,0,6,1,0,0,0,0,0,0,0,0",
                                                           first_table=1, tab2_entries=384, spec_cap=8, cl_report=0)),
    "trace": ("golden_n10240", "mode=0 trace=1", dict(path=0, decoder="classic:0,0,6,1,0,0,0,0,0,0,0,0")),
    "gt_bits": ("-", "n=30000 n_pad=30016 m=15000 max_dv=3 max_dc=6 n_pat=8 n_tasks=1400 cu_count=256 mode=1 "
                     "first_table=1 tab2=384 classic=1", dict(path=0, gt=1, bucket=16, first_table=0, tab2_entries=0,
                                                               decoder="classic:1,0,16,1,1,0,0,0,0,0,0,0")),
    "gt_lds": ("-", "n=20000 n_pad=20032 m=10000 max_dv=3 max_dc=6 n_pat=8 n_tasks=940 cu_count=256 mode=1 "
                    "first_table=1 tab2=384 classic=1", dict(path=0, gt=1, first_table=0, tab2_entries=0)),
    "many_checks": ("-", "n=60000 n_pad=60032 m=70000 max_dv=6 max_dc=6 n_tasks=6600 cu_count=256 mode=0",
                    dict(path=0, gt=1)),
    # LLR
    "llr": ("golden_n10240", "mode=0 flags=0", dict(path=1, spec=0, decoder="split:0,0,6,0,0,0,0,0,0,0,0,0")),
    "llr_spec": ("golden_n10240", "mode=0 spec_cap=8", dict(path=1, spec=1, ftab_entries=0,
                                                            decoder="split:0,0,6,1,0,1,0,0,0,0,0,0",
                                                            # 30912 - 18368 slots = 196 x 64: even
                                                            c2b_stride=197 * 64)),
    "llr_era": ("golden_n10240", "mode=0 flags=3 spec_cap=8", dict(path=1, spec=0, spec_cap=0,
                                                                    decoder="split:0,0,6,1,0,0,0,1,0,0,0,0")),
    "llr_era_f32": ("golden_n10240", "mode=0 flags=19", dict(status=UNSUPPORTED, message=ERA_TEXT)),
    "llr_era_classic": ("golden_n10240", "mode=0 flags=3 classic=1", dict(path=0, decoder="classic:0,0,6,1,0,0,0,1,0,0,0,0")),
    # class bytes
    "class": ("golden_n10240", "mode=2 adapt=1 spec_cap=8", dict(path=1, spec=0, spec_cap=0,
                                                                  decoder="split:2,0,6,1,0,0,0,1,0,0,0,0")),
    "class_vfy": ("golden_n10240", "mode=2 adapt=1 vfy=1", dict(path=1, decoder="split:2,0,6,1,0,0,0,1,1,0,0,0")),
    "class_vfy_classic": ("golden_n10240", "mode=2 adapt=1 vfy=1 classic=1",
                          dict(path=0, decoder="classic:2,0,6,1,0,0,0,1,1,0,0,0")),
    "class_no_plan": ("golden_n10240", "mode=2", dict(status=UNSUPPORTED, message=ERA_TEXT)),
    "keys_era": ("golden_n10240", "mode=1 flags=3", dict(status=UNSUPPORTED, message=ERA_TEXT)),
    # binary64 under a budget that leaves fewer than 64 LDS slots
    "b64_budget": ("golden_n10240", KEYS + " budget=23000", dict(path=0, rule=0, gt=0)),
    # QKD_C2B_PAD: the rest rounded to 32 slots plus the pad (at most n_pad)
    "pad": ("golden_n10240", KEYS + " c2b_pad=64", dict(c2b_stride=30912 - 17472 + 64)),
    "pad_big": ("golden_n10240", KEYS + " c2b_pad=999999", dict(c2b_stride=30912 - 17472 + 10304)),
    # the dead slot word: a region of 300 M global slots is past it
    "dead": ("-", "n=60000 n_pad=60032 m=30000 max_dv=5000 max_dc=6 n_tasks=2900 cu_count=256 mode=0",
             dict(path=1, rule=0, dead_ok=0)),
    # the interleaved decoder: forced, and its default rule
    "ilv1": ("golden_n10240", KEYS + " ilv=1", dict(path=2, need_ilv=1, ilv_forced=1, ilv="ilv:0,0,6,0,0,0,0,0,0,8,0,0",
                                                    decoder="split:1,0,6,1,0,1,0,0,0,0,0,0",
                                                    handoff="split:1,0,6,1,0,0,0,0,0,0,0,0", ilv_bytes=48168)),
    "ilv0": ("golden_n10240", KEYS + " ilv=0", dict(path=1, need_ilv=0, ilv_forced=1)),
    "ilv_small": ("golden_n10240", KEYS + " n_frames=65536", dict(path=1)),        # S * 4 >= slots
    "ilv_big": ("-", BIG + " n_frames=2048", dict(path=2, tsg=0, ug=0, ilv_forced=0)),
    "ilv_few": ("-", BIG + " n_frames=2047", dict(path=1)),                        # 2 F < 16 CUs
    "ilv_bits": ("-", BIG + " n_frames=2048 bits_out=1", dict(path=1)),
    "ilv_ckpt": ("-", BIG + " n_frames=2048 ckpt_unsat=128", dict(path=1, ckpt=1)),
    "ilv_nofirst": ("-", BIG.replace("first_table=1", "first_table=0") + " n_frames=2048", dict(path=1, spec=0)),
    "ilv_denied": ("-", BIG + " n_frames=2048 allow_ilv=0", dict(path=1, need_ilv=0)),
    # its syndrome arrays: three in LDS up to M ~ 24,400, the target's in global
    # memory up to ~ 36,600, then the uncertainty words too
    "ilv_tsg_lo": ("-", BIG.replace("m=20000", "m=24000") + " n_frames=2048", dict(path=2, tsg=0, ug=0)),
    "ilv_tsg_hi": ("-", BIG.replace("m=20000", "m=25000") + " n_frames=2048",
                   dict(path=2, tsg=1, ug=0, ilv="ilv:0,0,6,0,0,0,0,0,0,8,1,0")),
    "ilv_ug_lo": ("-", BIG.replace("m=20000", "m=36000") + " n_frames=2048", dict(path=2, tsg=1, ug=0)),
    "ilv_ug_hi": ("-", BIG.replace("m=20000", "m=37000") + " n_frames=2048",
                  dict(path=2, tsg=1, ug=1, ilv="ilv:0,0,6,0,0,0,0,0,0,8,1,1")),
    # long codes: the interleaved decoder with the LONG hand-off kernel, else classic
    "long": ("-", LONG + " mode=1", dict(path=2, decoder="split:1,0,6,1,0,0,1,0,0,0,0,0",
                                          handoff="split:1,0,6,1,0,0,1,0,0,0,0,0", need_ckpt=0, cl_form=0)),
    "long_denied": ("-", LONG + " mode=1 allow_ilv=0", dict(path=0, gt=1, spec_cap=8, cl_report=1, cl_form=0,
                                                             cl_rem_tasks=4700, decoder="classic:1,0,16,1,1,0,0,0,0,0,0,0")),
    "long_llr": ("-", LONG + " mode=0", dict(path=0, gt=1, cl_report=0)),
    "long_dc17": ("-", LONG.replace("max_dc=6", "max_dc=17") + " mode=1", dict(path=0, gt=1, bucket=64)),
}


@pytest.fixture(scope="module")
def choice_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("native") / "launch_choice_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", out, NATIVE])
    return out


def parse(text):
    out = {}
    for ln in text.splitlines():
        name, rest = ln.split(" ", 1)
        if " message=" in rest:
            head, msg = rest.split(" message=", 1)
            out[name] = {"status": int(head.split("=")[1]), "message": msg}
            continue
        d = {}
        for kv in rest.split():
            k, v = kv.split("=", 1)
            d[k] = v if ":" in v else int(v)
        out[name] = d
    return out


def run_cases(binary, tmp, cases):
    """cases: name -> (code, arguments); one run of the program per code"""
    all_codes = None
    res = {}
    for code in sorted({c for c, _ in cases.values()}):
        path = "-"
        if code != "-":
            all_codes = all_codes or codes()
            path = str(tmp / (code + ".code"))
            write_code(path, all_codes[code])
        lines = str(tmp / (code.replace("-", "synthetic") + ".cases"))
        with open(lines, "w") as f:
            for name, (c, args) in cases.items():
                if c == code:
                    f.write(name + " " + args + "\n")
        res.update(parse(subprocess.check_output([binary, path, lines], text=True)))
    return res


@pytest.fixture(scope="module")
def choices(choice_bin, tmp_path_factory):
    return run_cases(choice_bin, tmp_path_factory.mktemp("cases"), {k: v[:2] for k, v in CASES.items()})


@pytest.mark.parametrize("name", sorted(CASES))
def test_branch(choices, name):
    got, want = choices[name], CASES[name][2]
    want = dict({"status": 0}, **want)
    assert {k: got.get(k) for k in want} == want


# The LDS layouts restated from the kernels' side (qkd_launch.h DecodeLds, SplitLds, IlvLds
# as the commit before had them in qkd_decode.h): kDecodeBlock 1024, kFirstTableDeg 16.
def up16(x):
    return (x + 15) & ~15


def m_words(m):
    return (m + 63) // 64 * 2


def split_lds(n_pad, n_words, m, max_dv, dc, tab2, ftab, esz, budget):
    zw = up16(4 * m_words(m) * 4)
    aw = up16(zw + n_pad // 64 * 8)
    tval = up16(aw + n_words * 8)
    ctab = up16(tval + max(16 * (64 + dc) * esz, n_words * 8))
    ftab_at = up16(ctab + 17 * 8 + tab2 * 8)
    ctl = up16(ftab_at + ftab * 8)
    msg = up16(ctl + 48 + (9 * 8 * dc if dc <= 8 else 0) * 4)
    fit = (budget - msg) // esz - 64 if budget > msg + 64 * esz else 0
    S = min(max_dv * n_pad, fit) & ~63
    return msg, S, msg + (S + 64) * esz


def classic_lds(n_pad, n_words, m, dc, tab2, rule, gt, sc):
    esz = 8 if rule == 0 else 4
    msl = rule in (3, 4)
    tval = up16(up16(n_pad * (0 if gt else esz)) + 3 * m_words(m) * 4)
    ctab = up16(tval + max(16 * (64 + dc) * esz, n_words * 16))
    ctl = up16(ctab + 17 * 8 + tab2 * 8 + (n_pad * 2 if tab2 else 0))
    return ctl + 16 + (m * 16 if msl else 0) + (m * 4 if msl and sc else 0)


def ilv_lds(m, tsg, ug):
    mw2 = (m + 1) // 2
    return up16(((0 if tsg else 1) + 1 + (0 if ug else 1)) * mw2 * 4) + 64 * 4 + 17 * 8 + 64 * 4 * 16 * 4


def key_fields(k):
    kind, rest = k.split(":")
    return kind, [int(x) for x in rest.split(",")]


def test_structure(choices):
    """what holds for every choice (read off the launch before the split)"""
    for name, ch in choices.items():
        if ch["status"] != 0:
            continue
        n = int(re.search(r"\bn=(\d+)", CASES[name][1]).group(1)) if CASES[name][0] == "-" else 0
        n_words = (ch["n"] + 63) // 64
        if ch["path"] == 0:
            assert key_fields(ch["decoder"])[0] == "classic", name
            assert ch["lds_bytes"] == classic_lds(ch["n_pad"], n_words, ch["m"], ch["bucket"], ch["tab2_entries"],
                                                  ch["rule"], ch["gt"], ch["sc"]), name
            continue
        assert (ch["split_msg"], ch["split_S"], ch["split_bytes"]) == split_lds(
            ch["n_pad"], n_words, ch["m"], ch["max_dv"], ch["bucket"], ch["tab2_in"], ch["ftab_entries"], ch["esz"],
            ch["lds_budget"]), name
        assert ch["ilv_bytes"] == ilv_lds(ch["m"], ch["tsg"], ch["ug"]), name
        assert ch["split_S"] % 64 == 0 and ch["split_S"] >= 64, name
        assert ch["split_bytes"] <= K_LDS_MAX, name
        assert ch["split_bytes"] == ch["split_msg"] + (ch["split_S"] + 64) * ch["esz"], name
        if "c2b_pad" not in CASES[name][1]:
            assert ch["c2b_stride"] % K_C2B_PAD == 0 and (ch["c2b_stride"] // K_C2B_PAD) % 2 == 1, name
            assert ch["c2b_stride"] >= ch["slots"] - ch["split_S"], name
        if ch["rule"] == 0:
            assert ch["dead_ok"] == ch["dead_check"], name
        else:
            # the binary32 rules: every slot in LDS
            assert ch["split_S"] >= ch["slots"] and ch["dead_ok"] == 1, name
        for k in ("decoder", "handoff"):
            kind, f = key_fields(ch[k])
            assert kind == "split" and f[2] == ch["bucket"], name
            # a long code never gets a non-LONG split kernel
            assert f[6] == (1 if n > K_MAX_BITS_SPLIT else 0), name
        if ch["path"] == 2:
            assert ch["ilv_bytes"] <= K_LDS_MAX and key_fields(ch["ilv"])[0] == "ilv", name
            assert key_fields(ch["handoff"])[1][5] == 0, name      # the hand-offs decode exactly


# ---- against the recorded dispatch of the commit before --------------------------
MODES = {0: "0", 1: "1", 2: "2"}


def kernel_name(key):
    """the instantiation a KernelKey names, as the profiler prints it"""
    kind, (mode, rule, dc, clamp, gt, spec, lng, era, vfy, rs, tg, ug) = key_fields(key)
    b = lambda x: "true" if x else "false"
    if kind == "classic":
        return "decode_kernel<%d, %d, %d, %s, %s, %s, %s>" % (mode, rule, dc, b(clamp), b(gt), b(era), b(vfy))
    if kind == "split":
        return "decode_split_kernel<%d, %d, %d, %s, %d, %s, %s, %s>" % (mode, rule, dc, b(clamp), spec, b(lng), b(era),
                                                                         b(vfy))
    return "decode_ilv_kernel<%d, %d, %s, %s>" % (rs, dc, b(tg), b(ug))


def decoders(kernels):
    out = []
    for name, grid, block, lds in kernels:
        m = re.search(r"(decode_(?:split_|ilv_)?kernel<[^>]*>)", name)
        if m:
            out.append((m.group(1), lds))
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_recorded_dispatch(choice_bin, recorded, tmp_path):
    got = run_cases(choice_bin, tmp_path, {k: (v["code"], v["choice"] + " n_frames=%d" % v["n_frames"]) for k, v in recorded.items()})
    assert len(recorded) >= 40 and {v["entry"] for v in recorded.values()} == {
        "keys", "llr", "reconcile", "adaptive", "blind", "trace"}
    # The profiler's LDS column: where it carries the dispatch's dynamic LDS, the
    # choice's bytes must equal it. The rocprofv3 of the recording reports the
    # kernels' static LDS there, which is 0 for every decoder (the split
    # kernels need that: check_no_static_lds); the choice's bytes are then held
    # by test_structure's restatement of the layouts alone.
    dynamic = any(lds for rec in recorded.values() for _, lds in decoders(rec["kernels"]))
    for name, rec in recorded.items():
        ch = got[name]
        assert ch["status"] == 0, name
        if ch["path"] == 0:
            want = [(kernel_name(ch["decoder"]), ch["lds_bytes"])]
        elif ch["path"] == 1:
            want = [(kernel_name(ch["decoder"]), ch["split_bytes"])]
        else:
            want = [(kernel_name(ch["ilv"]), ch["ilv_bytes"]), (kernel_name(ch["handoff"]), ch["split_bytes"])]
        if not dynamic:
            want = [(k, 0) for k, _ in want]
        got_k = decoders(rec["kernels"])
        if rec["entry"] == "blind":          # one launch per round, the same kernel
            assert len(got_k) >= 1
            want = want * len(got_k)
        assert got_k == want, name
        # a fresh workspace reports -1, 0, 0 until a split launch
        lanes = [ch["cl_form"], ch["cl_tasks"], ch["cl_rem_tasks"]] if ch["cl_report"] else [-1, 0, 0]
        assert rec["check_lanes"] == lanes, name
