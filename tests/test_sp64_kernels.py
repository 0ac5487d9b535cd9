"""The binary64 sum-product decoder held to its references on every kernel a code
can give it, not only on the golden code's bucket 6 (tests/test_gpu_parity.py,
test_spec.py, test_adapt*.py) and the (3,6) codes of tests/test_large_codes.py.

One table of cases, code x entry x forcing options x parameters, used twice, in the
pattern of tests/test_variant_kernels.py:
  * on the CPU, the launch's decision (csrc/qkd_launch.h choose_decode through
    tests/native/launch_choice_check.cpp) must name the kernel the case is meant
    for, the written-out set NEED of instantiations must be covered, and the
    references alone must meet the conditions that make a case worth running
    (frames that decode after three iterations or more, frames that end at the cap,
    checks with one and with several erased inputs);
  * on the GPU, every decoded word, iteration count and flag equals the
    reference's: the oracle (oracle/oracle.c) for the keys, LLR and trials entries,
    tests/adapt_model.py with the oracle's libm for the erasure rule and the class
    bytes, tests/adapt_verify_model.py for the payload tags. No tolerance anywhere;
    the NaN paths of the unclamped rule on checks of degree 1 are compared as they
    are.
The codes are the smallest that select each kernel: one per check-degree bucket
with checks of degree 1 and 2 and a largest degree at the bucket's top, bit
degrees other than 3, N past the LDS totals (20,480), M past the interleaved
decoder's two LDS thresholds, N past the split kernel's 65,536 bits."""
import collections
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import write_alist
from test_launch_choice import K_LDS_MAX, K_MAX_BITS_SPLIT, ilv_lds, run_cases
from test_variant_kernels import (ALL_SPECS, CODE_SPECS, CYC8, DV2, FRAMES, NATIVE, _degrees, code, frames, parse,
                                  write_code)
from tests import adapt_model as AM
from tests import adapt_verify_model as VM

K_MAX_BITS_LDS = 20480
K_MAX_CHECKS_SPLIT = 65536

# ---- the codes -------------------------------------------------------------------
CYC4 = [4, 3, 4, 1, 2, 4]
CYC6 = [6, 5, 6, 1, 2, 4, 6, 3]
CYC16 = [16, 9, 1, 12, 2, 15, 3, 16]
CYC64 = [64, 33, 1, 50, 2, 17, 40]
CYC4L = [4, 4, 3, 4, 1, 4, 2, 4]           # average 3.25: M < N, so N past 65,536 keeps M under it
CYC8T = [8, 3, 4, 1, 2, 5, 3, 4]           # low averages: M past a threshold at a small N
CYC16T = [16, 1, 2, 5, 9, 3, 4]

# name -> (seed, bit degrees, check degrees); from test_variant_kernels: i8 (degrees 1 .. 8), dv5
# (bit degrees 1, 2, 3, 5: no packed bit words, nothing speculates), dv2 (bit degrees 2 and 3,
# bucket 6), i16g / i64g (N = 21,000: the classic kernel's totals in global scratch)
SPECS64 = {
    "i4": (201, DV2, _degrees(CYC4, sum(DV2))),                    # bit degrees 2 and 3, checks 1 .. 4
    "i6": (202, [3] * 2048, _degrees(CYC6, 3 * 2048)),
    "j16": (203, [3] * 2048, _degrees(CYC16, 3 * 2048)),
    "j64": (204, [3] * 2048, _degrees(CYC64, 3 * 2048)),
    # the interleaved decoder's target words in global memory (TG): M in (24,508, 36,764]
    "t4": (205, [3] * 27200, _degrees(CYC4L, 3 * 27200)),
    "t8": (206, [3] * 31500, _degrees(CYC8T, 3 * 31500)),
    "t16": (207, [3] * 48000, _degrees(CYC16T, 3 * 48000)),
    # its uncertainty words there too (UG): M past 36,764; N past 65,536 with N mod 64 = 2: the
    # long codes, whose hand-offs the LONG split kernel decodes
    "u4": (208, [3] * 65602, _degrees(CYC4L, 3 * 65602)),
    "u8": (209, [3] * 65602, _degrees(CYC8, 3 * 65602)),
    "u16": (210, [3] * 70722, _degrees(CYC16T, 3 * 70722)),
    # no check of degree 1: without the clamp such a check sends +-inf, the next b2c on its
    # edge is inf - inf, and the NaN reaches every bit within a few iterations; the CLAMP =
    # false kernels are held to finite messages on these codes (k4, and dv2, r8, i16, i64)
    "k4": (211, DV2, _degrees([4, 3, 4, 2, 4, 3], sum(DV2))),
    # every row of the interleaved decoder's <16,16> form full
    "r16": (212, [3] * 4096, [16] * 768),
}
IMPORTED = ["i8", "dv5", "dv2", "i16g", "i64g", "r8", "i16", "i64"]
ALL_SPECS.update(SPECS64)
SMALL = {4: "i4", 6: "i6", 8: "i8", 16: "j16", 64: "j64"}       # the small code of each bucket
CLEAN = {4: "k4", 6: "dv2", 8: "r8", 16: "i16", 64: "i64"}      # ... without a check of degree 1
DEG1 = ("i4", "i6", "i8", "j16", "j64", "dv5")                   # codes with checks of degree 1
GT = {16: "i16g", 64: "i64g"}
TG = {4: "t4", 8: "t8", 16: "t16"}
UG = {4: "u4", 8: "u8", 16: "u16"}
EDGE = ("i4", "i6", "i8", "j16", "j64")                          # checks of degree 1 and 2
ILV_FRAMES = 40          # with QKD_ILV_GRID=2: 16 columns per workgroup refill, the last round ragged
MODEL_FRAMES = {"i16g": 2, "i64g": 2}                            # the numpy model on 63,000 edges
# the share of the bits the erasure and class cases puncture, and again shorten (a check of
# degree 64 beside two erased bits says nothing: fewer on those codes)
ERASED = {"j64": 0.003, "i64g": 0.003, "i64": 0.01}
NAMES = list(SPECS64) + IMPORTED


@functools.lru_cache(maxsize=None)
def graph(name):
    n, m, off, idx = code(name)
    return AM.Graph(n, off, idx)


# ---- the parameters ----------------------------------------------------------------
# QBER per code, chosen on the CPU with the references alone (test_reference_*): Q_MAIN the
# reference decodes at least half of the frames and one decoded frame takes three iterations or
# more; Q_HIGH with the clamp at 2.5 and 4 iterations fewer than half decode. The erasure and
# class entries erase or fix 6 % of the bits and take Q_ERA.
Q_MAIN = {"i4": 0.03, "i6": 0.04, "i8": 0.03, "j16": 0.012, "j64": 0.002, "dv5": 0.02, "dv2": 0.05, "i16g": 0.008,
          "i64g": 0.002, "t4": 0.05, "t8": 0.05, "t16": 0.02, "u4": 0.05, "u8": 0.03, "u16": 0.02,
          "k4": 0.05, "r8": 0.02, "i16": 0.012, "i64": 0.002, "r16": 0.01}
Q_HIGH = {"i4": 0.15, "i6": 0.12, "i8": 0.08, "j16": 0.05, "j64": 0.02, "dv5": 0.08, "dv2": 0.12, "i16g": 0.05,
          "i64g": 0.02, "t4": 0.15, "t8": 0.15, "t16": 0.08, "u4": 0.15, "u8": 0.08, "u16": 0.08}
Q_ERA = dict(Q_MAIN)

Par = collections.namedtuple("Par", "max_it thr thr_on high")
PARS = {
    "main": Par(30, 100.0, True, False),
    "noclamp": Par(30, 100.0, False, False),    # the CLAMP = false instantiations
    "stuck": Par(4, 2.5, True, True),           # most frames end at max_it
    # the speculative kernels where they must give up: Q_HIGH under main's clamp and cap, so
    # that interval iterations are replayed exactly (SPEC 1), checkpoints restored (SPEC 2)
    # and interleaved columns handed off (LONG); spec_replays(ws) > 0 is asserted
    "replay": Par(30, 100.0, True, True),
}
MODE = {"keys": 1, "llr": 0, "trials": 1, "llr_era": 0, "class": 2, "class_vfy": 2}
# a shortened bit's LLR: the default clamp; without the clamp 20, since tanh(50) = 1 exactly and a
# check of degree 2 beside such a bit sends 2 atanh(+-1) = +-inf, then inf - inf, on any code
KNOWN = {"main": 100.0, "stuck": 100.0, "noclamp": 20.0}
HASH_SEED = 0x5eed64


def key(kind, mode, dc, clamp, gt=0, spec=0, lng=0, era=0, vfy=0, rs=0, tg=0, ug=0):
    """a KernelKey of the binary64 rule as launch_choice_check.cpp prints it"""
    return "%s:%d,0,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d" % (kind, mode, dc, clamp, gt, spec, lng, era, vfy, rs, tg, ug)


def fields(k):
    """mode, rule, dc, clamp, gt, spec, lng, era, vfy, rs, tg, ug of a key"""
    return [int(x) for x in k.split(":")[1].split(",")]


def entry_key(kind, entry, dc, clamp, **kw):
    era = int(entry in ("llr_era", "class", "class_vfy"))
    return key(kind, MODE[entry], dc, clamp, era=era, vfy=int(entry == "class_vfy"), **kw)


# code, entry, the debug options (name, value)..., parameters, the decoder's key, the interleaved
# decoder's and its hand-off kernel's keys (None: the split or classic path), the check phases'
# form (QKD_CHECK_LANES as applied)
Case = collections.namedtuple("Case", "code entry opts par decoder ilv handoff cl_form")

CAP0 = (("QKD_SPEC_CAP", "0"),)
CLASSIC = (("QKD_DECODE_KERNEL", "classic"),)
CKPT = (("QKD_CKPT_UNSAT", "128"), ("QKD_SPEC_CKPT", "1"))
CKPT_ALL = (("QKD_CKPT_UNSAT", "100000"), ("QKD_SPEC_CKPT", "1"))    # every frame speculates from iteration 1
ILV = (("QKD_ILV", "1"), ("QKD_ILV_GRID", "2"))
LANES0 = (("QKD_CHECK_LANES", "0"),)
ERA_ENTRIES = ("llr_era", "class", "class_vfy")


def _cases():
    out = []

    def add(name, entry, opts, par, decoder, ilv=None, handoff=None, cl_form=0):
        out.append(Case(name, entry, tuple(sorted(opts)), par, decoder, ilv, handoff, cl_form))

    for b, name in SMALL.items():
        spec = b != 64                     # (j64: no packed bit words, nothing speculates)
        lanes = 1 if b in (4, 6) else 0    # the check-lane form is the default at buckets 4 and 6
        for entry in ("keys", "llr"):
            # split, exact
            add(name, entry, CAP0 if spec else (), "main", entry_key("split", entry, b, 1))
            add(name, entry, (), "noclamp", entry_key("split", entry, b, 0))
            # classic
            add(name, entry, CLASSIC, "main", entry_key("classic", entry, b, 1))
            add(name, entry, CLASSIC, "noclamp", entry_key("classic", entry, b, 0))
            # split, SPEC 1
            if spec:
                k = entry_key("split", entry, b, 1, spec=1)
                add(name, entry, (), "main", k, cl_form=lanes)
                add(name, entry, (), "replay", k, cl_form=lanes)
        # split, SPEC 2
        if spec:
            k = entry_key("split", "keys", b, 1, spec=2)
            add(name, "keys", CKPT, "main", k)
            add(name, "keys", CKPT_ALL, "replay", k)
        # the erasure rule and the class bytes, split and classic
        for entry in ERA_ENTRIES:
            for par in ("main", "noclamp"):
                add(name, entry, (), par, entry_key("split", entry, b, int(par == "main")))
                add(name, entry, CLASSIC, par, entry_key("classic", entry, b, int(par == "main")))
        # frames that end at the cap, once per family and entry
        entry = ("keys", "llr")[b in (6, 16)]
        add(name, entry, CAP0 if spec else (), "stuck", entry_key("split", entry, b, 1))
        add(name, ("llr", "keys")[b in (6, 16)], CLASSIC, "stuck",
            entry_key("classic", ("llr", "keys")[b in (6, 16)], b, 1))
        if spec:
            add(name, "keys", (), "stuck", entry_key("split", "keys", b, 1, spec=1), cl_form=lanes)
        era_entry = ERA_ENTRIES[list(SMALL).index(b) % 3]
        add(name, era_entry, (), "stuck", entry_key("split", era_entry, b, 1))
    # the CLAMP = false kernels on finite messages: every entry, split and classic
    for b, name in CLEAN.items():
        for entry in ("keys", "llr") + ERA_ENTRIES:
            add(name, entry, (), "noclamp", entry_key("split", entry, b, 0))
            add(name, entry, CLASSIC, "noclamp", entry_key("classic", entry, b, 0))
    # bucket 4, the edge-lane form of the speculative kernel (tests/test_check_lanes*.py hold bucket 6)
    k = entry_key("split", "keys", 4, 1, spec=1)
    add("i4", "keys", LANES0, "main", k)
    add("i4", "keys", LANES0, "replay", k)
    # bit degrees other than 3: dv5 the generic bit phase (exact kernels only), dv2 the packed words
    for entry in ("keys", "llr"):
        add("dv5", entry, (), "main", entry_key("split", entry, 8, 1))
        add("dv5", entry, (), "noclamp", entry_key("split", entry, 8, 0))
        add("dv5", entry, CLASSIC, "main", entry_key("classic", entry, 8, 1))
        add("dv2", entry, (), "main", entry_key("split", entry, 6, 1, spec=1), cl_form=1)
        add("dv2", entry, CAP0, "main", entry_key("split", entry, 6, 1))
    add("dv5", "class_vfy", (), "main", entry_key("split", "class_vfy", 8, 1))
    add("dv2", "keys", CKPT, "main", entry_key("split", "keys", 6, 1, spec=2))
    # the classic kernel with its totals in global scratch (no clamp on its erasure forms: WAIVED)
    for b, name in GT.items():
        for entry in ("keys", "llr"):
            add(name, entry, CLASSIC, "main", entry_key("classic", entry, b, 1, gt=1))
            add(name, entry, CLASSIC, "noclamp", entry_key("classic", entry, b, 0, gt=1))
        for entry in ERA_ENTRIES:
            add(name, entry, CLASSIC, "main", entry_key("classic", entry, b, 1, gt=1))
        add(name, "keys" if b == 16 else "llr", CLASSIC, "stuck",
            entry_key("classic", "keys" if b == 16 else "llr", b, 1, gt=1))
    # the interleaved decoder: plain on the small codes, TG and TG + UG on M past its thresholds;
    # the frames it does not certify go to the exact split kernel (past 65,536 bits: LONG)
    for b in (4, 8, 16):
        rs = 16 if b == 16 else 8
        for name, tg, ug in ((SMALL[b], 0, 0), (TG[b], 1, 0), (UG[b], 1, 1)):
            lng = int(name in UG.values())
            hand = key("split", 1, b, 1, lng=lng)
            dec = hand if lng else key("split", 1, b, 1, spec=1)
            lanes = int(b == 4 and not lng)
            add(name, "trials", ILV, "main", dec, key("ilv", 0, b, 0, rs=rs, tg=tg, ug=ug), hand, lanes)
            if lng or not tg:
                # hand-offs, counted: a cap of one interval round at Q_HIGH
                add(name, "trials", ILV + (("QKD_SPEC_CAP", "1"),), "replay", dec,
                    key("ilv", 0, b, 0, rs=rs, tg=tg, ug=ug), hand, lanes)
    # <16,16> with every row full (r16) and with rows of 9 to 16 (i16): on the codes above the
    # checks of degree 16 are few and their messages weak beside those of the short checks
    for name in ("r16", "i16"):
        add(name, "trials", ILV, "main", key("split", 1, 16, 1, spec=1), key("ilv", 0, 16, 0, rs=16),
            key("split", 1, 16, 1))
    # QKD_ILV=0 on a code whose message slots are mostly global: the speculative split kernel
    add("t8", "trials", (("QKD_ILV", "0"),), "main", key("split", 1, 8, 1, spec=1))
    return out


CASES = _cases()


def case_id(c):
    tag = "+".join(n[4:].lower() + v for n, v in c.opts) or "default"
    return "-".join([c.code, c.entry, c.par, tag])


def case_q(c):
    if PARS[c.par].high:
        return Q_HIGH[c.code]
    return Q_ERA[c.code] if c.entry in ERA_ENTRIES else Q_MAIN[c.code]


def n_frames(c):
    return ILV_FRAMES if c.ilv else FRAMES.get(c.code, 12)


# ---- the instantiations: NEED ----------------------------------------------------------
# Read off the three lookups with rule = kRuleSp64: decode_split.hip split_bucket / split_kernel
# (lines 2146-2212), decode.hip classic_bucket / classic_kernel (656-709), decode_ilv.hip
# ilv_rows / ilv_kernel (608-624), less what choose_decode (qkd_launch.h 432-624) gives no real
# code (UNREACHABLE) and what other modules hold (ELSEWHERE).
def _need():
    need = set()
    for mode in (0, 1):
        for b in (4, 6, 8, 16, 64):
            need |= {key("split", mode, b, cl) for cl in (0, 1)}
            need |= {key("classic", mode, b, cl) for cl in (0, 1)}
        for b in (16, 64):
            need |= {key("classic", mode, b, cl, gt=1) for cl in (0, 1)}
        need |= {key("split", mode, b, 1, spec=1) for b in (4, 6, 8, 16)}
    need |= {key("split", 1, b, 1, spec=2) for b in (4, 6, 8, 16)}
    need |= {key("split", 1, b, 1, lng=1) for b in (4, 8, 16)}
    for entry in ERA_ENTRIES:
        for cl in (0, 1):
            need |= {entry_key("split", entry, b, cl) for b in (4, 6, 8, 16, 64)}
            need |= {entry_key("classic", entry, b, cl) for b in (4, 6, 8, 16, 64)}
            need |= {entry_key("classic", entry, b, cl, gt=1) for b in (16, 64)}
    for b in (4, 8, 16):
        need |= {key("ilv", 0, b, 0, rs=16 if b == 16 else 8, tg=tg, ug=ug) for tg, ug in ((0, 0), (1, 0), (1, 1))}
    return need


NEED = _need()
# Left out, each dominated by a neighbour in the table (at most 12):
WAIVED = {
    # the large-code classic kernel's erasure forms without the clamp: the clamp is one compare
    # per message, held without it on the same kernels' keys and LLR forms (GT 16 / 64 noclamp)
    # and on every non-GT erasure form; the numpy model takes seconds per frame on these codes
    entry_key("classic", e, b, 0, gt=1): "GT erasure form, clamp off: held with the clamp, and without it on the "
                                         "GT keys / LLR kernels and the non-GT erasure kernels"
    for e in ERA_ENTRIES for b in (16, 64)
}
# Instantiated, but no code and call make choose_decode name them (test_unreachable_kernels):
UNREACHABLE = (
    # the packed bit words need every check degree <= 16 (qkd_layout.h packable)
    [key("split", m, 64, 1, spec=1) for m in (0, 1)] + [key("split", 1, 64, 1, spec=2)] +
    # the interleaved decoder speculates, so it needs the clamp; without it a long code is the classic kernel's
    [key("split", 1, b, 0, lng=1) for b in (4, 6, 8, 16)])
# Held by other modules: LONG bucket 6 and decode_ilv_kernel<8, 6, ...> by tests/test_large_codes.py
ELSEWHERE = [key("split", 1, 6, 1, lng=1)] + [key("ilv", 0, 6, 0, rs=8, tg=t, ug=u) for t, u in ((0, 0), (1, 0), (1, 1))]


def covered():
    out = set()
    for c in CASES:
        out |= {c.ilv, c.handoff} if c.ilv else {c.decoder}
    return out


def test_kernels_covered():
    assert len(set(map(case_id, CASES))) == len(CASES)
    assert len(NEED) == 144 and not NEED & (set(UNREACHABLE) | set(ELSEWHERE))
    assert len(WAIVED) <= 12 and set(WAIVED) <= NEED
    assert NEED - covered() <= set(WAIVED), sorted(NEED - covered() - set(WAIVED))
    assert not covered() & set(WAIVED)
    # every SPEC 1 / SPEC 2 kernel and every LONG kernel once where it must give up
    replay = set()
    for c in CASES:
        if c.par == "replay":
            replay |= {c.ilv, c.handoff} if c.ilv else {c.decoder}
    assert {k for k in NEED if fields(k)[5] or fields(k)[6]} <= replay


# ---- CPU: every case is on the kernel it is meant for -------------------------------------

def choice_line(c):
    import qkd_ldpc_amd as Q
    p, opts = PARS[c.par], dict(c.opts)
    flags = Q.decoder_flags(p.thr_on, "sp_f64", None, None, False, c.entry == "llr_era")
    s = "mode=%d flags=%d n_frames=%d spec_cap=%s" % (MODE[c.entry], flags, n_frames(c), opts.get("QKD_SPEC_CAP", "8"))
    if MODE[c.entry] == 1:
        s += " first_table=auto tab2=auto"
    if c.entry in ("keys", "llr", "llr_era"):
        s += " bits_out=1"
    if MODE[c.entry] == 2:
        s += " adapt=1 vfy=%d" % (c.entry == "class_vfy")
    if opts.get("QKD_SPEC_CKPT") == "1":
        s += " ckpt_unsat=" + opts["QKD_CKPT_UNSAT"]
    if "QKD_DECODE_KERNEL" in opts:
        s += " classic=1"
    if "QKD_ILV" in opts:
        s += " ilv=" + opts["QKD_ILV"]
    if "QKD_CHECK_LANES" in opts:
        s += " check_lanes=" + opts["QKD_CHECK_LANES"]
    return s


@pytest.fixture(scope="module")
def choice_bin(tmp_path_factory):
    binary = str(tmp_path_factory.mktemp("sp64_kernels") / "launch_choice_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", binary, NATIVE])
    return binary


@pytest.fixture(scope="module")
def choices(choice_bin, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sp64_cases")
    lines = collections.defaultdict(list)
    for c in CASES:
        lines[c.code].append(case_id(c) + " " + choice_line(c))
    res = {}
    for name, ls in lines.items():
        path = str(tmp / (name + ".code"))
        write_code(path, code(name))
        with open(path + ".cases", "w") as f:
            f.write("\n".join(ls) + "\n")
        res.update(parse(subprocess.check_output([choice_bin, path, path + ".cases"], text=True)))
    return res


def thresholds(m):
    """-> (TG, UG) of M checks: which of the interleaved decoder's word arrays leave the LDS"""
    tg = ilv_lds(m, False, False) > K_LDS_MAX
    return int(tg), int(tg and ilv_lds(m, True, False) > K_LDS_MAX)


def want_choice(c):
    kind, f = c.decoder.split(":")[0], fields(c.decoder)
    spec = f[5] if not c.ilv else 1
    want = dict(status=0, path=2 if c.ilv else int(kind == "split"), bucket=f[2], decoder=c.decoder,
                gt=f[4], spec=int(spec != 0), ckpt=int(spec == 2), cl_form=c.cl_form, tsg=0, ug=0)
    if kind == "split":
        want["tsg"], want["ug"] = thresholds(code(c.code)[1])
    if c.ilv:
        want.update(ilv=c.ilv, handoff=c.handoff, need_ilv=1)
    return want


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_reaches_its_kernel(choices, c):
    got, want = choices[case_id(c)], want_choice(c)
    assert {k: got.get(k) for k in want} == want


def test_unreachable_kernels(choice_bin, tmp_path):
    """The instantiations no code reaches. A check of degree 17 leaves the code without packed
    bit words, so nothing speculates at bucket 64; a long code without the clamp cannot
    speculate, so the interleaved decoder and its LONG hand-off kernel do not take it."""
    facts = ("n=2048 n_pad=2048 m=1024 max_dv=3 n_pat=4 n_tasks=100 has_ilv_slots=0 cu_count=256 first_table=0 "
             "tab2=0 spec_cap=8 n_frames=12 max_dc=17 has_bit_code=0")
    long_ = ("n=70000 n_pad=70016 m=35000 max_dv=3 n_pat=0 n_tasks=3300 cl_dc=%d ilv_rs=%d has_bit_code=1 "
             "has_ilv_slots=1 cu_count=256 first_table=1 tab2=0 spec_cap=8 n_frames=4096 mode=1 max_dc=%d flags=%d")
    cases = {"b64_keys": ("-", facts + " mode=1"), "b64_llr": ("-", facts + " mode=0"),
             "b64_ckpt": ("-", facts + " mode=1 ckpt_unsat=128")}
    for b in (4, 6, 8, 16):
        cases["long%d_noclamp" % b] = ("-", long_ % (b if b <= 6 else 0, 16 if b == 16 else 8, b, 0))
        cases["long%d_clamp" % b] = ("-", long_ % (b if b <= 6 else 0, 16 if b == 16 else 8, b, 1))
    got = run_cases(choice_bin, tmp_path, cases)
    for name in ("b64_keys", "b64_llr", "b64_ckpt"):
        ch = got[name]
        assert (ch["status"], ch["path"], ch["bucket"], ch["spec"], ch["ckpt"]) == (0, 1, 64, 0, 0), name
        assert ch["decoder"] == key("split", int(name != "b64_llr"), 64, 1)
    for b in (4, 6, 8, 16):
        ch = got["long%d_noclamp" % b]
        assert (ch["status"], ch["path"], ch["gt"], ch["decoder"]) == (0, 0, 1, key("classic", 1, 16, 0, gt=1)), b
        ch = got["long%d_clamp" % b]
        assert (ch["path"], ch["handoff"]) == (2, key("split", 1, b, 1, lng=1)), b
    used = {x for ch in got.values() for x in (ch["decoder"], ch["ilv"], ch["handoff"])}
    assert not used & {k for k in UNREACHABLE}


def test_codes_are_as_described():
    assert set(IMPORTED) <= set(CODE_SPECS) and not set(SPECS64) & set(CODE_SPECS)
    for name in NAMES:
        seed, dv, dc = ALL_SPECS[name]
        n, m, off, idx = code(name)
        assert (np.bincount(idx, minlength=n) == dv).all() and (np.diff(off) == dc).all(), name
    # the small codes: checks of degree 1 and 2, irregular, the largest degree at the bucket's top
    for b, name in SMALL.items():
        dc = set(ALL_SPECS[name][2])
        assert {1, 2, b} <= dc and max(dc) == b and len(dc) >= 4, name
        assert 2048 <= code(name)[0] <= 4096
    assert set(ALL_SPECS["i4"][1]) == {2, 3} and set(ALL_SPECS["dv2"][1]) == {2, 3}
    assert set(ALL_SPECS["dv5"][1]) == {1, 2, 3, 5}
    for b, name in CLEAN.items():
        dc = ALL_SPECS[name][2]
        assert min(dc) >= 2 and max(dc) == b and name not in DEG1, name
    assert all(1 in ALL_SPECS[name][2] for name in DEG1) and set(ALL_SPECS["r16"][2]) == {16}
    assert {17, 33, 64} <= set(ALL_SPECS["j64"][2]) and max(ALL_SPECS["i64g"][2]) == 64
    assert max(ALL_SPECS["i16g"][2]) == 16
    # sizes: the classic kernel's LDS totals, the split kernel's bits and checks
    for name in NAMES:
        n, m = code(name)[:2]
        assert (n > K_MAX_BITS_LDS) == (name in list(GT.values()) + list(TG.values()) + list(UG.values())), name
        assert (n > K_MAX_BITS_SPLIT) == (name in UG.values()), name
        assert m <= K_MAX_CHECKS_SPLIT
        assert thresholds(m) == ((1, 1) if name in UG.values() else (1, 0) if name in TG.values() else (0, 0)), name
    for b in (4, 8, 16):
        for name in (TG[b], UG[b]):
            seed, dv, dc = ALL_SPECS[name]
            # packed bit words and interleaved lines: bit degrees <= 3, check degrees 1 .. 16
            assert set(dv) == {3} and {1, 2, b} <= set(dc) and max(dc) == b, name
        assert code(UG[b])[0] % 64 == 2
    # the exact switch points of IlvLds: M = 24,508 is the last with three arrays, 36,764 with two
    assert thresholds(24508) == (0, 0) and thresholds(24509) == (1, 0)
    assert thresholds(36764) == (1, 0) and thresholds(36765) == (1, 1)


# ---- the inputs and the references --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def positions(name):
    """-> (punctured, shortened) positions of a code's erasure and class cases: 3 % of the bits
    each, seeded; on the codes with such checks first a punctured bit on a check of degree 1
    (z = 1 with an empty product: 2 atanh(+-1), then the clamp), two punctured bits sharing a
    check of degree 2 (z = 2) and a shortened bit on a check of degree 1."""
    g = graph(name)
    pu, sh = [], []
    if name in EDGE:
        taken = set()

        def first(deg):
            for j in np.nonzero(g.cdeg == deg)[0]:
                bits = g.cidx[g.cptr[j]:g.cptr[j + 1]].tolist()
                if not taken & set(bits):
                    taken.update(bits)
                    return bits
            raise AssertionError("no free check of degree %d" % deg)
        pu = first(1) + first(2)
        sh = first(1)
    rs = np.random.RandomState(500 + len(name))
    rest = rs.permutation(np.setdiff1d(np.arange(g.n), pu + sh))
    k = max(2, int(round(ERASED.get(name, 0.03) * g.n)))
    return (np.array(pu + rest[:k].tolist(), np.int32), np.array(sh + rest[k:2 * k].tolist(), np.int32))


@functools.lru_cache(maxsize=None)
def inputs(name, entry, par, q):
    """-> a dict of a case's inputs. keys: Alice's and Bob's bits and the QBER; llr: LLRs with
    magnitudes spread over [0.75, 1.25] log_p and Alice's syndromes; llr_era: those with real
    zeros at the punctured positions; class: the payload positions, Bob's payload, the syndromes
    of Alice's frames (0 at the shortened positions) and the contract's LLRs."""
    a, b, qq = frames(name, q, 64 + len(par))
    if entry in ERA_ENTRIES:
        f = MODEL_FRAMES.get(name, len(a))
        a, b = a[:f], b[:f]
    g = graph(name)
    lp = np.log((1 - qq) / qq)
    d = dict(a=a, b=b, q=qq)
    if entry in ("llr", "llr_era"):
        llr = np.where(b == 1, -lp, lp) * np.random.RandomState(1000 + len(par)).uniform(0.75, 1.25, b.shape)
        if entry == "llr_era":
            llr[:, positions(name)[0]] = 0.0
        d.update(llr=llr, syn=np.stack([g.syndrome(x) for x in a]))
    if entry in ("class", "class_vfy"):
        pu, sh = positions(name)
        a = a.copy()
        a[:, sh] = 0
        pay = np.setdiff1d(np.arange(g.n), np.concatenate([pu, sh]))
        llr = np.stack([AM.frame_llrs(g.n, pu, sh, x[pay], qq, KNOWN[par])[0] for x in b])
        d.update(a=a, pay=pay, bob=np.ascontiguousarray(b[:, pay]), llr=llr, syn=np.stack([g.syndrome(x) for x in a]))
    return d


_tmp = None


@functools.lru_cache(maxsize=None)
def _oracle_code(name):
    from oracle import oracle as O
    global _tmp
    _tmp = _tmp or tempfile.TemporaryDirectory(prefix="sp64_alist")
    g = graph(name)
    path = os.path.join(_tmp.name, name + ".alist")
    write_alist(path, g.n, g.m, g.bptr, g.chk_of[g.by_bit], g.cptr, g.cidx)
    return O.Code.from_alist(path)


def trial_seeds(O, c):
    return O.seeds(6400 + len(c.code) + len(c.par), n_frames(c))


_want = {}


def want(O, c):
    """the reference's result of a case (shared by the cases that differ in kernel only): a dict of
    iters, ok and, by entry, bits [F, N], key_ok, exact_q, z1 / z2 (the model's counts of checks
    with one / several erased inputs, summed over the iterations, per frame)"""
    p, q = PARS[c.par], case_q(c)
    entry = "class" if c.entry == "class_vfy" else c.entry
    k = (c.code, entry, c.par, n_frames(c) if entry == "trials" else 0)
    if k in _want:
        return _want[k]
    if entry == "trials":
        t = _oracle_code(c.code).trials(q, trial_seeds(O, c), 0, p.max_it, p.thr, p.thr_on)
        w = dict(iters=t["iters"], ok=t["sp_ok"], key_ok=t["key_ok"], exact_q=t["exact_q"])
    else:
        d = inputs(c.code, entry, c.par, q)
        if entry == "keys":
            r = [_oracle_code(c.code).qkd_ldpc(a, b, d["q"], p.max_it, p.thr, p.thr_on) for a, b in zip(d["a"], d["b"])]
        elif entry == "llr":
            r = [_oracle_code(c.code).decode(x, s, p.max_it, p.thr, p.thr_on) for x, s in zip(d["llr"], d["syn"])]
        else:
            r = [AM.decode(graph(c.code), x, s, O.libm, p.max_it, p.thr, p.thr_on) for x, s in zip(d["llr"], d["syn"])]
        w = dict(iters=np.array([x["iters"] for x in r]), ok=np.array([x["sp_ok"] for x in r]),
                 bits=np.stack([x["out"] for x in r]).astype(np.uint8))
        if entry == "keys":
            w["key_ok"] = np.array([x["key_ok"] for x in r])
        if entry in ERA_ENTRIES:
            w["z1"] = np.array([sum(x["z1"]) for x in r])
            w["z2"] = np.array([sum(x["z2"]) for x in r])
    _want[k] = w
    return w


def _ref_cases(pars, entries=None):
    seen, out = set(), []
    for c in CASES:
        entry = "class" if c.entry == "class_vfy" else c.entry
        k = (c.code, entry, c.par, n_frames(c))
        if c.par in pars and (entries is None or entry in entries) and k not in seen:
            seen.add(k)
            out.append(c)
    return out


@pytest.mark.parametrize("c", _ref_cases(("main",)) + [c for c in _ref_cases(("noclamp",)) if c.code not in DEG1],
                         ids=case_id)
def test_reference_decodes_and_iterates(oracle_mod, c):
    """every main case, and every case without the clamp on a code without checks of degree 1
    (finite messages): the reference decodes at least half of the frames, one of them in three
    iterations or more"""
    w = want(oracle_mod, c)
    assert w["ok"].mean() >= 0.5 and (w["iters"][w["ok"].astype(bool)] >= 3).any(), (w["iters"], w["ok"])


@pytest.mark.parametrize("c", _ref_cases(("stuck",)), ids=case_id)
def test_reference_stuck(oracle_mod, c):
    """every stuck case: fewer than half decode, the others end at the cap"""
    w = want(oracle_mod, c)
    assert w["ok"].mean() < 0.5 and (w["iters"][~w["ok"].astype(bool)] == PARS["stuck"].max_it).all(), (w["iters"], w["ok"])


@pytest.mark.parametrize("c", _ref_cases(("main", "noclamp", "stuck"), ("llr_era", "class")), ids=case_id)
def test_reference_erases(oracle_mod, c):
    """every erasure and class case: checks with one erased input and with several"""
    w = want(oracle_mod, c)
    assert w["z1"].max() > 0 and w["z2"].max() > 0, (w["z1"], w["z2"])


# The interleaved decoder's outputs cannot show a wrong message of its own: it iterates on
# intervals, a frame it cannot certify goes to the exact kernel, and the result is the reference's
# either way (a parity that drops the 16th edge's sign changes no output of this module, only the
# hand-offs: 6 of 40 frames become 35). What must hold instead: on the codes that get this decoder
# by default (most message slots global: the TG and UG codes), at a QBER where the reference
# decodes every frame in fewer iterations than the speculation cap, it certifies the majority
# itself. One that hands most frames off decodes them twice and is slower than the split kernel
# it stands in for. So there at most half of the frames may be handed off.
SPEC_CAP_DEFAULT = 8
CERTIFIES = [c for c in CASES if c.ilv and c.par == "main" and c.code in list(TG.values()) + list(UG.values())]


@pytest.mark.parametrize("c", CERTIFIES, ids=case_id)
def test_reference_within_spec_cap(oracle_mod, c):
    w = want(oracle_mod, c)
    assert w["ok"].all() and w["iters"].max() < SPEC_CAP_DEFAULT, w["iters"]


def test_erasure_edges():
    """the explicit positions: a punctured and a shortened bit each alone on a check of degree 1,
    two punctured bits that are all of a check of degree 2"""
    for name in EDGE:
        g = graph(name)
        pu, sh = positions(name)
        assert len(set(pu.tolist()) | set(sh.tolist())) == len(pu) + len(sh)
        rows = [set(g.cidx[g.cptr[j]:g.cptr[j + 1]].tolist()) for j in range(g.m)]
        assert any(len(r) == 1 and r <= {int(pu[0])} for r in rows), name
        assert any(len(r) == 2 and r == {int(pu[1]), int(pu[2])} for r in rows), name
        assert any(len(r) == 1 and r <= {int(sh[0])} for r in rows), name
    # the LLR entry's erasures are real zeros, nothing else is
    c = next(c for c in CASES if c.entry == "llr_era")
    d = inputs(c.code, "llr_era", c.par, case_q(c))
    assert ((d["llr"] == 0.0).sum(axis=1) == len(positions(c.code)[0])).all()


# ---- GPU ---------------------------------------------------------------------------------

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import qkd_ldpc_amd as Q
    return Q


@pytest.fixture(scope="module")
def hmatrix(Q):
    """one HMatrix per code, made when first asked for"""
    @functools.lru_cache(maxsize=None)
    def get(name):
        n, m, off, idx = code(name)
        return Q.HMatrix.from_check_lists(n, off, idx)
    return get


def _dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x).astype(dtype)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _setup(Q, H, qkd_opt, c):
    for name, value in c.opts:
        qkd_opt(name, value)
    ws = Q.Workspace(H)             # (its own: the speculation's policy remembers earlier calls)
    Q.spec_replays(ws, reset=True)
    return ws


def _check_replays(Q, ws, c):
    n = Q.spec_replays(ws)
    print("%s: %d replays" % (case_id(c), n))
    if c.par == "replay":
        assert n > 0
    return n


def _by(entries):
    return [c for c in CASES if c.entry in entries]


@pytest.mark.gpu
@pytest.mark.parametrize("c", _by(("keys", "llr")), ids=case_id)
def test_decode_equals_oracle(Q, hmatrix, oracle_mod, qkd_opt, c):
    """qkd_ldpc(want_bits=True) / sum_product_decoding against the oracle: words, iterations, flags"""
    w, p = want(oracle_mod, c), PARS[c.par]
    d = inputs(c.code, c.entry, c.par, case_q(c))
    H = hmatrix(c.code)
    ws = _setup(Q, H, qkd_opt, c)
    if c.entry == "keys":
        r = Q.qkd_ldpc(H, _dev(d["a"], np.uint8), _dev(d["b"], np.uint8), float(d["q"]), p.max_it, p.thr, p.thr_on,
                       want_bits=True, workspace=ws)
    else:
        r = Q.sum_product_decoding(H, _dev(d["llr"], np.float64), _dev(d["syn"], np.uint8), p.max_it, p.thr, p.thr_on,
                                   workspace=ws)
    print("iterations", _host(r.iterations).tolist(), "want", w["iters"].tolist())
    assert (_host(r.iterations) == w["iters"]).all()
    assert (_host(r.syndromes_match) == w["ok"]).all()
    assert (_host(r.bits) == w["bits"]).all()
    if c.entry == "keys":
        assert (_host(r.keys_match) == w["key_ok"]).all()
    _check_replays(Q, ws, c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", _by(("trials",)), ids=case_id)
def test_trials_equal_oracle(Q, hmatrix, oracle_mod, qkd_opt, c):
    """run_trials (no decoded words: the interleaved decoder and the LONG kernel take no others)
    against the oracle: iterations, both flags, the exact QBER; hand-offs counted"""
    w, p = want(oracle_mod, c), PARS[c.par]
    H = hmatrix(c.code)
    ws = _setup(Q, H, qkd_opt, c)
    seeds = trial_seeds(oracle_mod, c)
    r = Q.run_trials(H, torch.from_numpy(seeds.view(np.int64)).cuda(), case_q(c), 0, p.max_it, p.thr, p.thr_on,
                     workspace=ws)
    print("iterations", _host(r.iterations).tolist(), "want", w["iters"].tolist())
    assert (_host(r.iterations) == w["iters"]).all()
    assert (_host(r.syndromes_match).astype(bool) == w["ok"]).all()
    assert (_host(r.keys_match).astype(bool) == w["key_ok"]).all()
    assert (_host(r.exact_qber) == w["exact_q"]).all()
    n = _check_replays(Q, ws, c)
    if c in CERTIFIES:
        assert 2 * n <= n_frames(c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", _by(("llr_era",)), ids=case_id)
def test_erasure_equals_model(Q, hmatrix, oracle_mod, qkd_opt, c):
    """sum_product_decoding(erasures=True) on LLRs with real zeros against the model"""
    w, p = want(oracle_mod, c), PARS[c.par]
    d = inputs(c.code, c.entry, c.par, case_q(c))
    H = hmatrix(c.code)
    ws = _setup(Q, H, qkd_opt, c)
    r = Q.sum_product_decoding(H, _dev(d["llr"], np.float64), _dev(d["syn"], np.uint8), p.max_it, p.thr, p.thr_on,
                               workspace=ws, erasures=True)
    print("iterations", _host(r.iterations).tolist(), "want", w["iters"].tolist())
    assert (_host(r.iterations) == w["iters"]).all()
    assert (_host(r.syndromes_match) == w["ok"]).all()
    assert (_host(r.bits) == w["bits"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("c", _by(("class", "class_vfy")), ids=case_id)
def test_class_equals_model(Q, hmatrix, oracle_mod, qkd_opt, c):
    """reconcile_adaptive on explicit positions against the model on the contract's LLRs; with
    alice_tags also the payload tags and `verified`, one frame's tag flipped"""
    w, p = want(oracle_mod, c), PARS[c.par]
    d = inputs(c.code, "class", c.par, case_q(c))
    H = hmatrix(c.code)
    pu, sh = positions(c.code)
    plan = Q.AdaptPlan(H, pu, sh)
    ws = _setup(Q, H, qkd_opt, c)
    kw = {}
    if c.entry == "class_vfy":
        R = VM.expand_key(HASH_SEED, len(d["pay"]))
        alice = np.array([VM.payload_tag(R, x[d["pay"]]) for x in d["a"]], np.uint64)
        alice[1] ^= np.uint64(1)
        kw = dict(hash_seed=HASH_SEED, alice_tags=torch.from_numpy(alice.view(np.int64)).cuda())
    r = Q.reconcile_adaptive(H, plan, _dev(d["bob"], np.uint8), _dev(d["syn"], np.uint8), float(d["q"]), KNOWN[c.par],
                             p.max_it, p.thr, p.thr_on, want_frames=True, workspace=ws, **kw)
    print("iterations", _host(r.iterations).tolist(), "want", w["iters"].tolist())
    assert (_host(r.iterations) == w["iters"]).all()
    assert (_host(r.syndromes_match) == w["ok"]).all()
    assert (_host(r.frames) == w["bits"]).all()
    assert (_host(r.bits) == w["bits"][:, d["pay"]]).all()
    assert (_host(r.corrected) == (w["bits"][:, d["pay"]] ^ d["bob"]).sum(axis=1)).all()
    if c.entry == "class_vfy":
        tags = np.array([VM.payload_tag(R, x[d["pay"]]) for x in w["bits"]], np.uint64)
        assert (_host(r.tags).view(np.uint64) == tags).all()
        assert (_host(r.verified).astype(bool) == (w["ok"].astype(bool) & (tags == alice))).all()
        assert not _host(r.verified)[1]             # (the flipped tag)
    plan.close()
