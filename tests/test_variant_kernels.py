"""The binary32 decoder variants (sp_f32, min-sum, self-corrected min-sum) held to
their models (oracle/variants.py) on every kernel a code can give them, not only
on the ones the golden code reaches (tests/test_variants.py: bucket 6, packed bit
words, folded first iteration).

One table of cases, code x rule x entry x parameters, used twice:
  * on the CPU, the launch's decision (csrc/qkd_launch.h choose_decode through
    tests/native/launch_choice_check.cpp) must name the kernel the case is meant
    for, so a later change of the dispatch cannot leave a GPU case passing on a
    kernel that is tested elsewhere;
  * on the GPU, decoded words, iteration counts and flags equal the model's
    exactly: MinSumModel.decode for the min-sum rules, sp_f32_decode with the
    device's own elementwise steps plugged in for sp_f32.
The codes are the smallest that reach each kernel: check degrees in buckets 8, 16,
32 and 64 with partial segments and checks of degree 1 and 2, bit degrees other
than 3, and the three sizes around the classic kernel's LDS totals (13,056 where
the split store stops fitting a (3,6) code's binary32 slots, 20,480 the last with
LDS totals, 20,544 the first with the totals in global scratch)."""
import collections
import functools
import subprocess

import numpy as np
import pytest

from oracle.variants import MinSumModel, sp_f32_decode
from test_code_layout import _socket_code, write_code
from test_launch_choice import NATIVE, SC_TEXT, UNSUPPORTED, parse

# ---- the codes -------------------------------------------------------------------


def _degrees(cycle, edges):
    """check degrees: `cycle` repeated until the edges are used up, the last check the rest"""
    out, left, i = [], edges, 0
    while left > 0:
        out.append(min(cycle[i % len(cycle)], left))
        left -= out[-1]
        i += 1
    return out


CYC8 = [8, 7, 5, 8, 3, 6, 8, 1, 2, 4]
CYC16 = [16, 9, 12, 10, 15, 11, 3, 16]
CYC32 = [32, 17, 25, 20, 31, 9, 32]
CYC64 = [64, 33, 50, 40, 63, 17, 64]
DV5 = [3] * 2000 + [5] * 500 + [2] * 400 + [1] * 100
DV2 = [3] * 2000 + [2] * 500

# name -> (seed, bit degrees, check degrees)
CODE_SPECS = {
    "r8": (101, [3] * 4096, [8] * 1536),                       # (3,8) regular
    "i8": (102, [3] * 4096, _degrees(CYC8, 3 * 4096)),         # degrees 1 .. 8
    "i16": (103, [3] * 2048, _degrees(CYC16, 3 * 2048)),
    "i32": (104, [3] * 2048, _degrees(CYC32, 3 * 2048)),       # largest degree exactly 32
    "i64": (105, [3] * 2048, _degrees(CYC64, 3 * 2048)),
    "dv5": (106, DV5, _degrees(CYC8, sum(DV5))),               # bit degrees 1, 2, 3, 5: no packed bit words
    "dv2": (107, DV2, _degrees([6, 5, 6, 4, 6, 3], sum(DV2))),  # bit degrees 2 and 3, packed
    "n13056": (108, [3] * 13056, [6] * 6528),                  # binary32 slots no longer all in LDS
    "n20480": (109, [3] * 20480, [6] * 10240),                 # the last with the totals in LDS
    "n20544": (110, [3] * 20544, [6] * 10272),                 # the first with them in global scratch
    "i16g": (111, [3] * 21000, _degrees(CYC16, 3 * 21000)),
    "i64g": (112, [3] * 21000, _degrees(CYC64, 3 * 21000)),
    "i32l": (113, [3] * 13056, _degrees(CYC32, 3 * 13056)),
    "i16l": (114, [3] * 13056, _degrees(CYC16, 3 * 13056)),
}
SMALL = ["r8", "i8", "i16", "i32", "i64", "dv5", "dv2"]
FRAMES = {"i32": 8, "i64": 8, "i64g": 4, "i32l": 8, "i16l": 8, "i16g": 8, "n20544": 8, "n20480": 8, "n13056": 8}
# every code code() and frames() know by name: this module's, and those a module that
# shares the helpers adds (tests/test_sp64_kernels.py; frame counts: FRAMES)
ALL_SPECS = dict(CODE_SPECS)


@functools.lru_cache(maxsize=None)
def code(name):
    seed, dv, dc = ALL_SPECS[name]
    return _socket_code(seed, dv, dc)


@functools.lru_cache(maxsize=None)
def model(name):
    n, m, off, idx = code(name)
    return MinSumModel(n, m, off, idx)


@functools.lru_cache(maxsize=None)
def frames(name, q, seed):
    """-> Alice's and Bob's bits [F, N] with round(q N) flipped positions each, and that QBER"""
    n = code(name)[0]
    rs = np.random.RandomState(seed)
    f = FRAMES.get(name, 12)
    k = max(1, int(round(q * n)))
    a = rs.randint(0, 2, (f, n)).astype(np.uint8)
    b = a.copy()
    for i in range(f):
        b[i, rs.choice(n, k, replace=False)] ^= 1
    return a, b, k / n


@functools.lru_cache(maxsize=None)
def inputs(name, q, par, entry):
    """-> Alice's and Bob's bits, the QBER, the LLRs and the target syndromes of a case.
    The keys entry's LLRs are +-log_p; the LLR entry's have magnitudes spread over
    [0.75, 1.25] log_p, so that a check's first minimum is one edge's and the folded
    first iteration's per-degree constants are not all a message can be."""
    a, b, qq = frames(name, q, 7 + len(par))
    lp = np.log((1 - qq) / qq)
    llr = np.where(b == 1, -lp, lp)
    if entry == "llr":
        llr = llr * np.random.RandomState(1000 + len(par)).uniform(0.75, 1.25, llr.shape)
    return a, b, qq, llr, model(name).syndrome(a)


# ---- the kernels: (code, rule, store) -> (kind, rule, bucket, gt), None: refused -----
SP, MS, SCM = "sp_f32", "minsum", "minsum_sc"
EXPECT = {
    ("r8", SP, None): ("split", 1, 8, 0), ("r8", MS, None): ("split", 5, 8, 0), ("r8", SCM, None): ("split", 6, 8, 0),
    ("r8", MS, "lds"): ("classic", 3, 8, 0), ("r8", MS, "global"): ("classic", 2, 8, 0),
    ("r8", SCM, "lds"): ("classic", 4, 8, 0),
    ("i8", SP, None): ("split", 1, 8, 0), ("i8", MS, None): ("split", 5, 8, 0), ("i8", SCM, None): ("split", 6, 8, 0),
    ("i16", SP, None): ("split", 1, 16, 0), ("i16", MS, None): ("classic", 3, 16, 0),
    ("i16", SCM, None): ("classic", 4, 16, 0), ("i16", MS, "global"): ("classic", 2, 16, 0),
    ("i32", SP, None): ("split", 1, 64, 0), ("i32", MS, None): ("classic", 3, 32, 0),
    ("i32", SCM, None): ("classic", 4, 32, 0), ("i32", MS, "global"): ("classic", 2, 64, 0),
    ("i64", SP, None): ("split", 1, 64, 0), ("i64", MS, None): ("classic", 2, 64, 0), ("i64", SCM, None): None,
    ("dv5", SP, None): ("split", 1, 8, 0), ("dv5", MS, None): ("classic", 3, 8, 0),
    ("dv5", SCM, None): ("classic", 4, 8, 0),
    ("dv2", SP, None): ("split", 1, 6, 0), ("dv2", MS, None): ("split", 5, 6, 0), ("dv2", SCM, None): ("split", 6, 6, 0),
    ("n13056", SP, None): ("classic", 1, 6, 0), ("n13056", MS, None): ("classic", 2, 6, 0),
    ("n13056", SCM, None): None,
    ("n20480", SP, None): ("classic", 1, 6, 0), ("n20480", MS, None): ("classic", 2, 6, 0),
    ("n20480", SCM, None): None,
    ("n20544", SP, None): ("classic", 1, 16, 1), ("n20544", MS, None): ("classic", 2, 16, 1),
    ("n20544", SCM, None): None,
    ("i16g", SP, None): ("classic", 1, 16, 1), ("i16g", MS, None): ("classic", 2, 16, 1),
    ("i64g", SP, None): ("classic", 1, 64, 1), ("i64g", MS, None): ("classic", 2, 64, 1),
    ("i32l", SP, None): ("classic", 1, 64, 0), ("i32l", MS, None): ("classic", 3, 32, 0),
    ("i32l", SCM, None): ("classic", 4, 32, 0),
    ("i16l", SP, None): ("classic", 1, 16, 0),
}

# ---- the parameters ----------------------------------------------------------------
# QBER of the cases that should converge, per code (chosen on the CPU: each rule's
# model decodes at least half of the frames and one decoded frame takes three
# iterations or more; test_minsum_model_conditions holds the min-sum ones to that, the
# GPU tests the sp_f32 ones), and of the cases that must not converge.
Q_MAIN = {"r8": 0.02, "i8": 0.03, "i16": 0.012, "i32": 0.005, "i64": 0.002, "dv5": 0.02, "dv2": 0.05, "n13056": 0.06,
          "n20480": 0.06, "n20544": 0.06, "i16g": 0.008, "i64g": 0.002, "i32l": 0.003, "i16l": 0.008}
Q_HIGH = {"r8": 0.08, "i8": 0.08, "i16": 0.05, "i32": 0.03, "i64": 0.02, "dv5": 0.08, "dv2": 0.12, "n13056": 0.12,
          "n20480": 0.12, "n20544": 0.12, "i16g": 0.05, "i64g": 0.02, "i32l": 0.03, "i16l": 0.05}

Par = collections.namedtuple("Par", "max_it thr thr_on scale offset high")
PARS = {
    "main": Par(30, 100.0, True, None, None, False),
    "stuck": Par(4, 2.5, True, None, None, True),            # most frames end at max_it
    "noclamp": Par(30, 100.0, False, None, None, False),     # the CLAMP = false instantiations
    "scale": Par(30, 100.0, True, 255 / 256, None, False),
    "offset": Par(30, 100.0, True, 0.9375, 0.25, False),
    "sc875": Par(30, 100.0, True, 0.875, None, False),
}

Case = collections.namedtuple("Case", "code rule entry store par")


def _cases():
    out = []
    for i, name in enumerate(CODE_SPECS):
        for rule in (SP, MS, SCM):
            if EXPECT.get((name, rule, None)) is None:
                continue
            out += [Case(name, rule, "llr", None, "main"), Case(name, rule, "keys", None, "main"),
                    Case(name, rule, ("llr", "keys")[(i + (rule == MS)) % 2], None, "stuck")]
            if rule == SCM:
                out.append(Case(name, rule, ("keys", "llr")[i % 2], None, "sc875"))
    # the forced stores
    for name, rule, store in [("r8", MS, "lds"), ("r8", MS, "global"), ("r8", SCM, "lds"), ("i16", MS, "global"),
                              ("i32", MS, "global")]:
        out += [Case(name, rule, "llr", store, "main"), Case(name, rule, "keys", store, "main")]
    # no clamp, once per kernel family and on the codes with checks of degree 1
    # (i8, dv5: scale * (+inf) messages, then inf - inf)
    out += [Case("i8", SP, "keys", None, "noclamp"), Case("i8", MS, "llr", None, "noclamp"),          # split
            Case("i8", SCM, "keys", None, "noclamp"), Case("dv5", SP, "llr", None, "noclamp"),
            Case("dv2", SP, "keys", None, "noclamp"), Case("i64", SP, "llr", None, "noclamp"),
            Case("n13056", SP, "llr", None, "noclamp"), Case("i32l", SP, "keys", None, "noclamp"),    # LDS totals
            Case("n20544", SP, "keys", None, "noclamp"), Case("i16g", MS, "llr", None, "noclamp"),    # GT
            Case("i64g", SP, "llr", None, "noclamp"),
            Case("i16", MS, "llr", None, "noclamp"), Case("dv5", MS, "keys", None, "noclamp"),        # LDS state
            Case("dv5", SCM, "llr", None, "noclamp"), Case("i32", SCM, "keys", None, "noclamp"),
            Case("i64", MS, "keys", None, "noclamp"), Case("n13056", MS, "keys", None, "noclamp")]    # global store
    # min-sum: another scale, an offset
    for name, entry in [("i16", "llr"), ("i32", "keys"), ("i16g", "keys")]:
        out += [Case(name, MS, entry, None, "scale"), Case(name, MS, entry, None, "offset")]
    return out


CASES = _cases()
REFUSED = [(name, entry) for (name, rule, store), v in EXPECT.items() if v is None for entry in ("llr", "keys")]


def case_id(c):
    return "-".join([c.code, c.rule, c.entry, c.store or "default", c.par])


def call_args(c):
    """what the public entry is called with: QBER, then max_it, thr, thr_on and the variant's keywords"""
    p = PARS[c.par]
    q = Q_HIGH[c.code] if p.high else Q_MAIN[c.code]
    kw = dict(variant="sp_f32" if c.rule == SP else "minsum")
    if c.rule != SP:
        kw.update(minsum_scale=p.scale, minsum_offset=p.offset, minsum_self_correct=c.rule == SCM)
    return q, p, kw


def want_key(c):
    kind, rule, bucket, gt = EXPECT[(c.code, c.rule, c.store)]
    clamp = int(PARS[c.par].thr_on)
    mode = 1 if c.entry == "keys" else 0
    return dict(status=0, path=1 if kind == "split" else 0, rule=rule, bucket=bucket, gt=gt,
                decoder="%s:%d,%d,%d,%d,%d,0,0,0,0,0,0,0" % (kind, mode, rule, bucket, clamp, gt))


@functools.lru_cache(maxsize=None)
def minsum_want(name, rule, par, entry):
    """the min-sum model's (bits, iterations, ok) of a case, shared by its stores"""
    q, p, kw = call_args(Case(name, rule, entry, None, par))
    a, b, qq, llr, syn = inputs(name, q, par, entry)
    with np.errstate(invalid="ignore"):      # (inf - inf without the clamp, see DEG1)
        return model(name).decode(llr, syn, p.max_it, p.thr, p.thr_on, 0.8125 if p.scale is None else p.scale,
                                  p.offset or 0.0, self_correct=rule == SCM)


def decodes_and_iterates(it, ok):
    """the main cases' condition: the check phases' sums matter"""
    return ok.mean() >= 0.5 and (it[ok.astype(bool)] >= 3).any()


# ---- CPU: every case is on the kernel it is meant for -----------------------------------

@pytest.fixture(scope="module")
def choices(tmp_path_factory):
    import qkd_ldpc_amd as Q
    tmp = tmp_path_factory.mktemp("variant_kernels")
    binary = str(tmp / "launch_choice_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", binary, NATIVE])

    def line(name, entry, rule, store, par):
        p = PARS[par]
        flags = Q.decoder_flags(p.thr_on, "sp_f32" if rule == SP else "minsum", p.scale if rule != SP else None,
                                p.offset if rule != SP else None, rule == SCM)
        s = "mode=%d flags=%d n_frames=%d" % (entry == "keys", flags, FRAMES.get(name, 12))
        if entry == "keys":
            s += " first_table=auto tab2=auto"
        if store:
            s += " ms_%s=1" % store
        return s

    lines = collections.defaultdict(list)
    for c in CASES:
        lines[c.code].append(case_id(c) + " " + line(c.code, c.entry, c.rule, c.store, c.par))
    for name, entry in REFUSED:
        lines[name].append("refused-%s-%s " % (name, entry) + line(name, entry, SCM, None, "main"))
    res = {}
    for name, ls in lines.items():
        path = str(tmp / (name + ".code"))
        write_code(path, code(name))
        with open(path + ".cases", "w") as f:
            f.write("\n".join(ls) + "\n")
        res.update(parse(subprocess.check_output([binary, path, path + ".cases"], text=True)))
    return res


def test_codes_are_as_described():
    for name, (seed, dv, dc) in CODE_SPECS.items():
        n, m, off, idx = code(name)
        assert (np.bincount(idx, minlength=n) == dv).all() and (np.diff(off) == dc).all(), name
    assert max(CODE_SPECS["i32"][2]) == 32 and max(CODE_SPECS["i32l"][2]) == 32
    for name in ("i8", "dv5"):
        assert {1, 2, 8} <= set(CODE_SPECS[name][2])
    assert len(set(map(case_id, CASES))) == len(CASES)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_reaches_its_kernel(choices, c):
    got, want = choices[case_id(c)], want_key(c)
    assert {k: got.get(k) for k in want} == want


@pytest.mark.parametrize("name,entry", REFUSED)
def test_self_corrected_refused_choice(choices, name, entry):
    assert choices["refused-%s-%s" % (name, entry)] == {"status": UNSUPPORTED, "message": SC_TEXT}


def test_kernels_covered():
    """the instantiations no other module compares with a model: (kind, rule, bucket, gt)"""
    have = {EXPECT[(c.code, c.rule, c.store)] for c in CASES}
    need = [("classic", 1, b, 0) for b in (6, 16, 64)] + [("classic", 1, b, 1) for b in (16, 64)]
    need += [("classic", 2, b, 1) for b in (16, 64)] + [("classic", r, b, 0) for r in (3, 4) for b in (8, 16, 32)]
    need += [("classic", 2, 64, 0)] + [("split", r, 8, 0) for r in (1, 5, 6)] + [("split", 1, b, 0) for b in (16, 64)]
    assert not [k for k in need if k not in have]
    # every main kernel on both entries, with and without the clamp per family
    fam = {(EXPECT[(c.code, c.rule, c.store)][:2], EXPECT[(c.code, c.rule, c.store)][3]) for c in CASES
           if c.par == "noclamp"}
    assert {(("split", 1), 0), (("split", 5), 0), (("split", 6), 0), (("classic", 1), 0), (("classic", 1), 1),
            (("classic", 2), 1), (("classic", 3), 0), (("classic", 4), 0), (("classic", 2), 0)} <= fam


# (without the clamp a check of degree 1 sends scale * (+inf); the bit's next b2c on that
# edge is inf - inf, and a check of degree 2 that ignores the NaN sends +inf on: such
# frames are compared word for word but need not decode)
DEG1 = ("i8", "dv5")
MS_MAIN = sorted({(c.code, c.rule, c.par, c.entry) for c in CASES
                  if c.rule != SP and not PARS[c.par].high and (PARS[c.par].thr_on or c.code not in DEG1)})


@pytest.mark.parametrize("name,rule,par,entry", MS_MAIN)
def test_minsum_model_conditions(name, rule, par, entry):
    """the QBER of every min-sum case that should converge: the model decodes at least
    half of the frames, and one of them in three iterations or more"""
    bits, it, ok = minsum_want(name, rule, par, entry)
    assert decodes_and_iterates(it, ok), (it, ok)


@pytest.mark.parametrize("name,rule,entry", sorted({(c.code, c.rule, c.entry) for c in CASES
                                                    if c.rule != SP and c.par == "stuck"}))
def test_minsum_model_stuck(name, rule, entry):
    """... and of the cases that should not: most frames end at max_it"""
    bits, it, ok = minsum_want(name, rule, "stuck", entry)
    assert ok.mean() < 0.5 and (it[ok == 0] == PARS["stuck"].max_it).all()


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


@pytest.fixture(scope="module")
def sp_want(Q):
    """the sp_f32 specification with the device's elementwise steps, once per (code, parameters, entry)"""
    from test_variants import _dev_math

    @functools.lru_cache(maxsize=None)
    def get(name, par, entry):
        q, p, kw = call_args(Case(name, SP, entry, None, par))
        a, b, qq, llr, syn = inputs(name, q, par, entry)
        return sp_f32_decode(model(name), llr, syn, p.max_it, p.thr, p.thr_on,
                             tanh_half=_dev_math(2), two_atanh=_dev_math(3))
    return get


def _dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x).astype(dtype)).cuda()


def _decode(Q, H, c):
    """the case through its public entry -> the result and Alice's bits"""
    q, p, kw = call_args(c)
    a, b, qq, llr, syn = inputs(c.code, q, c.par, c.entry)
    if c.entry == "keys":
        r = Q.qkd_ldpc(H, _dev(a, np.uint8), _dev(b, np.uint8), float(qq), p.max_it, p.thr, p.thr_on,
                       want_bits=True, **kw)
    else:
        r = Q.sum_product_decoding(H, _dev(llr, np.float64), _dev(syn, np.uint8), p.max_it, p.thr, p.thr_on, **kw)
    torch.cuda.synchronize()
    return r, a


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_variant_kernel_bit_exact(Q, hmatrix, sp_want, qkd_opt, c):
    if c.store:
        qkd_opt("QKD_MINSUM_STORE", c.store)
    if c.rule == SP:
        wb, wi, wo = sp_want(c.code, c.par, c.entry)
        if c.par == "main":
            assert decodes_and_iterates(wi, wo), (wi, wo)
    else:
        wb, wi, wo = minsum_want(c.code, c.rule, c.par, c.entry)
    r, a = _decode(Q, hmatrix(c.code), c)
    assert (r.iterations.cpu().numpy() == wi).all()
    assert (r.syndromes_match.cpu().numpy() == wo).all()
    assert (r.bits.cpu().numpy() == wb).all()
    if c.entry == "keys":
        assert (r.keys_match.cpu().numpy() == (wb == a).all(axis=1)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name,entry", REFUSED)
def test_self_corrected_refused(Q, hmatrix, name, entry):
    """self-corrected min-sum where neither the split nor the LDS-state kernel takes the code"""
    with pytest.raises(Q.QkdError) as e:
        _decode(Q, hmatrix(name), Case(name, SCM, entry, None, "main"))
    assert e.value.status == UNSUPPORTED


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_sp_f64_trials_match_oracle(Q, hmatrix, oracle_mod, tmp_path, name):
    """The reference rule on the same small codes, fused trials against the oracle: the
    binary64 split kernel's generic bit phase (dv5) and its irregular buckets 8, 16, 64."""
    from conftest import write_alist
    H = hmatrix(name)
    n, m = code(name)[:2]
    cptr, cidx, bptr, bidx = H.adjacency()
    p = str(tmp_path / "code.alist")
    write_alist(p, n, m, bptr, bidx, cptr, cidx)
    oc = oracle_mod.Code.from_alist(p)
    seeds = oracle_mod.seeds(41, 16)
    q = Q_MAIN[name]
    r = Q.run_trials(H, torch.from_numpy(seeds.view(np.int64)).cuda(), q, 0, 30)
    torch.cuda.synchronize()
    want = oc.trials(q, seeds, 0, 30, 100.0, True)
    assert (r.iterations.cpu().numpy() == want["iters"]).all()
    assert (r.syndromes_match.cpu().numpy().astype(bool) == want["sp_ok"]).all()
    assert (r.keys_match.cpu().numpy().astype(bool) == want["key_ok"]).all()
    assert want["sp_ok"].mean() >= 0.5
