"""The code layout (csrc/qkd_layout.h) on the CPU, through a g++ build of the
header (tests/native/code_layout_check.cpp): every array build_code uploads or
keeps, (a) byte for byte what the commit before the layout / upload split
uploaded and kept (tests/golden/code_layout_parent.json, recorded from that
commit's build_code run against a stand-in HIP runtime whose host-to-device
copy logs its bytes), (b) against a numpy restatement from the adjacency."""
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

K_DECODE_BLOCK = 1024
K_BIT_PAD_ROUNDS = 4
K_MAX_BITS_SPLIT_LONG = 128 * K_DECODE_BLOCK
PLAN_BIT_MASK = 0xFFFFFF
PLAN_PAD_TASKS = 128

DTYPES = {
    "check_ptr": "<i4", "check_idx": "<i4", "bit_ptr": "<i4", "bit_idx": "<i4", "chk_bits": "<i4", "chk_deg": "u1",
    "chk_odd": "<u4", "bit_chk": "<i4", "bit_pos": "u1", "bit_deg": "u1", "bit_pat": "<u2", "pat_deg": "u1",
    "plan": "<u4", "perm": "<i4", "inv": "<i4", "bit_chk_s": "<i4", "bit_deg_s": "u1", "bit_pat_s": "<u2",
    "chk_rows16": "<u2", "bit_code": "<u8", "ilv_slots": "<u4", "plan_slot": "<u4", "jump": "<u8", "jpoly": "<u8",
    "jpoly2": "<u8", "cl0_slot": "<u4", "cl0_chk": "<u4", "cl0_rem": "<u4", "cl1_slot": "<u4", "cl1_chk": "<u4",
    "cl1_rem": "<u4",
}


def _socket_code(seed, dv, dc):
    """A seeded random code with bit degrees dv[i] and check degrees dc[j]
    (equal sums): shuffled sockets dealt to the checks, duplicates inside a
    check swapped away. RandomState: its stream is frozen across numpy versions."""
    rs = np.random.RandomState(seed)
    dv, dc = np.asarray(dv), np.asarray(dc)
    assert dv.sum() == dc.sum()
    sock = np.repeat(np.arange(len(dv), dtype=np.int32), dv)
    rs.shuffle(sock)
    chk = np.repeat(np.arange(len(dc)), dc)
    while True:
        sock = sock[np.lexsort((sock, chk))]
        dup = np.nonzero((sock[1:] == sock[:-1]) & (chk[1:] == chk[:-1]))[0] + 1
        if len(dup) == 0:
            break
        for p in dup:
            q = rs.randint(len(sock))
            sock[p], sock[q] = sock[q], sock[p]
    off = np.concatenate([[0], np.cumsum(dc)]).astype(np.int32)
    return len(dv), len(dc), off, sock.astype(np.int32)


def _dense_code(dense):
    m, n = dense.shape
    rows = [np.nonzero(r)[0] for r in dense]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return n, m, off, np.concatenate(rows).astype(np.int32)


def codes():
    """name -> (n, m, check_ptr, check_idx): the cases of the layout's paths."""
    out = {}
    g = np.load(os.path.join(GOLDEN, "code_n10240.npz"))
    out["golden_n10240"] = (int(g["dims"][0]), len(g["chk_off"]) - 1, g["chk_off"].astype(np.int32),
                            g["chk_idx"].astype(np.int32))
    with open(os.path.join(GOLDEN, "dense_codes.json")) as f:
        for name, rows in sorted(json.load(f).items()):
            out["dense_" + name] = _dense_code(np.array(rows, np.uint8))
    # a bit of degree 4: no packed words, no check-lane plan, no interleaved lines
    out["bit_degree_4"] = _socket_code(11, [3] * 599 + [4] + [3] * 401, [6] * 500 + [1] + [3])
    # a check of degree 17: no sliced rows (and no packed words)
    out["check_degree_17"] = _socket_code(12, [3] * 700, [6] * 347 + [17] + [1])
    # check degrees <= 4, more than one round of check-lane tasks and a remainder: bucket 4
    out["check_lanes_4"] = _socket_code(13, [3] * 1400 + [2] * 100, [4] * 1000 + [3] * 132 + [2] * 2)
    # N just past kMaxBitsSplitLong: no split view at all
    nl = K_MAX_BITS_SPLIT_LONG + 1
    out["past_split_long"] = _socket_code(14, [2] * nl, [8] * (2 * nl // 8) + [2 * nl % 8])
    return out


def write_code(path, code):
    n, m, off, idx = code
    with open(path, "wb") as f:
        np.array([n, m, len(idx)], "<i4").tofile(f)
        np.asarray(off, "<i4").tofile(f)
        np.asarray(idx, "<i4").tofile(f)


def parse_report(text):
    """status, message, scalars, {name: (kind, bytes, hash)} of a layout report"""
    lines = text.splitlines()
    head = lines[0].split(" ", 2)
    scal, arrs = {}, {}
    for ln in lines[1:]:
        t = ln.split()
        if t[0] == "s":
            scal[t[1]] = int(t[2])
        elif t[0] == "a":
            arrs[t[1]] = (t[2], int(t[3]), t[4])
    return int(head[1]), head[2] if len(head) > 2 else "", scal, arrs


@pytest.fixture(scope="module")
def layout_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("native") / "code_layout_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", out,
                           os.path.join(HERE, "native", "code_layout_check.cpp")])
    return out


@pytest.fixture(scope="module")
def all_codes():
    return codes()


@pytest.fixture(scope="module")
def layouts(layout_bin, all_codes, tmp_path_factory):
    """name -> (scalars, arrays' (kind, bytes, hash), arrays): derived once, shared"""
    out = {}
    for name, code in all_codes.items():
        d = tmp_path_factory.mktemp("layout")
        path = str(d / "code.bin")
        write_code(path, code)
        st, msg, scal, arrs = parse_report(subprocess.check_output([layout_bin, path, "-", str(d)], text=True))
        assert st == 0, (name, st, msg)
        data = {k: np.fromfile(str(d / (k + ".bin")), DTYPES[k]) for k in arrs}
        out[name] = (scal, arrs, data)
    return out


CODE_NAMES = ["golden_n10240", "dense_(N=10,K=5,M=5,R=0.5).txt", "dense_(N=6,K=2,M=4,R=0.34).txt",
              "dense_(N=7,K=4,M=3,R=0.57).txt", "bit_degree_4", "check_degree_17", "check_lanes_4", "past_split_long"]


def test_code_names(all_codes):
    assert sorted(all_codes) == sorted(CODE_NAMES)


@pytest.mark.parametrize("name", CODE_NAMES)
def test_layout_equals_parent_commit(layouts, name):
    with open(os.path.join(GOLDEN, "code_layout_parent.json")) as f:
        want = json.load(f)[name]
    scal, arrs, _ = layouts[name]
    uploaded = sorted([b, h] for kind, b, h in arrs.values() if "d" in kind and b > 0)
    assert uploaded == sorted(want["uploaded"])
    for key, (b, h) in want["host"].items():
        assert arrs[key][0].endswith("h") and list(arrs[key][1:]) == [b, h], key
    for key, v in want["scalars"].items():
        assert scal[key] == v, key


def _restate(code):
    n, m, off, idx = code
    dc = np.diff(off)
    chk = np.repeat(np.arange(m), dc)
    order = np.argsort(idx, kind="stable")            # edges by bit, checks ascending
    dv = np.bincount(idx, minlength=n)
    bptr = np.concatenate([[0], np.cumsum(dv)])
    krow = np.empty(len(idx), np.int64)
    krow[order] = np.arange(len(idx)) - bptr[idx[order]]
    return dc, dv, chk, krow, order, bptr


@pytest.mark.parametrize("name", CODE_NAMES)
def test_layout_equals_restatement(layouts, all_codes, name):
    n, m, off, idx = all_codes[name]
    scal, arrs, A = layouts[name]
    dc, dv, chk, krow, order, bptr = _restate(all_codes[name])
    e = len(idx)
    n_pad, m_pad = (n + 1 + 63) // 64 * 64, (m + 63) // 64 * 64
    max_dv, max_dc = int(dv.max()), int(dc.max())
    assert (scal["n"], scal["m"], scal["e"], scal["n_pad"], scal["m_pad"]) == (n, m, e, n_pad, m_pad)
    assert (scal["max_dv"], scal["min_dv"], scal["max_dc"], scal["min_dc"]) == (max_dv, dv.min(), max_dc, dc.min())
    assert scal["is_regular"] == int(dv.min() == max_dv and dc.min() == max_dc)
    slot = np.arange(e) - off[chk]                    # position of the edge in its check
    # the adjacency and the ELL arrays
    assert (A["check_ptr"] == off).all() and (A["check_idx"] == idx).all()
    assert (A["bit_ptr"] == bptr).all() and (A["bit_idx"] == chk[order]).all()
    chk_bits = np.full(max_dc * m_pad, -1)
    chk_bits[slot * m_pad + chk] = idx
    bit_chk = np.full(max_dv * n_pad, -1)
    bit_chk[krow * n_pad + idx] = chk
    bit_pos = np.zeros(max_dv * n_pad, np.int64)
    bit_pos[krow * n_pad + idx] = slot
    assert (A["chk_bits"] == chk_bits).all() and (A["bit_chk"] == bit_chk).all() and (A["bit_pos"] == bit_pos).all()
    assert (A["chk_deg"] == dc).all() and (A["bit_deg"] == dv).all()
    # chk_odd: the degree parity, one bit per check, whole 64-check words
    odd = np.zeros((m + 63) // 64 * 64, np.uint8)
    odd[:m] = dc & 1
    assert (np.unpackbits(A["chk_odd"].view(np.uint8), bitorder="little") == odd).all()
    # degree patterns: pat_deg[bit_pat[i]] = the degrees of bit i's checks
    if scal["n_pat"] > 0:
        pd = A["pat_deg"].reshape(scal["n_pat"], max_dv)
        want = np.zeros((n, max_dv), np.int64)
        want[idx, krow] = dc[chk]
        assert (pd[A["bit_pat"]] == want).all()
        assert len(np.unique(pd, axis=0)) == scal["n_pat"]
    else:
        assert len(A["bit_pat"]) == 0 and len(A["pat_deg"]) == 0
    # the wave plan: every edge on exactly one lane, {bit | row << 24, check | start << 20 | (deg - 1) << 26}
    plan = A["plan"].reshape(-1, 2)
    tasks = scal["n_tasks"]
    assert len(plan) == (tasks + PLAN_PAD_TASKS) * 64
    pb, prow, pchk = plan[:, 0] & PLAN_BIT_MASK, plan[:, 0] >> 24, plan[:, 1] & 0xFFFFF
    live = pb < n
    assert not live[tasks * 64:].any() and (pb[~live] == n).all()
    got = sorted(zip(pchk[live].tolist(), pb[live].tolist(), prow[live].tolist()))
    assert got == sorted(zip(chk.tolist(), idx.tolist(), krow.tolist()))
    assert ((plan[live, 1] >> 26) + 1 == dc[pchk[live]]).all()

    split = n <= K_MAX_BITS_SPLIT_LONG and m <= 65536
    assert scal["split"] == int(split)
    if not split:
        for k in ("perm", "inv", "bit_chk_s", "bit_deg_s", "bit_pat_s", "chk_rows16", "bit_code", "ilv_slots",
                  "plan_slot", "cl0_slot", "cl1_slot"):
            assert len(A[k]) == 0, k
        assert scal["cl_dc"] == 0
        return
    perm, inv = A["perm"], A["inv"]
    assert (np.sort(perm) == np.arange(n)).all() and (inv[perm] == np.arange(n)).all()
    bcs = np.full(max_dv * n_pad, -1)
    for k in range(max_dv):
        bcs[k * n_pad:k * n_pad + n] = bit_chk[k * n_pad + perm]
    assert (A["bit_chk_s"] == bcs).all() and (A["bit_deg_s"] == dv[perm]).all()
    if scal["n_pat"] > 0:
        bps = np.zeros((n + K_DECODE_BLOCK - 1) // K_DECODE_BLOCK * K_DECODE_BLOCK + K_BIT_PAD_ROUNDS * K_DECODE_BLOCK,
                       np.int64)
        bps[:n] = A["bit_pat"][perm]
        assert (A["bit_pat_s"] == bps).all()
    else:
        assert len(A["bit_pat_s"]) == 0
    # plan_slot: plan re-addressed by message slot
    ps = A["plan_slot"].reshape(-1, 2)
    assert (ps[:, 1] == plan[:, 1]).all()
    assert (ps[:, 0] == prow * n_pad + np.where(live, inv[np.minimum(pb, n - 1)], pb)).all()
    # the sliced syndrome rows
    if n < 65535 and max_dc <= 16:
        rs = 8 if max_dc <= 8 else 16
        rows = np.full((m, rs), 0xFFFF)
        rows[chk, slot] = idx
        assert scal["chk_rs"] == rs and (A["chk_rows16"].reshape(m, rs) == rows).all()
    else:
        assert scal["chk_rs"] == 0 and len(A["chk_rows16"]) == 0
    # the packed per-bit words and the interleaved decoder's lines
    packable = m <= 65536 and max_dv <= 3 and dc.min() >= 1 and max_dc <= 16
    if packable:
        code = A["bit_code"]
        assert len(code) == max(n_pad, (n + K_DECODE_BLOCK - 1) // K_DECODE_BLOCK * K_DECODE_BLOCK) + \
            K_BIT_PAD_ROUNDS * K_DECODE_BLOCK
        assert (code[n:] == 0).all()
        w = code[:n]
        deg = ((w >> np.uint64(48)) & np.uint64(3)).astype(np.int64)
        assert (deg == dv[perm]).all() and (w >> np.uint64(62) == 0).all()
        for k in range(3):
            j = ((w >> np.uint64(16 * k)) & np.uint64(0xFFFF)).astype(np.int64)
            d1 = ((w >> np.uint64(50 + 4 * k)) & np.uint64(15)).astype(np.int64)
            has = deg > k
            want_j = bit_chk[k * n_pad + perm] if k < max_dv else np.full(n, -1)
            assert (j[has] == want_j[has]).all() and (d1[has] == dc[want_j[has]] - 1).all()
            assert (j[~has] == 0).all() and (d1[~has] == 0).all()
        rs = 8 if max_dc <= 8 else 16
        lines = np.full((m, rs), 0xFFFFFFFF)
        lines[chk, slot] = krow * n_pad + inv[idx]
        assert scal["ilv_rs"] == rs and (A["ilv_slots"].reshape(m, rs) == lines).all()
    else:
        assert len(A["bit_code"]) == 0 and len(A["ilv_slots"]) == 0 and scal["ilv_rs"] == 0
    # the check-lane plans: every edge's slot once, in the check-lane part or the remainder
    if packable and max_dc <= 6:
        cdc = 4 if max_dc <= 4 else 6
        assert scal["cl_dc"] == cdc
        edge_slots = np.sort(krow * n_pad + inv[idx])
        for form in (0, 1):
            cs, rem = A[f"cl{form}_slot"], A[f"cl{form}_rem"].reshape(-1, 2)
            t = scal[f"cl{form}_tasks"]
            assert t == ((m // 1024 * 1024 if form == 0 else m) + 63) // 64
            assert len(cs) == (t + PLAN_PAD_TASKS) * cdc * 64 and len(A[f"cl{form}_chk"]) == (t + PLAN_PAD_TASKS) * 64
            rlive = rem[:scal[f"cl{form}_rem_tasks"] * 64, 0]
            rlive = rlive[rlive % n_pad != n]
            assert (np.sort(np.concatenate([cs[cs != 0xFFFFFFFF], rlive])) == edge_slots).all()
    else:
        assert scal["cl_dc"] == 0 and len(A["cl0_slot"]) == 0 and len(A["cl1_slot"]) == 0


def test_case_paths(layouts):
    """each special code takes the path it was made for"""
    s = {k: v[0] for k, v in layouts.items()}
    a = {k: v[1] for k, v in layouts.items()}
    assert s["golden_n10240"]["cl_dc"] == 6 and a["golden_n10240"]["ilv_slots"][1] > 0
    assert s["bit_degree_4"]["max_dv"] == 4
    assert [a["bit_degree_4"][k][1] for k in ("bit_code", "ilv_slots", "cl0_slot")] == [0, 0, 0]
    assert s["check_degree_17"]["max_dc"] == 17 and a["check_degree_17"]["chk_rows16"][1] == 0
    assert s["check_lanes_4"]["cl_dc"] == 4 and s["check_lanes_4"]["cl0_tasks"] == 16
    assert s["check_lanes_4"]["cl0_rem_tasks"] > 0
    assert s["past_split_long"]["n"] == K_MAX_BITS_SPLIT_LONG + 1 and s["past_split_long"]["split"] == 0
    assert a["past_split_long"]["perm"][1] == 0


@pytest.mark.parametrize("case,status,text", [
    ("degree_65", 8, "check degree 65 exceeds 64"),
    ("unsorted", 3, "check 1: bit list not strictly ascending at slot 1 (2 after 5)"),
    ("duplicate", 2, "check 0: bit list not strictly ascending at slot 2 (4 after 4)"),
])
def test_limit_errors(layout_bin, tmp_path, case, status, text):
    code = {
        "degree_65": (100, 2, [0, 65, 66], list(range(65)) + [99]),
        "unsorted": (8, 2, [0, 2, 4], [0, 1, 5, 2]),
        "duplicate": (8, 1, [0, 3], [1, 4, 4]),
    }[case]
    path = str(tmp_path / "code.bin")
    write_code(path, code)
    st, msg, scal, arrs = parse_report(subprocess.check_output([layout_bin, path], text=True))
    assert (st, msg) == (status, text) and not arrs
