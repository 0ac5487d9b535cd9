"""The check-lane check phases (decode_split.hip spec_check_phase_lanes) on
codes whose checks are mostly SHORTER than their bucket: entries past a
check's degree carry the reserved dead slot word (qkd_decode.h kSlotDead),
which loads {+0, +0} and stores nowhere, and nothing else masks them. The
shapes here have what tests/test_check_lanes.py lacks: checks with one live
entry, odd numbers of dead entries, and (at the higher QBER and the low clamp,
where b2c cancel exactly) a dead entry beside an uncertified input.

Decoded words, iteration counts and both flags must be the oracle's under
every form (QKD_CHECK_LANES 1, 0, 2) and the forms must agree; the replays are
printed, not fixed.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FORMS = ["1", "0", "2"]


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import qkd_ldpc_amd as Q
    return Q


def make_code(m, degs, seed):
    """m checks of degrees degs[j % len(degs)] over ceil(E / 3) bits of degree
    <= 3 (the speculative kernel's limit), no bit twice in a check.
    (A copy of tests/test_check_lanes.py's.)"""
    rng = np.random.default_rng(seed)
    d = np.array([degs[j % len(degs)] for j in range(m)])
    e = int(d.sum())
    n = (e + 2) // 3
    sockets = rng.permutation(np.repeat(np.arange(n), 3))[:e].tolist()
    # (at most two sockets dropped: every bit keeps at least one)
    ptr = np.concatenate([[0], np.cumsum(d)])
    for _ in range(50):
        clean = True
        for j in range(m):
            row = sockets[ptr[j]:ptr[j + 1]]
            for k in range(len(row)):
                if row[k] in row[:k]:
                    clean = False
                    s = int(rng.integers(0, e))
                    sockets[ptr[j] + k], sockets[s] = sockets[s], sockets[ptr[j] + k]
                    row = sockets[ptr[j]:ptr[j + 1]]
        if clean:
            break
    assert clean
    idx = np.concatenate([np.sort(sockets[ptr[j]:ptr[j + 1]]) for j in range(m)])
    assert np.bincount(idx, minlength=n).min() >= 1 and np.bincount(idx, minlength=n).max() <= 3
    return n, ptr.astype(np.int32), idx.astype(np.int32)


# (name, checks, degrees, seed): bucket 6, a single partial task and one whole
# round of 16 check-lane tasks plus a 64-check remainder; bucket 4
SHAPES = {
    "b6_m96": (96, [1, 2, 3, 6], 11),
    "b6_m1088": (1088, [1, 2, 3, 6], 12),
    "b4_m80": (80, [1, 2, 4], 13),
}
# (qber, clamp): the two QBERs at clamp 100, and the low clamp once
RUNS = [(0.03, 100.0), (0.08, 100.0), (0.03, 2.5)]


@pytest.fixture(scope="module")
def codes(Q, oracle_mod):
    out = {}
    for name, (m, degs, seed) in SHAPES.items():
        n, ptr, idx = make_code(m, degs, seed)
        dense = np.zeros((m, n), np.uint8)
        for j in range(m):
            dense[j, idx[ptr[j]:ptr[j + 1]]] = 1
        out[name] = {"H": Q.HMatrix.from_check_lists(n, ptr, idx), "ref": oracle_mod.Code.from_dense(dense), "n": n}
    return out


def keys_frames(n, f, q, seed):
    rng = np.random.default_rng(seed)
    alice = rng.integers(0, 2, (f, n))
    bob = alice ^ (rng.random((f, n)) < q)
    return alice, bob


def lane_tasks_of(m, form):
    tasks = (m + 63) // 64
    return {"0": 0, "1": tasks // 16 * 16, "2": tasks}[form]


def run_keys(Q, H, alice, bob, q, max_it, thr, m, form):
    ws = Q.Workspace(H)
    Q.spec_replays(ws, reset=True)
    r = Q.qkd_ldpc(H, torch.from_numpy(alice.astype(np.uint8)).cuda(), torch.from_numpy(bob.astype(np.uint8)).cuda(),
                   q, max_it, thr, True, want_bits=True, workspace=ws)
    torch.cuda.synchronize()
    # the launch ran the form asked for
    got, lanes, edges = Q.check_lanes(ws)
    assert got == int(form) and lanes == lane_tasks_of(m, form), (form, got, lanes)
    assert (edges > 0) == (lanes * 64 < m), (form, lanes, edges)
    return (r.iterations.cpu().numpy(), r.syndromes_match.cpu().numpy().astype(bool),
            r.keys_match.cpu().numpy().astype(bool), r.bits.cpu().numpy(), Q.spec_replays(ws))


@pytest.mark.parametrize("q,thr", RUNS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_low_degree_checks(Q, codes, qkd_opt, name, q, thr):
    """32 frames, at most 50 iterations, speculation always on, every form."""
    c = codes[name]
    m = SHAPES[name][0]
    alice, bob = keys_frames(c["n"], 32, q, 300 + int(q * 100))
    w = [c["ref"].qkd_ldpc(alice[k], bob[k], q, 50, thr, True) for k in range(32)]
    want = (np.array([x["iters"] for x in w]), np.array([x["sp_ok"] for x in w]),
            np.array([x["key_ok"] for x in w]), np.stack([x["out"] for x in w]))
    qkd_opt("QKD_SPEC_POLICY", "always")
    got = {}
    for form in FORMS:
        qkd_opt("QKD_CHECK_LANES", form)
        got[form] = run_keys(Q, c["H"], alice, bob, q, 50, thr, m, form)
        its, sp, ko, bits, _ = got[form]
        assert (its == want[0]).all(), (name, q, thr, form, its, want[0])
        assert (sp == want[1]).all() and (ko == want[2]).all(), (name, q, thr, form)
        assert (bits == want[3]).all(), (name, q, thr, form)
    print(f"{name} q {q} thr {thr}: replays per form {[got[f][4] for f in FORMS]} of 32, "
          f"iterations {np.bincount(got['1'][0]).nonzero()[0].tolist()}")
    for form in FORMS[1:]:
        for a, b in zip(got["1"][:4], got[form][:4]):
            assert (a == b).all(), (name, q, thr, form)
