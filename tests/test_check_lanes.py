"""The speculative check phases one check per lane (decode_split.hip
spec_check_phase_lanes, the check-lane plan of qkd_plan.h) against the
edge-per-lane phases they replace and against the oracle.

QKD_CHECK_LANES chooses the form per launch: 1 (the default) whole rounds of
check-lane tasks plus an edge-lane remainder, 2 every check on a lane, 0 the
edge-lane phases. The forms sum a check's phi terms in different orders, so
their intervals differ in the last bits, but every form's intervals enclose
the reference's messages: decoded words, iteration counts and flags must be
the oracle's exactly under each form, and so is the counters record of the
fused trial path (only the number of frames replayed on the exact path may
differ, and is printed).
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
    <= 3 (the speculative kernel's limit), no bit twice in a check."""
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


# (name, checks, degrees): a single partial task; one whole round of 16 tasks
# plus a 32-check remainder; whole rounds exactly (bucket 4); bucket 6 mixing
# degrees 4, 5 and 6
SMALL = {
    "m48": (48, [6], 1),
    "m1056": (1056, [6, 5], 2),
    "m1024": (1024, [4], 3),
    "mixed456": (1500, [4, 5, 6, 6, 5], 4),
}


@pytest.fixture(scope="module")
def small_codes(Q, oracle_mod):
    """Per shape: the device code, the oracle's, and the oracle's results per
    (qber) computed once and shared by the forms."""
    out = {}
    for name, (m, degs, seed) in SMALL.items():
        n, ptr, idx = make_code(m, degs, seed)
        dense = np.zeros((m, n), np.uint8)
        for j in range(m):
            dense[j, idx[ptr[j]:ptr[j + 1]]] = 1
        out[name] = {"H": Q.HMatrix.from_check_lists(n, ptr, idx), "ref": oracle_mod.Code.from_dense(dense), "n": n,
                     "want": {}}
    return out


def keys_frames(n, f, q, seed):
    rng = np.random.default_rng(seed)
    alice = rng.integers(0, 2, (f, n))
    bob = alice ^ (rng.random((f, n)) < q)
    return alice, bob


def lane_tasks_of(m, form):
    """Tasks (64 checks each) that form `form` runs one check per lane for a
    code of m checks: whole rounds of 16 tasks (1), every task (2), none (0)."""
    tasks = (m + 63) // 64
    return {"0": 0, "1": tasks // 16 * 16, "2": tasks}[form]


def assert_form(Q, ws, m, form):
    """The launch ran the form asked for (the forms differ in time only, so
    nothing else tells a launch that fell back to the edge-lane plan)."""
    got, lanes, edges = Q.check_lanes(ws)
    assert got == int(form), (form, got)
    assert lanes == lane_tasks_of(m, form), (form, lanes)
    assert (edges > 0) == (lanes * 64 < m), (form, lanes, edges)


def run_keys(Q, H, alice, bob, q, max_it, thr, m, form):
    ws = Q.Workspace(H)
    assert Q.check_lanes(ws)[0] == -1
    Q.spec_replays(ws, reset=True)
    r = Q.qkd_ldpc(H, torch.from_numpy(alice.astype(np.uint8)).cuda(), torch.from_numpy(bob.astype(np.uint8)).cuda(),
                   q, max_it, thr, True, want_bits=True, workspace=ws)
    torch.cuda.synchronize()
    assert_form(Q, ws, m, form)
    return (r.iterations.cpu().numpy(), r.syndromes_match.cpu().numpy().astype(bool),
            r.keys_match.cpu().numpy().astype(bool), r.bits.cpu().numpy(), Q.spec_replays(ws))


def want_keys(ref, alice, bob, q, max_it, thr):
    w = [ref.qkd_ldpc(alice[k], bob[k], q, max_it, thr, True) for k in range(alice.shape[0])]
    return (np.array([x["iters"] for x in w]), np.array([x["sp_ok"] for x in w]), np.array([x["key_ok"] for x in w]),
            np.stack([x["out"] for x in w]))


def check_equal(got, want, what):
    its, sp, ko, bits, _ = got
    assert (its == want[0]).all(), (what, its, want[0])
    assert (sp == want[1]).all() and (ko == want[2]).all(), what
    assert (bits == want[3]).all(), what


@pytest.mark.parametrize("q", [0.03, 0.08])
@pytest.mark.parametrize("name", list(SMALL))
def test_small_codes_keys_path(Q, small_codes, qkd_opt, name, q):
    """32 frames through the keys path per shape and QBER, every form: the
    oracle's words, iterations and flags, and the forms agree."""
    c = small_codes[name]
    alice, bob = keys_frames(c["n"], 32, q, 100 + int(q * 100))
    if q not in c["want"]:
        c["want"][q] = want_keys(c["ref"], alice, bob, q, 50, 100.0)
    qkd_opt("QKD_SPEC_POLICY", "always")
    got = {}
    for form in FORMS:
        qkd_opt("QKD_CHECK_LANES", form)
        got[form] = run_keys(Q, c["H"], alice, bob, q, 50, 100.0, SMALL[name][0], form)
        check_equal(got[form], c["want"][q], (name, q, form))
    print(f"{name} q {q}: replays per form {[got[f][4] for f in FORMS]} of 32, "
          f"iterations {np.bincount(got['1'][0]).nonzero()[0].tolist()}")
    for form in FORMS[1:]:
        for a, b in zip(got["1"][:4], got[form][:4]):
            assert (a == b).all()


@pytest.fixture(scope="module")
def H(Q, golden_code):
    return Q.HMatrix.from_check_lists(int(golden_code["dims"][0]), golden_code["chk_off"], golden_code["chk_idx"])


@pytest.fixture(scope="module")
def golden_keys(oracle_code):
    """8 frames of the N = 10240 code at QBER 0.03 and the oracle's results by
    (max_it, threshold), computed on first use."""
    alice, bob = keys_frames(10240, 8, 0.03, 5)
    return {"alice": alice, "bob": bob, "want": {}}


@pytest.mark.parametrize("cap", ["2", None])
@pytest.mark.parametrize("max_it,thr", [(1, 100.0), (2, 100.0), (3, 100.0), (4, 100.0), (50, 2.5)])
def test_golden_keys_path(Q, H, oracle_code, golden_keys, qkd_opt, max_it, thr, cap):
    """max_it 1 to 4: the folded first iteration, the psi-input form and the
    b2c-interval form each end a decode; a threshold of 2.5 clamps most
    messages; QKD_SPEC_CAP 2 hands every longer frame to the exact path after
    the psi-input form."""
    g = golden_keys
    key = (max_it, thr)
    if key not in g["want"]:
        g["want"][key] = want_keys(oracle_code, g["alice"], g["bob"], 0.03, max_it, thr)
    qkd_opt("QKD_SPEC_CAP", cap)
    qkd_opt("QKD_SPEC_POLICY", "always")
    rep = []
    for form in ("1", "0"):
        qkd_opt("QKD_CHECK_LANES", form)
        got = run_keys(Q, H, g["alice"], g["bob"], 0.03, max_it, thr, 5231, form)
        check_equal(got, g["want"][key], (max_it, thr, cap, form))
        rep.append(got[4])
    print(f"max_it {max_it} thr {thr} cap {cap}: replays {rep} of 8, iterations {g['want'][key][0].tolist()}")


@pytest.fixture(scope="module")
def golden_llr(oracle_code):
    """24 LLR frames of the N = 10240 code (QBER 0.03, magnitudes spread), one
    with a NaN LLR and one with +-inf LLRs, and the oracle's results."""
    rng = np.random.default_rng(31)
    f, q = 24, 0.03
    alice = rng.integers(0, 2, (f, 10240))
    bob = alice ^ (rng.random((f, 10240)) < q)
    lp = np.log((1 - q) / q)
    llr = np.where(bob == 1, -lp, lp) * (1.0 + 0.25 * rng.random((f, 10240)))
    llr[3, 1234] = np.nan
    llr[7, 77] = np.inf * np.sign(llr[7, 77])
    llr[7, 9000] = -np.inf * np.sign(llr[7, 9000])      # one of the wrong sign
    syn = np.stack([oracle_code.syndrome(a) for a in alice]).astype(np.uint8)
    want = [oracle_code.decode(llr[k], syn[k], 50, 100.0, True) for k in range(f)]
    return llr, syn, want


def test_golden_llr_path(Q, H, golden_llr, qkd_opt):
    """The LLR path has no folded first iteration: every check phase is the
    b2c-interval form, from the LLRs' own intervals. A NaN or infinite LLR
    cannot be certified: the round aborts and the frame is decoded exactly."""
    llr, syn, want = golden_llr
    rep = []
    for form in ("1", "0"):
        qkd_opt("QKD_CHECK_LANES", form)
        ws = Q.Workspace(H)
        Q.spec_replays(ws, reset=True)
        r = Q.sum_product_decoding(H, torch.from_numpy(llr).cuda(), torch.from_numpy(syn).cuda(), 50, 100.0, True,
                                   workspace=ws)
        torch.cuda.synchronize()
        assert_form(Q, ws, 5231, form)
        bits, its, ok = r.bits.cpu().numpy(), r.iterations.cpu().numpy(), r.syndromes_match.cpu().numpy()
        for k in range(llr.shape[0]):
            assert its[k] == want[k]["iters"], (form, k, its[k], want[k]["iters"])
            assert bool(ok[k]) == want[k]["sp_ok"], (form, k)
            assert (bits[k] == want[k]["out"]).all(), (form, k)
        rep.append(Q.spec_replays(ws))
        # decoded alone: the NaN frame and the infinite-LLR frame are replayed
        # (their first check phase cannot certify the entry and aborts the
        # round), a clean frame is not; results the oracle's each time
        for k, want_rep in ((3, 1), (7, 1), (0, 0)):
            ws1 = Q.Workspace(H)
            Q.spec_replays(ws1, reset=True)
            r1 = Q.sum_product_decoding(H, torch.from_numpy(llr[k:k + 1]).cuda(), torch.from_numpy(syn[k:k + 1]).cuda(),
                                        50, 100.0, True, workspace=ws1)
            torch.cuda.synchronize()
            assert Q.spec_replays(ws1) == want_rep, (form, k)
            assert int(r1.iterations[0]) == want[k]["iters"] and bool(r1.syndromes_match[0]) == want[k]["sp_ok"]
            assert (r1.bits.cpu().numpy()[0] == want[k]["out"]).all(), (form, k)
    print(f"LLR path: replays per form {rep} of {llr.shape[0]}")
    assert rep[0] >= 2 and rep[1] >= 2


def counters_of(iters, sp, ko):
    """The qkd_counters record (include/qkd_ldpc.h) of per-frame results: frames,
    converged, converged with the right key, sum and sum of squares of the
    converged frames' iterations, their minimum and maximum."""
    it = iters[sp].astype(np.uint64)
    rec = np.zeros(48, np.uint8)
    rec[:40] = np.array([len(iters), sp.sum(), (sp & ko).sum(), it.sum(), (it * it).sum()], np.uint64).view(np.uint8)
    rec[40:48] = np.array([it.min() if it.size else 0xFFFFFFFF, it.max() if it.size else 0], np.uint32).view(np.uint8)
    return rec


@pytest.mark.parametrize("q", [0.02, 0.06])
def test_trial_counters(Q, H, oracle_code, qkd_opt, q):
    """The fused trial path (device keys, decode, counters) over 512 frames:
    per-frame results and the counters record are byte for byte the same under
    every form and equal the oracle's trials and the record they imply."""
    seeds_np = Q.make_seeds(4242, 512)
    seeds = torch.from_numpy(seeds_np.view(np.int64)).cuda()
    want = oracle_code.trials(q, seeds_np, 0, 50, 100.0, True, threads=8)
    want_rec = counters_of(want["iters"], want["sp_ok"], want["key_ok"]).tobytes()
    recs = {}
    for form in FORMS:
        qkd_opt("QKD_CHECK_LANES", form)
        ws = Q.Workspace(H)
        Q.spec_replays(ws, reset=True)
        r = Q.run_trials(H, seeds, q, 0, 50, 100.0, True, workspace=ws)
        torch.cuda.synchronize()
        assert_form(Q, ws, 5231, form)
        assert (r.iterations.cpu().numpy() == want["iters"]).all(), form
        assert (r.syndromes_match.cpu().numpy().astype(bool) == want["sp_ok"]).all(), form
        assert (r.keys_match.cpu().numpy().astype(bool) == want["key_ok"]).all(), form
        recs[form] = r.counters.cpu().numpy().tobytes()
        assert recs[form] == want_rec, (form, Q.read_counters(r.counters))
        print(f"q {q} form {form}: {Q.spec_replays(ws)} of 512 replayed")
    assert recs["1"] == recs["0"] == recs["2"]
