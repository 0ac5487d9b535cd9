"""Blind reconciliation on the GPU (qkd_reconcile_blind_batch / reconcile_blind): class
bytes with revealed punctured bits, the per-round frame list in both decoder kernels and
the round bookkeeping, against the round loop of tests/blind_model.py on the numpy model
of tests/adapt_model.py (pinned to the oracle by tests/test_adapt_abi.py), the LLR entry
and reconcile_adaptive, all by exact equality. Inputs, seeds and QBERs were chosen on the
CPU with the model; each test asserts on the model's own record that it exercises what it
is for. The golden cases draw payload, fill, then noise from default_rng(400); their plan
punctures the first p positions of adapt_positions(seed 5)."""
import numpy as np
import pytest

from tests import adapt_model as AM
from tests import blind_model as BM

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_GOLD, M_GOLD = 10240, 5231
GUARD = 0xA5
STEP = 256


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import qkd_ldpc_amd as Q
    return Q


@pytest.fixture(scope="module")
def H(Q, golden_code):
    return Q.HMatrix.from_check_lists(int(golden_code["dims"][0]), golden_code["chk_off"],
                                      golden_code["chk_idx"])


@pytest.fixture(scope="module")
def G(golden_code):
    return AM.Graph(int(golden_code["dims"][0]), golden_code["chk_off"], golden_code["chk_idx"])


def dev(x, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(x).astype(dtype)).cuda()


class Case:
    """f frames of a code for the plan (punctured, shortened): Alice's payload and fill,
    her frames and their syndromes (embedded on the host), Bob's payload at QBER q."""

    def __init__(self, g, punctured, shortened, seed, q, f):
        self.g, self.q, self.f = g, q, f
        self.pu = np.asarray(punctured, np.int64)
        self.sh = np.asarray(shortened, np.int64)
        self.p = self.pu.size
        self.pay = np.setdiff1d(np.arange(g.n), np.concatenate([self.pu, self.sh]))
        rng = np.random.default_rng(seed)
        self.payload = rng.integers(0, 2, (f, self.pay.size)).astype(np.uint8)
        self.fill = rng.integers(0, 2, (f, self.p)).astype(np.uint8)
        self.bob = self.payload ^ (rng.random((f, self.pay.size)) < q).astype(np.uint8)
        self.frames = np.zeros((f, g.n), np.uint8)
        self.frames[:, self.pay] = self.payload
        self.frames[:, self.pu] = self.fill
        self.syn = np.stack([g.syndrome(x) for x in self.frames])

    def loop(self, libm, k, n_revealed=0, step=STEP, max_rounds=6, revealed=None):
        return BM.blind_loop(self.g, self.pu, self.sh, self.bob[k], self.syn[k], self.q, libm,
                             self.fill[k] if revealed is None else revealed, n_revealed, step, max_rounds)

    def known_only(self, counts):
        """Alice's fill as Bob holds it: past each frame's count, bytes he does not have."""
        out = np.full((self.f, self.p), GUARD, np.uint8)
        for k, c in enumerate(counts):
            out[k, :c] = self.fill[k, :c]
        return out


def result(r, sync=True):
    """A BlindResult on the host: a dict of numpy arrays."""
    if sync:
        torch.cuda.synchronize()
    out = {"iters": r.iterations, "ok": r.syndromes_match, "payload": r.bits, "corrected": r.corrected,
           "frames": r.frames, "rounds": r.rounds, "n_revealed": r.n_revealed, "leak_bits": r.leak_bits}
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def of_loops(loops):
    """What a call must return for frames whose model loops are `loops`."""
    return {"iters": np.array([m["last"]["iters"] for m in loops]),
            "ok": np.array([m["last"]["sp_ok"] for m in loops], np.uint8),
            "payload": np.stack([m["payload"] for m in loops]),
            "corrected": np.array([m["corrected"] for m in loops]),
            "frames": np.stack([m["last"]["out"] for m in loops]),
            "rounds": np.array([m["rounds"] for m in loops]),
            "n_revealed": np.array([m["n_revealed"] for m in loops]),
            "leak_bits": np.array([m["leak_bits"] for m in loops])}


def assert_equal(got, want, rows=None):
    assert set(got) == set(want)
    for key in want:
        g, w = got[key], want[key]
        if rows is not None:
            g, w = g[rows], w[rows]
        assert g.shape == w.shape and (g == w).all(), (key, g, w)


def blind(Q, H, plan, case, revealed=None, **kw):
    kw.setdefault("want_frames", True)
    return result(Q.reconcile_blind(H, plan, dev(case.bob), dev(case.syn), case.q,
                                    dev(case.fill if revealed is None else revealed), **kw))


@pytest.fixture(scope="module")
def plan1024(Q, H):
    plan = Q.AdaptPlan.choose(H, 1024, 1024, 5)
    yield plan
    plan.close()


@pytest.fixture(scope="module")
def multi(G, plan1024, oracle_mod):
    """The two multi-round calls (QBER 0.08 and 0.07, 3 frames each, p = 1024, step 256,
    6 rounds) and their model loops, computed once for every test that uses them."""
    out = {}
    for q in (0.08, 0.07):
        case = Case(G, plan1024.punctured, [], 400, q, 3)
        out[q] = (case, [case.loop(oracle_mod.libm, k) for k in range(3)])
    return out


def assert_multi_preconditions(multi):
    hi, lo = multi[0.08][1], multi[0.07][1]
    assert [m["rounds"] for m in hi] == [2, 4, 3] and [m["n_revealed"] for m in hi] == [256, 768, 512]
    assert [m["rounds"] for m in lo] == [1, 2, 2] and [m["n_revealed"] for m in lo] == [0, 256, 256]
    for case, loops in multi.values():
        assert all(m["last"]["sp_ok"] for m in loops)
        assert not any(r["nan"] for m in loops for r in m["all"])
        assert all(r["iters"] == 50 and not r["sp_ok"] for m in loops for r in m["all"][:-1])
        assert all((m["payload"] == case.payload[k]).all() for k, m in enumerate(loops))


# ---- 1. zero reveals: reconcile_adaptive, output for output ------------------------------

def test_zero_reveals(Q, H, plan1024, multi):
    case = multi[0.07][0]
    d_bob, d_syn = dev(case.bob), dev(case.syn)
    a = Q.reconcile_adaptive(H, plan1024, d_bob, d_syn, case.q, want_frames=True)
    # (Bob holds none of Alice's fill: every byte of `revealed` is one he does not have)
    b = Q.reconcile_blind(H, plan1024, d_bob, d_syn, case.q, dev(case.known_only([0, 0, 0])), want_frames=True)
    torch.cuda.synchronize()
    for name in ("iterations", "syndromes_match", "bits", "corrected", "frames"):
        x, y = getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()
        assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), name
    assert not a.syndromes_match.cpu().numpy().all()             # (a frame that fails is among them)
    assert b.rounds.cpu().tolist() == [1, 1, 1]
    assert b.n_revealed.cpu().tolist() == [0, 0, 0]
    assert b.leak_bits.cpu().tolist() == [M_GOLD - 1024] * 3


# ---- 2. one round against its definition -----------------------------------------------------

def test_one_round(Q, H, G, plan1024, oracle_mod, multi):
    case = multi[0.07][0]
    counts = [0, 256, 1024]
    loops = [case.loop(oracle_mod.libm, k, counts[k], 0, 1) for k in range(3)]
    recs = [m["last"] for m in loops]
    assert not any(r["nan"] for r in recs)
    assert all(sum(r["z1"][1:]) > 0 for r in recs[:2])           # zeros survive the first iteration
    assert sum(recs[2]["z1"]) + sum(recs[2]["z2"]) == 0          # none in the fully revealed frame
    assert [m["rounds"] for m in loops] == [1, 1, 1] and [m["n_revealed"] for m in loops] == counts
    # only byte & 1 counts (0xFF is a 1, 0xFE a 0); past a frame's count, bytes Bob does
    # not have: a read there would make the class 5
    revealed = case.known_only(counts)
    for k, c in enumerate(counts):
        revealed[k, :c] |= 0xFE
    got = blind(Q, H, plan1024, case, revealed, n_revealed=dev(counts, np.int32))
    assert_equal(got, of_loops(loops))
    llr = np.stack([BM.frame_llrs(G.n, case.pu, [], case.bob[k], case.q, 100.0, case.fill[k], counts[k])[0]
                    for k in range(3)])
    assert (np.count_nonzero(llr == 0.0, axis=1) == [1024, 768, 0]).all()
    sp = Q.sum_product_decoding(H, dev(llr, np.float64), dev(case.syn), erasures=True)
    torch.cuda.synchronize()
    assert (sp.iterations.cpu().numpy() == got["iters"]).all()
    assert (sp.syndromes_match.cpu().numpy() == got["ok"]).all()
    assert (sp.bits.cpu().numpy() == got["frames"]).all()


# ---- 3. several rounds on the device -----------------------------------------------------------

@pytest.mark.parametrize("kernel", [None, "classic"])
def test_multi_round(Q, H, plan1024, multi, qkd_opt, kernel):
    """Both calls on the split kernel and on the classic one (class bytes, payload map and
    ranks in the original bit order; the frame list in its claim)."""
    assert_multi_preconditions(multi)
    qkd_opt("QKD_DECODE_KERNEL", kernel)
    for q in (0.08, 0.07):
        case, loops = multi[q]
        got = blind(Q, H, plan1024, case, step=STEP, max_rounds=6)
        assert_equal(got, of_loops(loops))
        assert (got["payload"] == case.payload).all()            # Bob ends with Alice's payload
        assert (got["leak_bits"] == M_GOLD - 1024 + got["n_revealed"]).all()


def test_exhaustion(Q, H, G, oracle_mod):
    """QBER 0.12, p = 512: both frames fail at 0, 256 and 512 revealed bits and are not
    decoded a fourth time, whatever max_rounds allows."""
    plan = Q.AdaptPlan.choose(H, 512, 512, 5)
    case = Case(G, plan.punctured, [], 400, 0.12, 2)
    loops = [case.loop(oracle_mod.libm, k) for k in range(2)]
    assert all(len(m["all"]) == 3 and not any(r["sp_ok"] for r in m["all"]) for m in loops)
    assert not any(r["nan"] for m in loops for r in m["all"])
    # the third decode differs from the second: the outputs show which one was last
    assert all((m["all"][2]["out"] != m["all"][1]["out"]).any() for m in loops)
    got = blind(Q, H, plan, case, step=STEP, max_rounds=6)
    assert got["rounds"].tolist() == [3, 3] and got["n_revealed"].tolist() == [512, 512]
    assert got["ok"].tolist() == [0, 0] and got["iters"].tolist() == [50, 50]
    assert_equal(got, of_loops(loops))
    # counts past p on entry count as p, and are returned as p
    over = blind(Q, H, plan, case, n_revealed=dev([513, 2**31 - 1], np.int32), step=STEP, max_rounds=6)
    assert over["rounds"].tolist() == [1, 1] and over["n_revealed"].tolist() == [512, 512]
    for key in ("iters", "ok", "payload", "corrected", "frames"):
        assert (over[key] == got[key]).all(), key
    plan.close()


# ---- 4. skipped frames -------------------------------------------------------------------------

def raw_call(Q, H, plan, case, bufs, nrev, skip, step, max_rounds):
    """The C entry on the caller's own output buffers."""
    N = Q._native
    d = [dev(case.bob), dev(case.syn), dev(case.fill)]
    st = N.lib().qkd_reconcile_blind_batch(
        H.handle, None, plan.handle, d[0].data_ptr(), d[1].data_ptr(), case.f, case.q, 100.0, 50, 100.0,
        N.FLAG_THRESHOLD, d[2].data_ptr(), nrev.data_ptr(), None if skip is None else skip.data_ptr(), step,
        max_rounds, bufs["payload"].data_ptr(), bufs["frames"].data_ptr(), bufs["iters"].data_ptr(),
        bufs["ok"].data_ptr(), bufs["corrected"].data_ptr(), bufs["rounds"].data_ptr(),
        int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st


def guard_buffers(case):
    f = case.f
    shapes = {"payload": (f, case.pay.size, torch.uint8), "frames": (f, case.g.n, torch.uint8),
              "iters": (f, 1, torch.int32), "ok": (f, 1, torch.uint8), "corrected": (f, 1, torch.int32),
              "rounds": (f, 1, torch.int32)}
    bufs = {}
    for k, (a, b, dt) in shapes.items():
        t = torch.empty((a, b), dtype=dt, device="cuda")
        t.view(torch.uint8).fill_(GUARD)
        bufs[k] = t
    return bufs


def test_skip(Q, H, G, plan1024):
    f = 33
    case = Case(G, plan1024.punctured, [], 401, 0.075, f)
    skip = np.zeros(f, np.uint8)
    skip[[0, 3, 4, 11, 17, 18, 19, 32]] = [1, 2, 0xFF, 1, 0x80, 1, 1, 1]      # nonzero = skipped
    keep = skip == 0
    start = (np.arange(f) % 3) * 100
    full, part, none = guard_buffers(case), guard_buffers(case), guard_buffers(case)
    n_full, n_part, n_none = (dev(start, np.int32) for _ in range(3))
    assert raw_call(Q, H, plan1024, case, full, n_full, None, STEP, 6) == 0
    assert raw_call(Q, H, plan1024, case, part, n_part, dev(skip), STEP, 6) == 0
    assert raw_call(Q, H, plan1024, case, none, n_none, dev(np.ones(f, np.uint8)), STEP, 6) == 0
    rounds = full["rounds"].cpu().numpy()[:, 0]
    assert len(set(rounds[keep].tolist())) >= 3 and len(set(rounds[~keep].tolist())) >= 2     # a mixed batch
    guard32 = int.from_bytes(bytes([GUARD] * 4), "little", signed=True)
    for key in full:
        a, b, c = (x[key].cpu().numpy() for x in (full, part, none))
        g = GUARD if a.dtype == np.uint8 else guard32
        assert (b[keep] == a[keep]).all(), key                   # the others: the unskipped call's
        assert (b[~keep] == g).all(), key                        # skipped: the guard bytes
        assert (c == g).all(), key                               # all skipped: nothing written
        assert not (a == g).all(axis=1).any(), key               # (a written row never looks like one)
    a, b, c = (x.cpu().numpy() for x in (n_full, n_part, n_none))
    assert (b[keep] == a[keep]).all() and (b[~keep] == start[~keep]).all() and (c == start).all()
    assert (a >= start).all() and (a > start).any() and (a <= 1024).all()


# ---- 5. the real-link form ------------------------------------------------------------------------

def test_real_link(Q, H, plan1024, multi):
    """Bob's loop on a link: one round a call, with what he holds; then he asks Alice for
    256 more bits of each frame that failed and skips the frames that are done. The same
    final outputs as the one call that runs the rounds on the device."""
    assert_multi_preconditions(multi)
    case, loops = multi[0.08]
    want = blind(Q, H, plan1024, case, step=STEP, max_rounds=6)
    assert_equal(want, of_loops(loops))
    keys = ("iters", "ok", "payload", "corrected", "frames")
    final = {k: np.zeros_like(want[k]) for k in keys}
    held = np.zeros(3, np.int64)
    done = np.zeros(3, bool)
    rounds = np.zeros(3, np.int64)
    calls = 0
    while not done.all():
        calls += 1
        r = blind(Q, H, plan1024, case, case.known_only(held), n_revealed=dev(held, np.int32),
                  skip=dev(done.astype(np.uint8)))
        live = ~done
        assert (r["rounds"][live] == 1).all() and (r["n_revealed"][live] == held[live]).all()
        for k in keys:
            final[k][live] = r[k][live]
        rounds[live] += 1
        failed = live & (r["ok"] == 0) & (held < 1024)
        done = ~failed
        held[failed] = np.minimum(1024, held[failed] + STEP)      # Alice sends fill[f, held:held + 256]
    assert calls == 4
    for k in keys:
        assert (final[k] == want[k]).all(), k
    assert (rounds == want["rounds"]).all() and (held == want["n_revealed"]).all()


# ---- 6. a large code: the classic kernel's large-code form -----------------------------------------

Q_LARGE = 0.0185


def test_large_code(Q, oracle_mod, qkd_opt):
    """The (3,12)-regular N = 24576 code, 2048 punctured and 512 shortened positions, 1024
    bits a round: one frame closes in round 0, the other needs a second round. On the
    split kernel and on the classic one (bit totals in global memory)."""
    from tests.test_adapt import regular_3_12
    n = 24576
    ptr, idx = regular_3_12(n, 3)
    g = AM.Graph(n, ptr, idx)
    Hr = Q.HMatrix.from_check_lists(n, ptr, idx)
    plan = Q.AdaptPlan.choose(Hr, 2560, 2048, 9)
    case = Case(g, plan.punctured, plan.shortened, 77, Q_LARGE, 2)
    loops = [case.loop(oracle_mod.libm, k, 0, 1024, 4) for k in range(2)]
    assert [m["rounds"] for m in loops] == [1, 2] and [m["n_revealed"] for m in loops] == [0, 1024]
    assert all(m["last"]["sp_ok"] for m in loops) and not any(r["nan"] for m in loops for r in m["all"])
    want = of_loops(loops)
    for kernel in (None, "classic"):
        qkd_opt("QKD_DECODE_KERNEL", kernel)
        got = blind(Q, Hr, plan, case, step=1024, max_rounds=4)
        assert_equal(got, want)
        assert (got["payload"] == case.payload).all()
    plan.close()
    Hr.close()


# ---- 7. a launch stream that is not the current one ------------------------------------------------

@pytest.mark.parametrize("handle", ["stream", "int"])
def test_other_stream(Q, H, plan1024, multi, handle):
    """stream= names a stream that is not torch's current one, while the current one is
    busy: the wrapper's own copy of n_revealed and its leak_bits must run on the launch
    stream, in order with the kernels. The frames start with counts whose decodes the model
    loop already holds (its rounds 1, 2 and 0), so a count read before its copy has landed,
    or a leak taken before the rounds have advanced it, shows."""
    assert_multi_preconditions(multi)
    case, loops = multi[0.08]
    start = [256, 512, 0]
    want = of_loops(loops)
    want["rounds"] = np.array([len(m["all"]) - s // STEP for m, s in zip(loops, start)])
    assert want["rounds"].tolist() == [1, 2, 3] and want["n_revealed"].tolist() == [256, 768, 512]
    d_bob, d_syn, d_fill, d_start = dev(case.bob), dev(case.syn), dev(case.fill), dev(start, np.int32)
    busy = torch.zeros(1 << 27, dtype=torch.float32, device="cuda")          # 512 MiB
    side = torch.cuda.Stream()
    torch.cuda.synchronize()                                                # (the inputs are ready everywhere)
    for _ in range(100):                                                    # the current stream: some 25 ms of work
        busy.add_(1.0)
    r = Q.reconcile_blind(H, plan1024, d_bob, d_syn, case.q, d_fill, d_start, step=STEP, max_rounds=6,
                          want_frames=True, stream=side if handle == "stream" else int(side.cuda_stream))
    side.synchronize()                                                      # the launch stream alone
    with torch.cuda.stream(side):                                           # (and the copies to the host on it)
        got = result(r, sync=False)
    assert_equal(got, want)
    torch.cuda.synchronize()
    assert d_start.cpu().tolist() == start
    assert float(busy[0]) == 100.0


# ---- 8. stream capture -----------------------------------------------------------------------------

def test_stream_capture(Q, H, plan1024, multi):
    """One multi-round call captured in a graph (after a call that sized the workspace)
    and replayed once: no synchronisation, host read or allocation inside the call."""
    assert_multi_preconditions(multi)
    case, loops = multi[0.08]
    d_bob, d_syn, d_fill = dev(case.bob), dev(case.syn), dev(case.fill)
    nrev = torch.zeros(3, dtype=torch.int32, device="cuda")
    ws = Q.Workspace(H)

    def call():
        return Q.reconcile_blind(H, plan1024, d_bob, d_syn, case.q, d_fill, nrev, step=STEP, max_rounds=6,
                                 want_frames=True, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = result(call())
    torch.cuda.current_stream().wait_stream(side)
    assert_equal(warm, of_loops(loops))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = call()
    torch.cuda.synchronize()
    for t in (r.iterations, r.syndromes_match, r.bits, r.corrected, r.frames, r.rounds, r.n_revealed, r.leak_bits):
        t.view(torch.uint8).fill_(GUARD)
    graph.replay()
    assert_equal(result(r), of_loops(loops))
    assert nrev.cpu().tolist() == [0, 0, 0]
    del graph
    ws.close()
