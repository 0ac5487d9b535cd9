"""Key verification inside rate-adaptive and blind reconciliation on the GPU
(verify_tags on a plan, reconcile_adaptive / reconcile_blind with alice_tags=): the
payload's tag taken by both class-mode decoder kernels as they write the payload, and the
blind rounds closed by `verified`, against tests/adapt_verify_model.py (payload_tag from
the window definition; the round loop on the numpy decoder of tests/adapt_model.py, pinned
to the oracle by tests/test_adapt_abi.py) and against the non-verifying calls, all by
exact equality. Inputs were chosen on the CPU with the model; each test asserts on the
model's own record that it exercises what it is for. The golden cases are
tests/test_blind.py's: payload, fill, then noise from default_rng(400), the plan
puncturing the first p positions of adapt_positions(seed 5)."""
import numpy as np
import pytest

from tests import adapt_model as AM
from tests import adapt_verify_model as VM

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_blind import GUARD, STEP, Case, assert_equal, dev, of_loops  # noqa: E402

SEED = 12345
M_GOLD = 5231
MASK64 = (1 << 64) - 1


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


@pytest.fixture(scope="module")
def plan1024(Q, H):
    plan = Q.AdaptPlan.choose(H, 1024, 1024, 5)
    yield plan
    plan.close()


def words_dev(R):
    return torch.from_numpy(np.array(R, np.uint64).view(np.int64)).cuda()


def tags_host(t):
    return t.cpu().numpy().view(np.uint64)


def tags_dev(tags):
    return torch.from_numpy(np.array(tags, np.uint64).view(np.int64)).cuda()


def model_tags(R, payloads, tag_bits=64):
    return np.array([VM.payload_tag(R, x, tag_bits) for x in payloads], np.uint64)


def result(r, sync=True):
    """A verifying BlindResult / ReconcileResult on the host: a dict of numpy arrays."""
    if sync:
        torch.cuda.synchronize()
    out = {"iters": r.iterations, "ok": r.syndromes_match, "payload": r.bits, "corrected": r.corrected,
           "frames": r.frames, "rounds": getattr(r, "rounds", None), "n_revealed": getattr(r, "n_revealed", None),
           "leak_bits": getattr(r, "leak_bits", None), "tags": r.tags, "verified": r.verified}
    out = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    if out["tags"] is not None:
        out["tags"] = out["tags"].view(np.uint64)
    return {k: v for k, v in out.items() if v is not None}


def of_vloops(loops):
    """What a verifying blind call must return for frames whose model loops are `loops`."""
    want = of_loops(loops)
    want["tags"] = np.array([m["tag"] for m in loops], np.uint64)
    want["verified"] = np.array([m["ok"] for m in loops], np.uint8)
    return want


def without(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}


# ---- 1. Alice's tags -------------------------------------------------------------------

def check_plan_tags(Q, plan, n_payload, rng):
    assert plan.n_payload == n_payload
    payload = rng.integers(0, 256, (3, n_payload)).astype(np.uint8)       # (only byte & 1 counts)
    payload[1] &= 0xFE                                                       # the all-zero key
    R_seed = VM.expand_key(SEED, n_payload)
    assert Q.verify_expand_key(SEED, n_payload).tolist() == R_seed and len(R_seed) == Q.verify_key_words(n_payload)
    R_rand = rng.integers(0, 2**64, len(R_seed), dtype=np.uint64).tolist()
    d = dev(payload)
    out = min(64, n_payload)                     # (privacy amplification: out_bits <= n_in)
    for R, kw in ((R_seed, {"hash_seed": SEED}), (R_rand, {"hash_words": words_dev(R_rand)})):
        pw = words_dev(R[:Q.privacy_key_words(n_payload, out)])
        pa = Q.privacy_amplify(d, out, hash_words=pw)
        torch.cuda.synchronize()
        pa = pa.cpu().numpy().view(np.uint64)[:, 0]
        for t in (1, 13, 64):
            want = model_tags(R, payload, t)
            assert want[1] == 0
            got = tags_host(Q.verify_tags(plan, d, tag_bits=t, **kw))
            assert (got == want).all(), (n_payload, t, kw.keys())
            m = MASK64 >> (64 - min(t, out))
            assert ((got & np.uint64(m)) == (pa & np.uint64(m))).all(), (n_payload, t)
    assert (tags_host(Q.verify_tags(plan, d)) == model_tags(VM.expand_key(0, n_payload), payload)).all()


def test_alice_tags(Q, H, dense_codes):
    rng = np.random.default_rng(1)
    dense = next(d for d in dense_codes.values() if d.shape[1] == 7)
    Hd = Q.HMatrix.from_dense_array(dense)
    plans = [(Q.AdaptPlan(Hd, [2], [5]), 5), (Q.AdaptPlan.choose(H, 1024, 1024, 5), 9216),
             (Q.AdaptPlan.choose(H, 1037, 1000, 5), 9203)]
    for plan, n_payload in plans:
        check_plan_tags(Q, plan, n_payload, rng)
        plan.close()
    Hd.close()


# ---- 2, 3. the honest adaptive link, and tampered tags ------------------------------------

ADAPT_FIELDS = ("iterations", "syndromes_match", "bits", "corrected", "frames")


def same_decode(a, b):
    for name in ADAPT_FIELDS:
        x, y = getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()
        assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), name


@pytest.mark.parametrize("kernel", [None, "classic"])
def test_honest_adaptive_link(Q, H, G, plan1024, qkd_opt, kernel):
    qkd_opt("QKD_DECODE_KERNEL", kernel)
    case = Case(G, plan1024.punctured, [], 400, 0.02, 3)
    d_bob, d_syn = dev(case.bob), dev(case.syn)
    at = Q.verify_tags(plan1024, dev(case.payload), hash_seed=SEED)
    R = VM.expand_key(SEED, 9216)
    assert (tags_host(at) == model_tags(R, case.payload)).all()
    plain = Q.reconcile_adaptive(H, plan1024, d_bob, d_syn, case.q, want_frames=True)
    got = Q.reconcile_adaptive(H, plan1024, d_bob, d_syn, case.q, want_frames=True, hash_seed=SEED, alice_tags=at)
    torch.cuda.synchronize()
    assert plain.tags is None and plain.verified is None
    same_decode(got, plain)
    assert (got.bits.cpu().numpy() == case.payload).all()            # (QBER 0.02: every frame reconciles)
    assert got.verified.cpu().numpy().tolist() == [1, 1, 1]
    assert (tags_host(got.tags) == tags_host(at)).all()
    # the caller's key string, and tags without a verdict
    Rr = np.random.default_rng(2).integers(0, 2**64, len(R), dtype=np.uint64).tolist()
    only = Q.reconcile_adaptive(H, plan1024, d_bob, d_syn, case.q, want_frames=True, hash_words=words_dev(Rr),
                                tag_bits=13, want_tags=True)
    torch.cuda.synchronize()
    assert only.verified is None
    same_decode(only, plain)
    assert (tags_host(only.tags) == model_tags(Rr, case.payload, 13)).all()


def test_tampered_tags(Q, H, G, plan1024):
    """Alice's tags flipped inside the 13-bit mask: no frame verifies; outside it: nothing changes."""
    case = Case(G, plan1024.punctured, [], 400, 0.02, 3)
    d_bob, d_syn = dev(case.bob), dev(case.syn)
    t = 13
    at = Q.verify_tags(plan1024, dev(case.payload), hash_seed=SEED, tag_bits=t)
    call = lambda tags: Q.reconcile_adaptive(H, plan1024, d_bob, d_syn, case.q, want_frames=True, hash_seed=SEED,
                                             tag_bits=t, alice_tags=tags)
    good, inside, outside = call(at), call(at ^ (1 << (t - 1))), call(at ^ (1 << t))
    torch.cuda.synchronize()
    assert good.verified.cpu().numpy().tolist() == [1, 1, 1]
    assert inside.verified.cpu().numpy().tolist() == [0, 0, 0]
    assert outside.verified.cpu().numpy().tolist() == [1, 1, 1]
    for r in (inside, outside):
        same_decode(r, good)
        assert (tags_host(r.tags) == tags_host(good.tags)).all()
    assert (tags_host(good.tags) == model_tags(VM.expand_key(SEED, 9216), case.payload, t)).all()


# ---- 4. same syndrome, wrong key -------------------------------------------------------------

@pytest.mark.parametrize("kernel", [None, "classic"])
def test_same_syndrome_wrong_key(Q, dense_codes, oracle_mod, qkd_opt, kernel):
    """The case the feature exists for, on the 7-bit code with position 0 punctured: Bob's
    payload is that of alice ^ c for a nonzero codeword c, so the decoder lands on a word
    with Alice's syndrome that is not hers. Adaptive: syndromes_match 1, verified 0. Blind,
    two rounds of one bit: round 0 matches under a wrong tag and the frame is advanced; with
    c = 1010101 the revealed bit contradicts the wrong word and round 1 ends on Alice's
    key, verified; with c = 1110000 it ends on a wrong word again and stays unverified."""
    qkd_opt("QKD_DECODE_KERNEL", kernel)
    dense = next(d for d in dense_codes.values() if d.shape[1] == 7)
    g = AM.Graph.from_dense(dense)
    Hd = Q.HMatrix.from_dense_array(dense)
    plan = Q.AdaptPlan(Hd, [0], [])
    pay = np.arange(1, 7)
    R = VM.expand_key(SEED, 6)
    alice = np.random.default_rng(7).integers(0, 2, (4, 7)).astype(np.uint8)
    syn = np.stack([g.syndrome(x) for x in alice])
    at_model = model_tags(R, alice[:, pay])
    at = Q.verify_tags(plan, dev(alice[:, pay]), hash_seed=SEED)
    assert (tags_host(at) == at_model).all()
    for c, recovers in (([1, 0, 1, 0, 1, 0, 1], True), ([1, 1, 1, 0, 0, 0, 0], False)):
        c = np.array(c, np.uint8)
        assert not g.syndrome(c).any() and c.any()
        bob = (alice ^ c)[:, pay]
        loops = [VM.blind_loop(g, [0], [], bob[k], syn[k], 0.02, oracle_mod.libm, alice[k, :1], R, 64,
                               int(at_model[k]), 0, 1, 2) for k in range(4)]
        for k, m in enumerate(loops):
            first = m["all"][0]
            assert first["sp_ok"] and m["verified"][0] is False and m["rounds"] == 2 and m["n_revealed"] == 1
            assert (first["out"][pay] != alice[k, pay]).any() and not any(r["nan"] for r in m["all"])
            assert m["last"]["sp_ok"] and m["ok"] == recovers
            assert bool((m["payload"] == alice[k, pay]).all()) == recovers
        a = result(Q.reconcile_adaptive(Hd, plan, dev(bob), dev(syn), 0.02, want_frames=True, hash_seed=SEED,
                                        alice_tags=at))
        assert a["ok"].tolist() == [1] * 4 and a["verified"].tolist() == [0] * 4
        assert (a["payload"] == np.stack([m["all"][0]["out"][pay] for m in loops])).all()
        assert (a["tags"] == np.array([m["tags"][0] for m in loops], np.uint64)).all()
        b = result(Q.reconcile_blind(Hd, plan, dev(bob), dev(syn), 0.02, dev(alice[:, :1]), step=1, max_rounds=2,
                                     want_frames=True, hash_seed=SEED, alice_tags=at))
        assert_equal(b, of_vloops(loops))
        assert b["verified"].tolist() == [int(recovers)] * 4 and b["rounds"].tolist() == [2] * 4
        # without Alice's tags the wrong word closes the frame in round 0
        plain = result(Q.reconcile_blind(Hd, plan, dev(bob), dev(syn), 0.02, dev(alice[:, :1]), step=1, max_rounds=2,
                                         want_frames=True, hash_seed=SEED, want_tags=True))
        assert plain["rounds"].tolist() == [1] * 4 and plain["ok"].tolist() == [1] * 4
        assert (plain["payload"] == a["payload"]).all() and (plain["tags"] == a["tags"]).all()
    plan.close()
    Hd.close()


# ---- 5. failing frames ---------------------------------------------------------------------------

def test_failing_frames(Q, H, G, plan1024, oracle_mod):
    case = Case(G, plan1024.punctured, [], 400, 0.11, 3)
    recs = [AM.decode(G, AM.frame_llrs(G.n, case.pu, [], case.bob[k], case.q, 100.0)[0], case.syn[k],
                      oracle_mod.libm, 12) for k in range(3)]
    assert not any(r["sp_ok"] or r["nan"] for r in recs)
    at = Q.verify_tags(plan1024, dev(case.payload), hash_seed=SEED)
    got = result(Q.reconcile_adaptive(H, plan1024, dev(case.bob), dev(case.syn), case.q, max_iterations=12,
                                      want_frames=True, hash_seed=SEED, alice_tags=at))
    assert got["ok"].tolist() == [0, 0, 0] and got["verified"].tolist() == [0, 0, 0]
    assert got["iters"].tolist() == [12, 12, 12]
    assert (got["frames"] == np.stack([r["out"] for r in recs])).all()
    assert (got["tags"] == model_tags(VM.expand_key(SEED, 9216), got["payload"])).all()
    assert (got["tags"] != tags_host(at)).all()


# ---- 6 - 8, 12. blind reconciliation -----------------------------------------------------------------

FLIPPED = 0          # the frame of the QBER 0.08 call whose announced tag is wrong in tests 7, 8 and 12


@pytest.fixture(scope="module")
def multi(G, plan1024, oracle_mod):
    """test_blind.py's two multi-round calls (QBER 0.08 and 0.07, 3 frames each, p = 1024,
    step 256, 6 rounds) with Alice's honest tags, and the QBER 0.08 call with frame
    FLIPPED's tag wrong, as model loops computed once."""
    R = VM.expand_key(SEED, 9216)
    out = {"R": R}
    for q in (0.08, 0.07):
        case = Case(G, plan1024.punctured, [], 400, q, 3)
        tags = model_tags(R, case.payload)
        loops = [VM.blind_loop(G, case.pu, [], case.bob[k], case.syn[k], q, oracle_mod.libm, case.fill[k], R, 64,
                               int(tags[k]), 0, STEP, 6) for k in range(3)]
        out[q] = (case, tags, loops)
    case, tags, loops = out[0.08]
    bad = tags.copy()
    bad[FLIPPED] ^= np.uint64(1 << 40)
    k = FLIPPED
    wrong = VM.blind_loop(G, case.pu, [], case.bob[k], case.syn[k], 0.08, oracle_mod.libm, case.fill[k], R, 64,
                          int(bad[k]), 0, STEP, 6)
    out["flipped"] = (case, bad, [wrong if j == k else m for j, m in enumerate(loops)])
    return out


def assert_multi_preconditions(multi):
    hi, lo = multi[0.08][2], multi[0.07][2]
    assert [m["rounds"] for m in hi] == [2, 4, 3] and [m["n_revealed"] for m in hi] == [256, 768, 512]
    assert [m["rounds"] for m in lo] == [1, 2, 2] and [m["n_revealed"] for m in lo] == [0, 256, 256]
    for q in (0.08, 0.07):
        case, tags, loops = multi[q]
        assert all(m["last"]["sp_ok"] and m["ok"] for m in loops)
        assert not any(r["nan"] for m in loops for r in m["all"])
        assert all(r["iters"] == 50 and not r["sp_ok"] for m in loops for r in m["all"][:-1])
        assert all((m["payload"] == case.payload[k]).all() for k, m in enumerate(loops))
        assert all(m["tag"] == int(tags[k]) for k, m in enumerate(loops))
    wrong = multi["flipped"][2][FLIPPED]
    # the frame matches in its round 1 and in every later round, and never verifies
    assert wrong["rounds"] == 5 and wrong["n_revealed"] == 1024 and wrong["ok"] is False
    assert [r["sp_ok"] for r in wrong["all"]] == [False, True, True, True, True]
    assert wrong["verified"] == [False] * 5 and (wrong["payload"] == multi[0.08][0].payload[FLIPPED]).all()


def blind(Q, H, plan, case, tags, revealed=None, **kw):
    kw.setdefault("want_frames", True)
    return result(Q.reconcile_blind(H, plan, dev(case.bob), dev(case.syn), case.q,
                                    dev(case.fill if revealed is None else revealed), hash_seed=SEED,
                                    alice_tags=None if tags is None else tags_dev(tags), **kw))


@pytest.mark.parametrize("kernel", [None, "classic"])
def test_blind_honest(Q, H, plan1024, multi, qkd_opt, kernel):
    assert_multi_preconditions(multi)
    qkd_opt("QKD_DECODE_KERNEL", kernel)
    for q in (0.08, 0.07):
        case, tags, loops = multi[q]
        at = Q.verify_tags(plan1024, dev(case.payload), hash_seed=SEED)
        assert (tags_host(at) == tags).all()
        got = blind(Q, H, plan1024, case, tags, step=STEP, max_rounds=6)
        assert_equal(got, of_vloops(loops))
        assert got["verified"].tolist() == [1, 1, 1] and (got["tags"] == tags).all()
        plain = Q.reconcile_blind(H, plan1024, dev(case.bob), dev(case.syn), case.q, dev(case.fill), step=STEP,
                                  max_rounds=6, want_frames=True)
        assert plain.tags is None and plain.verified is None
        assert_equal(without(got, "tags", "verified"), result(plain))
        assert (got["leak_bits"] == M_GOLD - 1024 + got["n_revealed"]).all()


@pytest.mark.parametrize("kernel", [None, "classic"])
def test_blind_flipped_tag(Q, H, plan1024, multi, qkd_opt, kernel):
    """One frame's announced tag is wrong: it never verifies and is decoded until all 1024
    punctured bits are revealed; the other frames are what they were."""
    assert_multi_preconditions(multi)
    qkd_opt("QKD_DECODE_KERNEL", kernel)
    case, bad, loops = multi["flipped"]
    got = blind(Q, H, plan1024, case, bad, step=STEP, max_rounds=6)
    assert_equal(got, of_vloops(loops))
    assert got["rounds"].tolist() == [5, 4, 3] and got["n_revealed"].tolist() == [1024, 768, 512]
    assert got["verified"].tolist() == [0, 1, 1] and got["ok"].tolist() == [1, 1, 1]
    honest = of_vloops(multi[0.08][2])
    others = [k for k in range(3) if k != FLIPPED]
    assert_equal(got, honest, rows=others)
    # tags alone: closing stays on syndromes_match, the honest call's rounds
    only = blind(Q, H, plan1024, case, None, step=STEP, max_rounds=6, want_tags=True)
    assert "verified" not in only
    assert_equal(only, without(honest, "verified"))


def test_real_link(Q, H, plan1024, multi):
    """Bob's loop on a link, one round a call with what he holds, skip = verified so far:
    the device-side multi-round call of the flipped-tag case, field for field."""
    assert_multi_preconditions(multi)
    case, bad, loops = multi["flipped"]
    want = blind(Q, H, plan1024, case, bad, step=STEP, max_rounds=6)
    assert_equal(want, of_vloops(loops))
    keys = ("iters", "ok", "payload", "corrected", "frames", "tags", "verified")
    final = {k: np.zeros_like(want[k]) for k in keys}
    held = np.zeros(3, np.int64)
    done = np.zeros(3, bool)
    rounds = np.zeros(3, np.int64)
    calls = 0
    while not done.all():
        calls += 1
        r = blind(Q, H, plan1024, case, bad, case.known_only(held), n_revealed=dev(held, np.int32),
                  skip=dev(done.astype(np.uint8)))
        live = ~done
        assert (r["rounds"][live] == 1).all() and (r["n_revealed"][live] == held[live]).all()
        for k in keys:
            final[k][live] = r[k][live]
        rounds[live] += 1
        failed = live & (r["verified"] == 0) & (held < 1024)
        done = ~failed
        held[failed] = np.minimum(1024, held[failed] + STEP)      # Alice sends fill[f, held:held + 256]
    assert calls == 5
    for k in keys:
        assert (final[k] == want[k]).all(), k
    assert (rounds == want["rounds"]).all() and (held == want["n_revealed"]).all()


def test_chain(Q, H, plan1024, multi):
    """reconcile_blind(alice_tags=) then privacy_amplify(keep=verified): Alice's own secret
    key on the verified frames, zeros on the other."""
    assert_multi_preconditions(multi)
    case, bad, loops = multi["flipped"]
    r = Q.reconcile_blind(H, plan1024, dev(case.bob), dev(case.syn), case.q, dev(case.fill), step=STEP, max_rounds=6,
                          hash_seed=SEED, alice_tags=tags_dev(bad))
    bob_key = Q.privacy_amplify(r.bits, 256, hash_seed=SEED + 1, keep=r.verified)
    alice_key = Q.privacy_amplify(dev(case.payload), 256, hash_seed=SEED + 1)
    torch.cuda.synchronize()
    bob_key, alice_key = bob_key.cpu().numpy(), alice_key.cpu().numpy()
    assert r.verified.cpu().numpy().tolist() == [0, 1, 1]
    others = [k for k in range(3) if k != FLIPPED]
    assert bob_key.shape == (3, 4) and (bob_key[others] == alice_key[others]).all() and alice_key[others].any()
    assert not bob_key[FLIPPED].any() and alice_key[FLIPPED].any()


# ---- 9. skipped frames ----------------------------------------------------------------------------------

def test_skip(Q, H, plan1024, multi):
    """tags and verified of a skipped frame are not written, in any round."""
    assert_multi_preconditions(multi)
    case, bad, loops = multi["flipped"]
    N = Q._native
    d = [dev(case.bob), dev(case.syn), dev(case.fill), tags_dev(bad)]

    def raw(skip):
        bufs = {"payload": torch.empty((3, 9216), dtype=torch.uint8, device="cuda"),
                "iters": torch.empty(3, dtype=torch.int32, device="cuda"),
                "ok": torch.empty(3, dtype=torch.uint8, device="cuda"),
                "rounds": torch.empty(3, dtype=torch.int32, device="cuda"),
                "tags": torch.empty(3, dtype=torch.int64, device="cuda"),
                "verified": torch.empty(3, dtype=torch.uint8, device="cuda")}
        for t in bufs.values():
            t.view(torch.uint8).fill_(GUARD)
        nrev = torch.zeros(3, dtype=torch.int32, device="cuda")
        st = N.lib().qkd_reconcile_blind_verify_batch(
            H.handle, None, plan1024.handle, d[0].data_ptr(), d[1].data_ptr(), 3, case.q, 100.0, 50, 100.0,
            N.FLAG_THRESHOLD, d[2].data_ptr(), nrev.data_ptr(), None if skip is None else dev(skip).data_ptr(), STEP,
            6, bufs["payload"].data_ptr(), None, bufs["iters"].data_ptr(), bufs["ok"].data_ptr(), None,
            bufs["rounds"].data_ptr(), SEED, None, 64, d[3].data_ptr(), bufs["tags"].data_ptr(),
            bufs["verified"].data_ptr(), int(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert st == 0
        return {k: v.cpu().numpy() for k, v in bufs.items()}

    full, part, none = raw(None), raw(np.array([0, 0xFF, 0], np.uint8)), raw(np.ones(3, np.uint8))
    assert (full["tags"].view(np.uint64) == of_vloops(loops)["tags"]).all()
    assert full["verified"].tolist() == [0, 1, 1] and full["rounds"].tolist() == [5, 4, 3]
    guard64 = int.from_bytes(bytes([GUARD] * 8), "little", signed=True)
    guard32 = int.from_bytes(bytes([GUARD] * 4), "little", signed=True)
    for key in full:
        g = {np.dtype(np.uint8): GUARD, np.dtype(np.int32): guard32, np.dtype(np.int64): guard64}[full[key].dtype]
        assert (part[key][[0, 2]] == full[key][[0, 2]]).all(), key
        assert (part[key][1] == g).all() and (none[key] == g).all(), key
        assert not (full[key].reshape(3, -1) == g).all(axis=1).any(), key


# ---- 10. a code past 65,536 bits: the classic kernel's large-code form -------------------------------------

def test_long_code(Q, oracle_mod):
    """The (3,12)-regular N = 69632 code (past the split kernel's sizes: the classic
    class-mode kernel, bit totals in global memory), 2048 punctured and 515 shortened
    positions, one frame: payload indices past 2^16 and a ragged payload width."""
    from tests.test_adapt import regular_3_12
    n = 69632
    ptr, idx = regular_3_12(n, 3)
    g = AM.Graph(n, ptr, idx)
    Hr = Q.HMatrix.from_check_lists(n, ptr, idx)
    plan = Q.AdaptPlan.choose(Hr, 2563, 2048, 9)
    assert plan.n_payload == 67069
    case = Case(g, plan.punctured, plan.shortened, 77, 0.0185, 1)
    R = VM.expand_key(SEED, plan.n_payload)
    tags = model_tags(R, case.payload)
    loops = [VM.blind_loop(g, case.pu, case.sh, case.bob[0], case.syn[0], case.q, oracle_mod.libm, case.fill[0], R,
                           64, int(tags[0]), 0, 1024, 3)]
    m = loops[0]
    assert m["last"]["sp_ok"] and m["ok"] and not any(r["nan"] for r in m["all"])
    assert (m["payload"] == case.payload[0]).all() and m["payload"][65536:].any()
    at = Q.verify_tags(plan, dev(case.payload), hash_seed=SEED)
    assert (tags_host(at) == tags).all()
    got = blind(Q, Hr, plan, case, tags, step=1024, max_rounds=3)
    assert_equal(got, of_vloops(loops))
    bad = blind(Q, Hr, plan, case, tags ^ np.uint64(1), step=1024, max_rounds=1)
    assert bad["verified"].tolist() == [0] and (bad["tags"] == model_tags(R, bad["payload"])).all()
    plan.close()
    Hr.close()


# ---- 11. stream capture -----------------------------------------------------------------------------------

def test_stream_capture(Q, H, plan1024, multi):
    """One verifying multi-round call captured in a graph (after a call that sized the
    workspace, the seeded key string's buffer included) and replayed once."""
    assert_multi_preconditions(multi)
    case, bad, loops = multi["flipped"]
    d_bob, d_syn, d_fill, d_tags = dev(case.bob), dev(case.syn), dev(case.fill), tags_dev(bad)
    nrev = torch.zeros(3, dtype=torch.int32, device="cuda")
    ws = Q.Workspace(H)

    def call():
        return Q.reconcile_blind(H, plan1024, d_bob, d_syn, case.q, d_fill, nrev, step=STEP, max_rounds=6,
                                 want_frames=True, workspace=ws, hash_seed=SEED, alice_tags=d_tags)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = result(call())
    torch.cuda.current_stream().wait_stream(side)
    assert_equal(warm, of_vloops(loops))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = call()
    torch.cuda.synchronize()
    for t in (r.iterations, r.syndromes_match, r.bits, r.corrected, r.frames, r.rounds, r.n_revealed, r.leak_bits,
              r.tags, r.verified):
        t.view(torch.uint8).fill_(GUARD)
    graph.replay()
    assert_equal(result(r), warm)
    assert nrev.cpu().tolist() == [0, 0, 0]
    del graph
    ws.close()
