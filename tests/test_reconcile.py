"""Bob-side reconciliation from a received syndrome (qkd_reconcile_batch,
Q.reconcile): decoded words, iteration counts and flags against the golden
vectors, the oracle (its QKD_LDPC when the syndrome is H * alice, its decoder
on the +-log_p LLRs otherwise) and qkd_ldpc on the same keys, all by exact
equality; `corrected` against the host popcount of bits ^ bob."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_GOLD, M_GOLD = 10240, 5231


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


def dev(x, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(x).astype(dtype)).cuda()


def seeds_dev(seeds):
    return torch.from_numpy(np.ascontiguousarray(seeds, np.uint64).view(np.int64)).cuda()


def host(r):
    """(iterations, syndromes_match as bool, bits, corrected or None) on the host."""
    torch.cuda.synchronize()
    return (r.iterations.cpu().numpy(), r.syndromes_match.cpu().numpy().astype(bool), r.bits.cpu().numpy(),
            None if r.corrected is None else r.corrected.cpu().numpy())


def assert_same(got, want):
    """got: host(reconcile result); want: (iters, sp_ok, bits) arrays."""
    assert (got[0] == want[0]).all(), (got[0], want[0])
    assert (got[1] == np.asarray(want[1], bool)).all()
    assert (got[2] == want[2]).all()


def assert_corrected(got, bob):
    assert (got[3] == (got[2] ^ np.asarray(bob, np.uint8)).sum(axis=1)).all()


def of_ldpc(r):
    torch.cuda.synchronize()
    return r.iterations.cpu().numpy(), r.syndromes_match.cpu().numpy().astype(bool), r.bits.cpu().numpy()


@pytest.fixture(scope="module")
def gold33(Q, H):
    """The first 33 config-2 frames (two whole 16-frame groups and a ragged group
    of one): keys, Alice's syndromes, and reconcile's outputs with every option at
    its default (test_golden checks them; the kernel-form tests compare with them)."""
    a, b, q = Q.keygen(H, seeds_dev(Q.make_seeds(777, 33)), 0.02)
    syn = Q.calculate_syndrome(H, a)
    q = float(q[0])
    ref = host(Q.reconcile(H, b, syn, q))
    return a, b, syn, q, ref


# ---- 1. golden ----------------------------------------------------------------------

def test_golden(Q, H, gold33, golden_vectors):
    a, b, syn, q, got = gold33
    assert (got[0] == golden_vectors["c2_iters"][:33]).all()
    assert (got[1] == golden_vectors["c2_sp"][:33]).all()
    ko = golden_vectors["c2_ko"][:33].astype(bool)
    assert (got[2][ko] == a.cpu().numpy()[ko]).all()
    assert_corrected(got, b.cpu().numpy())
    assert_same(got, of_ldpc(Q.qkd_ldpc(H, a, b, q, want_bits=True)))


# ---- 2. oracle parity off the easy path ---------------------------------------------

@pytest.mark.parametrize("q", [0.02, 0.08, 0.11, 0.5, 0.7])
@pytest.mark.parametrize("thr,thr_on", [(100.0, True), (0.7, True), (100.0, False)])
def test_oracle_parity(Q, H, oracle_code, q, thr, thr_on):
    """Failing frames (q >= 0.11), log((1-q)/q) = 0 (q = 0.5: NaN messages), negative
    LLR magnitudes (q > 0.5); one frame's nonzero syndrome bytes are 255."""
    rng = np.random.default_rng(int(q * 1000) + int(thr * 10) + thr_on)
    f = 3
    alice = rng.integers(0, 2, (f, N_GOLD)).astype(np.uint8)
    bob = alice ^ (rng.random((f, N_GOLD)) < min(q, 0.3)).astype(np.uint8)
    syn = np.stack([oracle_code.syndrome(x) for x in alice]).astype(np.uint8)
    syn[1] *= 255
    max_it = 12 if q >= 0.11 else 50
    got = host(Q.reconcile(H, dev(bob), dev(syn), q, max_it, thr, thr_on))
    want = [oracle_code.qkd_ldpc(alice[k], bob[k], q, max_it, thr, thr_on) for k in range(f)]
    assert_same(got, ([w["iters"] for w in want], [w["sp_ok"] for w in want], np.stack([w["out"] for w in want])))
    assert_corrected(got, bob)          # also where syndromes_match = 0


# ---- 3. a syndrome no key explains --------------------------------------------------

def test_syndrome_no_key_explains(Q, H, oracle_code):
    """H * alice with 7 random checks flipped: the target really comes from the caller.
    The LLRs use libm's log, as the library and the reference do."""
    rng = np.random.default_rng(2024)
    f, q, max_it = 3, 0.04, 12
    alice = rng.integers(0, 2, (f, N_GOLD)).astype(np.uint8)
    bob = alice ^ (rng.random((f, N_GOLD)) < q).astype(np.uint8)
    syn = np.stack([oracle_code.syndrome(x) for x in alice]).astype(np.uint8)
    for k in range(f):
        syn[k, rng.choice(M_GOLD, 7, replace=False)] ^= 1
    lp = math.log((1 - q) / q)
    got = host(Q.reconcile(H, dev(bob), dev(syn), q, max_it))
    want = [oracle_code.decode(np.where(bob[k] == 1, -lp, lp), syn[k], max_it, 100.0, True) for k in range(f)]
    assert_same(got, ([w["iters"] for w in want], [w["sp_ok"] for w in want], np.stack([w["out"] for w in want])))
    assert_corrected(got, bob)
    # and not what Alice's own syndrome gives
    syn_a = np.stack([oracle_code.syndrome(x) for x in alice]).astype(np.uint8)
    other = host(Q.reconcile(H, dev(bob), dev(syn_a), q, max_it))
    assert not (other[1] == got[1]).all() or not (other[2] == got[2]).all()


# ---- 4. kernel forms ----------------------------------------------------------------

def _shift4(x):
    """A copy of x at an address = 4 mod 8."""
    buf = torch.empty(x.numel() + 4, dtype=torch.uint8, device=x.device)
    v = buf[4:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 8 == 4
    return v


@pytest.mark.parametrize("form", ["gather", "pack", "bob_misaligned", "classic"])
def test_kernel_forms(Q, H, gold33, qkd_opt, form):
    """The gather frame-syndrome kernel (QKD_SYN_SLICED=0), Bob packed by pack_kernel
    first (QKD_SYN_BYTES=0, and chosen by the launcher for a key at 4 mod 8), and the
    classic decoder: the same outputs as the default form."""
    a, b, syn, q, ref = gold33
    if form == "gather":
        qkd_opt("QKD_SYN_SLICED", "0")
    elif form == "pack":
        qkd_opt("QKD_SYN_BYTES", "0")
    elif form == "bob_misaligned":
        b = _shift4(b)
    elif form == "classic":
        qkd_opt("QKD_DECODE_KERNEL", "classic")
    got = host(Q.reconcile(H, b, syn, q))
    assert_same(got, ref)
    assert (got[3] == ref[3]).all()


def test_kernel_form_no_speculation(Q, H, oracle_code, qkd_opt):
    """QKD_SPEC_CAP=0 at q = 0.04 (the exact iterations only) on the 33 frames' seeds."""
    a, b, q = Q.keygen(H, seeds_dev(Q.make_seeds(777, 33)), 0.04)
    q = float(q[0])
    syn = Q.calculate_syndrome(H, a)
    ref = host(Q.reconcile(H, b, syn, q))
    assert_same(ref, of_ldpc(Q.qkd_ldpc(H, a, b, q, want_bits=True)))
    qkd_opt("QKD_SPEC_CAP", "0")
    got = host(Q.reconcile(H, b, syn, q))
    assert_same(got, ref)
    assert (got[3] == ref[3]).all()
    an, bn = a.cpu().numpy(), b.cpu().numpy()
    for k in (0, 16, 32):
        w = oracle_code.qkd_ldpc(an[k], bn[k], q)
        assert got[0][k] == w["iters"] and got[1][k] == w["sp_ok"] and (got[2][k] == w["out"]).all()


# ---- 5. variants --------------------------------------------------------------------

@pytest.mark.parametrize("variant,sc", [("sp_f32", False), ("minsum", False), ("minsum", True)])
def test_variants_equal_qkd_ldpc(Q, H, variant, sc):
    a, b, q = Q.keygen(H, seeds_dev(Q.make_seeds(777, 33)), 0.06)
    q = float(q[0])
    syn = Q.calculate_syndrome(H, a)
    got = host(Q.reconcile(H, b, syn, q, variant=variant, minsum_self_correct=sc))
    assert_same(got, of_ldpc(Q.qkd_ldpc(H, a, b, q, want_bits=True, variant=variant, minsum_self_correct=sc)))
    assert_corrected(got, b.cpu().numpy())


@pytest.mark.parametrize("sc", [False, True])
def test_minsum_lds_state_equals_qkd_ldpc(Q, H, qkd_opt, sc):
    """QKD_MINSUM_STORE=lds: the LDS-state min-sum rules run in the classic kernel,
    whose given-target branch then serves this entry."""
    qkd_opt("QKD_MINSUM_STORE", "lds")
    a, b, q = Q.keygen(H, seeds_dev(Q.make_seeds(777, 33)), 0.06)
    q = float(q[0])
    syn = Q.calculate_syndrome(H, a)
    got = host(Q.reconcile(H, b, syn, q, variant="minsum", minsum_self_correct=sc))
    assert_same(got, of_ldpc(Q.qkd_ldpc(H, a, b, q, want_bits=True, variant="minsum", minsum_self_correct=sc)))
    assert_corrected(got, b.cpu().numpy())


# ---- 6. tiny codes ------------------------------------------------------------------

def test_tiny_codes(Q, dense_codes, oracle_mod):
    """N = 6, 7, 10: N % 8 != 0 (Bob through pack_kernel), M < 32 (one ragged
    syndrome word), fewer frames than a 16-frame group."""
    rng = np.random.default_rng(6)
    assert sorted(d.shape[1] for d in dense_codes.values()) == [6, 7, 10]
    for name, dense in dense_codes.items():
        Hd = Q.HMatrix.from_dense_array(dense)
        oc = oracle_mod.Code.from_dense(dense)
        n = dense.shape[1]
        alice = rng.integers(0, 2, (5, n)).astype(np.uint8)
        bob = alice ^ (rng.random((5, n)) < 0.1).astype(np.uint8)
        syn = np.stack([oc.syndrome(x) for x in alice]).astype(np.uint8)
        got = host(Q.reconcile(Hd, dev(bob), dev(syn), 0.1))
        want = [oc.qkd_ldpc(alice[k], bob[k], 0.1) for k in range(5)]
        assert_same(got, ([w["iters"] for w in want], [w["sp_ok"] for w in want],
                          np.stack([w["out"] for w in want])))
        assert_corrected(got, bob)


# ---- 7. past the split limit --------------------------------------------------------

def regular_code(n, dv=3, dc=6, seed=0):
    """A random (dv, dc)-regular code by the permutation construction: the n * dv bit
    sockets shuffled into m rows of dc; rows with a repeated bit trade one entry with
    another row until none is left. -> (m, check_ptr, check_idx), rows ascending."""
    rng = np.random.default_rng(seed)
    m = n * dv // dc
    rows = rng.permutation(np.repeat(np.arange(n), dv)).reshape(m, dc)
    for _ in range(1000):
        srt = np.sort(rows, axis=1)
        bad = np.nonzero((np.diff(srt, axis=1) == 0).any(axis=1))[0]
        if bad.size == 0:
            break
        for j in bad:
            k = int(np.argmax(np.bincount(rows[j], minlength=1)[rows[j]] > 1))
            o, ko = int(rng.integers(0, m)), int(rng.integers(0, dc))
            rows[j, k], rows[o, ko] = rows[o, ko], rows[j, k]
    else:
        raise AssertionError("no simple regular code found")
    rows = np.sort(rows, axis=1)
    return m, np.arange(0, m * dc + 1, dc, dtype=np.int32), rows.ravel().astype(np.int32)


def test_past_split_limit(Q, oracle_mod):
    """N = 65,664, the first multiple of 64 above 65,536: this entry runs the classic
    keys path there (the interleaved long-code decoder gives no decisions)."""
    n = 65664
    m, cp, ci = regular_code(n, seed=7)
    Hb = Q.HMatrix.from_check_lists(n, cp, ci)
    cptr, cidx, bptr, bidx = Hb.adjacency()
    oc = oracle_mod.Code.from_lists({"bit_off": bptr, "bit_idx": bidx, "chk_off": cptr, "chk_idx": cidx,
                                     "dims": [n, m, 3, 6]})
    rng = np.random.default_rng(65664)
    alice = rng.integers(0, 2, (2, n)).astype(np.uint8)
    bob = alice ^ (rng.random((2, n)) < 0.02).astype(np.uint8)
    syn = np.stack([oc.syndrome(x) for x in alice]).astype(np.uint8)
    got = host(Q.reconcile(Hb, dev(bob), dev(syn), 0.02, 20))
    want = [oc.qkd_ldpc(alice[k], bob[k], 0.02, 20) for k in range(2)]
    assert_same(got, ([w["iters"] for w in want], [w["sp_ok"] for w in want], np.stack([w["out"] for w in want])))
    assert_corrected(got, bob)


# ---- 8. corrected not asked for -----------------------------------------------------

def test_without_corrected(Q, H, gold33, qkd_opt):
    a, b, syn, q, ref = gold33
    r = Q.reconcile(H, b, syn, q, want_corrected=False)
    assert r.corrected is None
    assert_same(host(r), ref)
    # the classic decoder writes the bytes itself: no count kernel follows it
    qkd_opt("QKD_DECODE_KERNEL", "classic")
    r = Q.reconcile(H, b, syn, q, want_corrected=False)
    assert r.corrected is None
    assert_same(host(r), ref)
