"""Key verification tags (qkd_verify_tags_batch / Q.verify_tags, and
qkd_reconcile_verify_batch / Q.reconcile with its hash arguments) against a
numpy model of the hash in its matrix form, tag bit i = XOR_p r[p + i] x_p, by
exact equality; the other outputs of the verifying reconcile against the plain
one's, by exact equality too."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_GOLD, M_GOLD = 10240, 5231
SEED = 0x5EEDC0DE2026


# ---- the model ------------------------------------------------------------------------

def splitmix_words(seed, count):
    """R[k] = mix(seed + (k + 1) * golden) mod 2^64 (SplitMix64 in counter form)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(count, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def key_words(n):
    return (n + 63 + 63) // 64


def model_tags(R, bits, t=64):
    """The matrix form: A[i, p] = r[p + i] (t x N, Hankel), tag = A x over GF(2), bit i
    of the tag = row i. bits [F, N] bytes (a key bit is byte & 1) -> uint64 [F]."""
    R = np.asarray(R, np.uint64)
    x = (np.atleast_2d(bits) & 1).astype(np.int64)
    n = x.shape[1]
    assert R.size == key_words(n)
    k = np.arange(n + 63)
    r = ((R[k >> 6] >> (k & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int64)
    A = r[np.arange(t)[:, None] + np.arange(n)[None, :]]
    b = ((x @ A.T) & 1).astype(np.uint64)
    return np.bitwise_or.reduce(b << np.arange(t, dtype=np.uint64), axis=1)


def test_model_window_form():
    """The model against the window form of the definition, at N = 10 with seed 12345."""
    R = splitmix_words(12345, key_words(10))
    assert R.size == 2
    big = int(R[0]) | (int(R[1]) << 64)
    x = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1], np.uint8)
    tag = 0
    for p in np.nonzero(x)[0]:
        tag ^= (big >> int(p)) & (2**64 - 1)
    assert int(model_tags(R, x)[0]) == tag
    assert int(model_tags(R, x, 13)[0]) == tag & 0x1fff
    assert int(model_tags(R, np.zeros(10, np.uint8))[0]) == 0


# ---- fixtures -------------------------------------------------------------------------

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


def words_dev(R):
    return torch.from_numpy(np.ascontiguousarray(R, np.uint64).view(np.int64)).cuda()


def seeds_dev(seeds):
    return torch.from_numpy(np.ascontiguousarray(seeds, np.uint64).view(np.int64)).cuda()


def tags_host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def host(r):
    """(iterations, syndromes_match as bool, bits, corrected or None, tags, verified as bool or None)"""
    torch.cuda.synchronize()
    return (r.iterations.cpu().numpy(), r.syndromes_match.cpu().numpy().astype(bool), r.bits.cpu().numpy(),
            None if r.corrected is None else r.corrected.cpu().numpy(),
            None if r.tags is None else r.tags.cpu().numpy().view(np.uint64),
            None if r.verified is None else r.verified.cpu().numpy().astype(bool))


def assert_same_decode(got, want, corrected=True):
    assert (got[0] == want[0]).all(), (got[0], want[0])
    assert (got[1] == want[1]).all()
    assert (got[2] == want[2]).all()
    if corrected:
        assert (got[3] == want[3]).all()


@pytest.fixture(scope="module")
def gold33(Q, H):
    """The first 33 config-2 frames (seed 777, QBER 0.02): keys, Alice's syndromes and
    tags, plain reconcile's outputs, the verifying reconcile's with every option at its
    default, and the seeded key string."""
    a, b, q = Q.keygen(H, seeds_dev(Q.make_seeds(777, 33)), 0.02)
    syn = Q.calculate_syndrome(H, a)
    q = float(q[0])
    at = Q.verify_tags(H, a, hash_seed=SEED)
    plain = host(Q.reconcile(H, b, syn, q))
    ver = host(Q.reconcile(H, b, syn, q, hash_seed=SEED, alice_tags=at))
    return dict(a=a, b=b, syn=syn, q=q, at=at, plain=plain, ver=ver, R=splitmix_words(SEED, key_words(N_GOLD)))


# ---- 1. tags of byte keys -------------------------------------------------------------

def code_n70(Q):
    """N = 70 (N % 4 != 0, more than one word), 35 checks of three bits, every bit covered."""
    rows = [sorted({2 * j, 2 * j + 1, (2 * j + 5) % 70}) for j in range(35)]
    ptr = np.arange(0, 3 * 35 + 1, 3, dtype=np.int32)
    return Q.HMatrix.from_check_lists(70, ptr, np.array(rows, np.int32).ravel())


def check_byte_tags(Q, Hc, n, frames, rng):
    """verify_tags against the model: random bytes (high bits set; only & 1 counts), one
    frame of even bytes (the all-zero key), seeded and with hash_words, t = 1, 13, 64,
    and the same bytes at an address one past an aligned one."""
    bits = rng.integers(0, 256, (frames, n)).astype(np.uint8)
    bits[frames // 2] &= 0xFE
    R_seed = splitmix_words(SEED, key_words(n))
    assert (Q.verify_expand_key(SEED, n) == R_seed).all()
    R_rand = rng.integers(0, 2**64, key_words(n), dtype=np.uint64)
    d = dev(bits)
    buf = torch.empty(bits.size + 1, dtype=torch.uint8, device="cuda")
    odd = buf[1:].view(frames, n)
    odd.copy_(d)
    assert odd.data_ptr() % 2 == 1
    for t in (1, 13, 64):
        want_seed = model_tags(R_seed, bits, t)
        want_rand = model_tags(R_rand, bits, t)
        assert want_seed[frames // 2] == 0 and want_rand[frames // 2] == 0
        for x in (d, odd):
            assert (tags_host(Q.verify_tags(Hc, x, hash_seed=SEED, tag_bits=t)) == want_seed).all(), (n, t)
            assert (tags_host(Q.verify_tags(Hc, x, hash_words=words_dev(R_rand), tag_bits=t)) == want_rand).all(), (n, t)
    # the defaults: seed 0, 64 bits
    assert (tags_host(Q.verify_tags(Hc, d)) == model_tags(splitmix_words(0, key_words(n)), bits)).all()


def test_tags_tiny_codes(Q, dense_codes):
    rng = np.random.default_rng(1)
    assert sorted(d.shape[1] for d in dense_codes.values()) == [6, 7, 10]
    for dense in dense_codes.values():
        check_byte_tags(Q, Q.HMatrix.from_dense_array(dense), dense.shape[1], 5, rng)


def test_tags_n70(Q):
    check_byte_tags(Q, code_n70(Q), 70, 5, np.random.default_rng(70))


def test_tags_golden_code(Q, H):
    check_byte_tags(Q, H, N_GOLD, 33, np.random.default_rng(33))


def test_tags_of_keygen_keys(Q, H, gold33):
    g = gold33
    assert (tags_host(g["at"]) == model_tags(g["R"], g["a"].cpu().numpy())).all()
    zero = torch.zeros(2, N_GOLD, dtype=torch.uint8, device="cuda")
    assert (tags_host(Q.verify_tags(H, zero, hash_seed=SEED)) == 0).all()


# ---- 2. the honest link ---------------------------------------------------------------

def test_honest_link(Q, H, gold33):
    g = gold33
    got, plain = g["ver"], g["plain"]
    assert_same_decode(got, plain)
    assert (got[4] == model_tags(g["R"], got[2])).all()
    same_key = (got[2] == g["a"].cpu().numpy()).all(axis=1)
    assert (got[5] == (same_key & got[1])).all()
    assert got[5].sum() >= 30          # config 2 at QBER 0.02: nearly every frame reconciles
    # want_tags alone: the tags, no verdict
    r = Q.reconcile(H, g["b"], g["syn"], g["q"], hash_seed=SEED, want_tags=True)
    assert r.verified is None
    only = host(r)
    assert_same_decode(only, plain)
    assert (only[4] == got[4]).all()


@pytest.mark.parametrize("t", [1, 13])
def test_honest_link_short_tags_and_hash_words(Q, H, gold33, t):
    """t-bit tags under a caller's key string; Alice's tags tampered inside the mask
    (every frame fails) and outside it (nothing changes)."""
    g = gold33
    rng = np.random.default_rng(t)
    R = rng.integers(0, 2**64, key_words(N_GOLD), dtype=np.uint64)
    w = words_dev(R)
    at = Q.verify_tags(H, g["a"], hash_words=w, tag_bits=t)
    assert (tags_host(at) == model_tags(R, g["a"].cpu().numpy(), t)).all()
    got = host(Q.reconcile(H, g["b"], g["syn"], g["q"], hash_words=w, tag_bits=t, alice_tags=at))
    assert_same_decode(got, g["plain"])
    assert (got[4] == model_tags(R, got[2], t)).all()
    # (a frame decoded to another word with Alice's syndrome collides with probability 2^-t)
    assert (got[5] == (got[1] & (got[4] == tags_host(at)))).all()
    assert (got[5] >= g["ver"][5]).all() and got[5].sum() >= 30
    inside = at ^ (1 << (t - 1))
    outside = at ^ (1 << t)
    bad = host(Q.reconcile(H, g["b"], g["syn"], g["q"], hash_words=w, tag_bits=t, alice_tags=inside))
    assert not bad[5].any()
    assert (bad[4] == got[4]).all()
    same = host(Q.reconcile(H, g["b"], g["syn"], g["q"], hash_words=w, tag_bits=t, alice_tags=outside))
    assert (same[5] == got[5]).all()


# ---- 3. same syndrome, wrong key ------------------------------------------------------

def test_same_syndrome_wrong_key(Q, dense_codes):
    """The case the feature exists for: bob = alice ^ c for a nonzero codeword c has
    Alice's syndrome, the decoder stays on it and reports syndromes_match = 1."""
    dense = next(d for d in dense_codes.values() if d.shape[1] == 7)
    Hd = Q.HMatrix.from_dense_array(dense)
    words = ((np.arange(128)[:, None] >> np.arange(7)) & 1).astype(np.uint8)
    cw = words[((words @ dense.T.astype(np.int64)) % 2 == 0).all(axis=1)]
    cw = cw[cw.any(axis=1)]
    assert len(cw) > 0
    c = cw[0]
    rng = np.random.default_rng(7)
    alice = rng.integers(0, 2, (4, 7)).astype(np.uint8)
    bob = alice ^ c
    syn = ((alice @ dense.T.astype(np.int64)) % 2).astype(np.uint8)
    R = splitmix_words(SEED, key_words(7))
    ta, tb = model_tags(R, alice), model_tags(R, bob)
    assert (ta != tb).all()                   # this seed separates the two keys
    at = Q.verify_tags(Hd, dev(alice), hash_seed=SEED)
    assert (tags_host(at) == ta).all()
    got = host(Q.reconcile(Hd, dev(bob), dev(syn), 0.02, hash_seed=SEED, alice_tags=at))
    assert got[1].all()                       # the syndromes match ...
    assert (got[2] != alice).any(axis=1).all()          # ... on a key that is not Alice's
    assert (got[4] == model_tags(R, got[2])).all()
    assert not got[5].any()
    ctl = host(Q.reconcile(Hd, dev(alice), dev(syn), 0.02, hash_seed=SEED, alice_tags=at))
    assert ctl[1].all() and (ctl[2] == alice).all()
    assert ctl[5].all()


def test_small_codes_reconcile(Q, dense_codes):
    """N = 6, 7, 10 and 70 through the verifying reconcile: N % 4 != 0, the unpack's
    one-position form; a single word and two words of decisions."""
    rng = np.random.default_rng(4)
    codes = [(Q.HMatrix.from_dense_array(d), d.shape[1]) for d in dense_codes.values()] + [(code_n70(Q), 70)]
    for Hc, n in codes:
        alice = rng.integers(0, 2, (5, n)).astype(np.uint8)
        bob = alice.copy()
        bob[1, n // 2] ^= 1
        bob[3, n - 1] ^= 1
        a_d, b_d = dev(alice), dev(bob)
        syn = Q.calculate_syndrome(Hc, a_d)
        R = splitmix_words(SEED, key_words(n))
        for t in (13, 64):
            at = Q.verify_tags(Hc, a_d, hash_seed=SEED, tag_bits=t)
            plain = host(Q.reconcile(Hc, b_d, syn, 0.1))
            for wc in (True, False):
                got = host(Q.reconcile(Hc, b_d, syn, 0.1, hash_seed=SEED, tag_bits=t, alice_tags=at,
                                       want_corrected=wc))
                assert_same_decode(got, plain, corrected=wc)
                assert (got[4] == model_tags(R, got[2], t)).all(), (n, t)
                assert (got[5] == (got[1] & (got[4] == model_tags(R, alice, t)))).all(), (n, t)


# ---- 4. failing frames ----------------------------------------------------------------

def test_failing_frames(Q, H):
    rng = np.random.default_rng(110)
    f, q, max_it, t = 3, 0.11, 12, 13
    alice = rng.integers(0, 2, (f, N_GOLD)).astype(np.uint8)
    bob = alice ^ (rng.random((f, N_GOLD)) < q).astype(np.uint8)
    syn = Q.calculate_syndrome(H, dev(alice))
    R = splitmix_words(SEED, key_words(N_GOLD))
    plain = host(Q.reconcile(H, dev(bob), syn, q, max_it))
    assert not plain[1].all()                 # frames fail at this QBER in 12 iterations
    r = Q.reconcile(H, dev(bob), syn, q, max_it, hash_seed=SEED, tag_bits=t, want_tags=True)
    got = host(r)
    assert_same_decode(got, plain)
    assert (got[4] == model_tags(R, got[2], t)).all()       # the last hard decision's tags
    # against the tags of the decisions themselves only the syndrome flag decides
    own = host(Q.reconcile(H, dev(bob), syn, q, max_it, hash_seed=SEED, tag_bits=t, alice_tags=r.tags))
    assert (own[5] == plain[1]).all()
    assert not own[5][~plain[1]].any()
    inside = host(Q.reconcile(H, dev(bob), syn, q, max_it, hash_seed=SEED, tag_bits=t, alice_tags=r.tags ^ 1))
    assert not inside[5].any()
    outside = host(Q.reconcile(H, dev(bob), syn, q, max_it, hash_seed=SEED, tag_bits=t,
                               alice_tags=r.tags ^ (1 << t)))
    assert (outside[5] == own[5]).all()
    # against Alice's real tags: nothing verifies where the syndrome does not match
    at = Q.verify_tags(H, dev(alice), hash_seed=SEED, tag_bits=t)
    real = host(Q.reconcile(H, dev(bob), syn, q, max_it, hash_seed=SEED, tag_bits=t, alice_tags=at))
    assert not real[5][~plain[1]].any()


# ---- 5. every path gives the same tags ------------------------------------------------

@pytest.mark.parametrize("form", ["classic", "gather", "no_corrected", "classic_no_corrected", "workspace", "stream"])
def test_every_path_same_outputs(Q, H, gold33, qkd_opt, form):
    g = gold33
    kw = dict(hash_seed=SEED, alice_tags=g["at"])
    if form in ("classic", "classic_no_corrected"):
        qkd_opt("QKD_DECODE_KERNEL", "classic")
    if form == "gather":
        qkd_opt("QKD_SYN_SLICED", "0")
    if form in ("no_corrected", "classic_no_corrected"):
        kw["want_corrected"] = False
    if form == "workspace":
        kw["workspace"] = Q.Workspace(H)
    if form == "stream":
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            r = Q.reconcile(H, g["b"], g["syn"], g["q"], stream=s, **kw)
        s.synchronize()
    else:
        r = Q.reconcile(H, g["b"], g["syn"], g["q"], **kw)
    got = host(r)
    assert (got[3] is None) == ("no_corrected" in form)
    assert_same_decode(got, g["ver"], corrected=got[3] is not None)
    assert (got[4] == g["ver"][4]).all()
    assert (got[5] == g["ver"][5]).all()


@pytest.mark.parametrize("store", [None, "lds"])
def test_minsum_variant(Q, H, gold33, qkd_opt, store):
    """min-sum on the split skeleton and with its state in LDS (the classic kernel, which
    writes bits_out itself): its own decisions, tagged."""
    g = gold33
    if store:
        qkd_opt("QKD_MINSUM_STORE", store)
    plain = host(Q.reconcile(H, g["b"], g["syn"], g["q"], variant="minsum"))
    got = host(Q.reconcile(H, g["b"], g["syn"], g["q"], variant="minsum", hash_seed=SEED, alice_tags=g["at"]))
    assert_same_decode(got, plain)
    assert (got[4] == model_tags(g["R"], got[2])).all()
    assert (got[5] == ((got[2] == g["a"].cpu().numpy()).all(axis=1) & got[1])).all()


# ---- 6. a long code -------------------------------------------------------------------

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


def test_long_code(Q):
    """N = 65,664, past the split decoder's limit: the classic kernel, then the byte-key
    tag kernel on bits_out (1027 key-string words)."""
    n = 65664
    m, cp, ci = regular_code(n, seed=7)
    Hb = Q.HMatrix.from_check_lists(n, cp, ci)
    rng = np.random.default_rng(65664)
    alice = rng.integers(0, 2, (2, n)).astype(np.uint8)
    bob = alice ^ (rng.random((2, n)) < 0.02).astype(np.uint8)
    a_d, b_d = dev(alice), dev(bob)
    syn = Q.calculate_syndrome(Hb, a_d)
    R = splitmix_words(SEED, key_words(n))
    assert R.size == 1027
    at = Q.verify_tags(Hb, a_d, hash_seed=SEED)
    assert (tags_host(at) == model_tags(R, alice)).all()
    plain = host(Q.reconcile(Hb, b_d, syn, 0.02, 20))
    got = host(Q.reconcile(Hb, b_d, syn, 0.02, 20, hash_seed=SEED, alice_tags=at))
    assert_same_decode(got, plain)
    assert (got[4] == model_tags(R, got[2])).all()
    assert (got[5] == ((got[2] == alice).all(axis=1) & got[1])).all()
