"""Privacy amplification (qkd_privacy_amplify_batch / Q.privacy_amplify) against a
numpy model of the hash in its matrix form, out_i = parity of x & r[i : i + n_in], by
exact equality, under both kernel forms (QKD_PRIVACY_KERNEL direct | table)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_GOLD = 10240
SEED = 0x9A17ACE5EED2026          # the privacy seed; test_verify.py's verification seed is another
VERIFY_SEED = 0x5EEDC0DE2026
FORMS = ["direct", "table"]


# ---- the model ------------------------------------------------------------------------

def splitmix_words(seed, count):
    """R[k] = mix(seed + (k + 1) * golden) mod 2^64 (SplitMix64 in counter form)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(count, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def key_words(n_in, L):
    return (n_in + L - 1 + 63) // 64


def model_hash(R, keys, L):
    """The matrix form: A[i, p] = r[p + i] (L x n_in, Hankel), out = A x over GF(2), in
    row blocks of A (binary32 products are exact: the sums stay below 2^24).
    keys [F, n_in] bytes (a key bit is byte & 1) -> uint64 [F, ceil(L / 64)]."""
    R = np.asarray(R, np.uint64)
    x = (np.atleast_2d(keys) & 1).astype(np.float32)
    f, n = x.shape
    assert R.size == key_words(n, L) and n < 2**24
    k = np.arange(n + L - 1)
    r = ((R[k >> 6] >> (k & 63).astype(np.uint64)) & np.uint64(1)).astype(np.float32)
    rows = np.lib.stride_tricks.sliding_window_view(r, n)          # rows[i] = r[i : i + n]
    assert rows.shape == (L, n)
    bits = np.zeros((f, (L + 63) // 64 * 64), np.uint64)
    step = max(1, (1 << 24) // n)
    for i0 in range(0, L, step):
        A = np.ascontiguousarray(rows[i0:i0 + step])
        bits[:, i0:i0 + A.shape[0]] = (x @ A.T).astype(np.int64) & 1
    return np.bitwise_or.reduce(bits.reshape(f, -1, 64) << np.arange(64, dtype=np.uint64), axis=2)


def test_model_window_form():
    """The model against the window form of the definition, at n_in = 10, L = 7."""
    R = splitmix_words(12345, key_words(10, 7))
    assert R.size == 1
    x = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1], np.uint8)
    out = 0
    for p in np.nonzero(x)[0]:
        out ^= (int(R[0]) >> int(p)) & 0x7f
    assert model_hash(R, x, 7).tolist() == [[out]]
    assert model_hash(R, x | 0xA4, 7).tolist() == [[out]]
    assert model_hash(R, np.zeros(10, np.uint8), 7).tolist() == [[0]]


# ---- fixtures -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import qkd_ldpc_amd as Q
    return Q


@pytest.fixture(params=FORMS)
def form(request, Q):
    """Runs the test under one kernel form; the default comes back afterwards."""
    try:
        Q.set_debug_option("QKD_PRIVACY_KERNEL", request.param)
        yield request.param
    finally:
        Q.set_debug_option("QKD_PRIVACY_KERNEL", None)


def dev(x, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(x).astype(dtype)).cuda()


def words_dev(R):
    return torch.from_numpy(np.ascontiguousarray(R, np.uint64).view(np.int64)).cuda()


def out_host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def misaligned(t):
    """The same bytes at a base address one past an aligned one."""
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device="cuda")
    odd = buf[1:].view(t.shape)
    odd.copy_(t)
    assert odd.data_ptr() % 2 == 1 and odd.is_contiguous()
    return odd


SHAPES = [(1, 1, 1), (70, 70, 33), (333, 65, 31), (333, 65, 65), (10240, 4096, 33), (20011, 20011, 3),
          (2**20 - 3, 130, 2)]
_cases = {}


def case(n_in, L, frames):
    """Random bytes 0..255 (only & 1 may count) with one frame of even bytes, the seeded
    key string and the model's output; computed once and shared, never modified."""
    key = (n_in, L, frames)
    if key not in _cases:
        rng = np.random.default_rng(n_in * 131 + L * 7 + frames)
        keys = rng.integers(0, 256, (frames, n_in)).astype(np.uint8)
        keys[frames // 2] &= 0xFE
        R = splitmix_words(SEED, key_words(n_in, L))
        want = model_hash(R, keys, L)
        assert not want[frames // 2].any()                  # the all-zero key
        if L % 64:
            assert not (want[:, -1] >> np.uint64(L % 64)).any()
        for a in (keys, R, want):
            a.setflags(write=False)
        _cases[key] = dict(keys=keys, R=R, want=want, d=dev(keys))
    return _cases[key]


# ---- 1. shapes, 2. misalignment -------------------------------------------------------

@pytest.mark.parametrize("n_in,L,frames", SHAPES)
def test_shapes(Q, form, n_in, L, frames):
    c = case(n_in, L, frames)
    assert Q.privacy_key_words(n_in, L) == key_words(n_in, L)
    assert (Q.privacy_expand_key(SEED, n_in, L) == c["R"]).all()
    wo = (L + 63) // 64
    seeded = Q.privacy_amplify(c["d"], L, hash_seed=SEED)
    assert seeded.shape == (frames, wo) and seeded.dtype == torch.int64
    assert (out_host(seeded) == c["want"]).all()
    worded = Q.privacy_amplify(c["d"], L, hash_seed=1, hash_words=words_dev(c["R"]))
    assert (out_host(worded) == c["want"]).all()
    odd = Q.privacy_amplify(misaligned(c["d"]), L, hash_seed=SEED)
    assert (out_host(odd) == c["want"]).all()


@pytest.mark.parametrize("n_in,L,frames", [(1, 1, 1), (70, 70, 33), (333, 65, 65)])
def test_random_key_string(Q, form, n_in, L, frames):
    """A caller's key string that no seed gives; uint64 words where torch has them."""
    c = case(n_in, L, frames)
    R = np.random.default_rng(L).integers(0, 2**64, key_words(n_in, L), dtype=np.uint64)
    want = model_hash(R, c["keys"], L)
    w = words_dev(R)
    assert (out_host(Q.privacy_amplify(c["d"], L, hash_words=w)) == want).all()
    if hasattr(torch, "uint64"):
        assert (out_host(Q.privacy_amplify(c["d"], L, hash_words=w.view(torch.uint64))) == want).all()


# ---- 3. output bounds -----------------------------------------------------------------

@pytest.mark.parametrize("n_in,L,frames", [(1, 1, 1), (70, 70, 33), (333, 65, 31), (10240, 4096, 33), (20011, 20011, 3)])
def test_output_bounds(Q, form, n_in, L, frames):
    """The C entry on a buffer of all-ones patterns with guard words after it: every
    word overwritten, the bits at and above L zero, the guards intact."""
    c = case(n_in, L, frames)
    wo, guard = (L + 63) // 64, 64
    buf = torch.full((frames * wo + guard,), -1, dtype=torch.int64, device="cuda")
    N = Q._native
    N.check(N.lib().qkd_privacy_amplify_batch(0, c["d"].data_ptr(), frames, n_in, L, SEED, None, None,
                                              buf.data_ptr(), torch.cuda.current_stream().cuda_stream))
    got = out_host(buf)
    assert (got[frames * wo:] == np.uint64(2**64 - 1)).all()
    assert (got[:frames * wo].reshape(frames, wo) == c["want"]).all()
    if L % 64:
        assert not (got[:frames * wo].reshape(frames, wo)[:, -1] >> np.uint64(L % 64)).any()


# ---- 4. keep --------------------------------------------------------------------------

@pytest.mark.parametrize("n_in,L,frames", [(70, 70, 33), (333, 65, 65), (10240, 4096, 33)])
def test_keep(Q, form, n_in, L, frames):
    c = case(n_in, L, frames)
    keep = (np.arange(frames) % 3 != 1).astype(np.uint8)
    keep[-1] = 0
    keep[frames // 2 - 1] = 7                     # any nonzero byte keeps
    got = out_host(Q.privacy_amplify(c["d"], L, hash_seed=SEED, keep=dev(keep)))
    assert not got[keep == 0].any()
    assert (got[keep != 0] == c["want"][keep != 0]).all()
    assert c["want"][keep == 0].any()             # (the mask did something)
    none = out_host(Q.privacy_amplify(c["d"], L, hash_seed=SEED, keep=dev(np.zeros(frames))))
    assert not none.any()


# ---- 5. the verification tag, 6. linearity, 7. streams --------------------------------

def test_is_the_verification_tag_at_64_bits(Q, form, golden_code):
    H = Q.HMatrix.from_check_lists(int(golden_code["dims"][0]), golden_code["chk_off"], golden_code["chk_idx"])
    a = case(N_GOLD, 4096, 33)["d"]
    assert Q.privacy_key_words(N_GOLD, 64) == Q.verify_key_words(N_GOLD)
    for s in (VERIFY_SEED, 0):
        tags = out_host(Q.verify_tags(H, a, hash_seed=s))
        assert (out_host(Q.privacy_amplify(a, 64, hash_seed=s))[:, 0] == tags).all()


def test_linearity(Q, form):
    rng = np.random.default_rng(6)
    x, y = rng.integers(0, 256, (2, 1, 333)).astype(np.uint8)
    hx, hy, hxy = (out_host(Q.privacy_amplify(dev(v), 65, hash_seed=SEED)) for v in (x, y, x ^ y))
    assert hx.any() and hy.any()
    assert (hxy == hx ^ hy).all()


def test_non_default_stream(Q, form):
    c = case(333, 65, 65)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = Q.privacy_amplify(c["d"], 65, hash_seed=SEED, stream=s)
    s.synchronize()
    assert (out_host(got) == c["want"]).all()


# ---- 8. end to end --------------------------------------------------------------------

def test_end_to_end(Q, form, golden_code):
    """The first 33 config-2 frames (seed 777, QBER 0.02): keygen, Alice's syndromes and
    tags, Bob's verifying reconcile, then both sides' privacy amplification under a seed
    of its own."""
    assert SEED != VERIFY_SEED
    H = Q.HMatrix.from_check_lists(int(golden_code["dims"][0]), golden_code["chk_off"], golden_code["chk_idx"])
    seeds = torch.from_numpy(Q.make_seeds(777, 33).view(np.int64)).cuda()
    a, b, q = Q.keygen(H, seeds, 0.02)
    syn = Q.calculate_syndrome(H, a)
    at = Q.verify_tags(H, a, hash_seed=VERIFY_SEED)
    r = Q.reconcile(H, b, syn, float(q[0]), hash_seed=VERIFY_SEED, alice_tags=at)
    alice = out_host(Q.privacy_amplify(a, 4096, hash_seed=SEED))
    bob = out_host(Q.privacy_amplify(r.bits, 4096, hash_seed=SEED, keep=r.verified))
    ok = r.verified.cpu().numpy().astype(bool)
    assert ok.all() and ok.size == 33
    assert alice.shape == (33, 64) and alice.any(axis=1).all()
    assert (alice[ok] == bob[ok]).all()
    # B frames hashed as one block: the same bits_out buffer, n_in = B * N
    block = out_host(Q.privacy_amplify(r.bits[:32].view(4, 8 * N_GOLD), 8192, hash_seed=SEED))
    assert (block == out_host(Q.privacy_amplify(a[:32].view(4, 8 * N_GOLD), 8192, hash_seed=SEED))).all()
    assert block.shape == (4, 128)
