"""Long-block privacy amplification (qkd_privacy_amplify_long_batch /
Q.privacy_amplify_long) by exact equality: against the numpy model of the hash in its
matrix form (tests/privacy_model.py) under one, two and many transform passes
(QKD_PRIVACY_NTT_LOG2), against the direct and table kernels of privacy_amplify where both
forms accept the shape, against their tiled composition past the old limit, and at the
largest size (a transform of 2^27 points) against inputs whose hash is known in closed
form."""
import numpy as np
import pytest

from tests import privacy_model as PM

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 0x10F6B10C5EED2026
M20 = 2**20


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import qkd_ldpc_amd as Q
    return Q


def dev(x, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(x).astype(dtype)).cuda()


def words_dev(R):
    return torch.from_numpy(np.ascontiguousarray(R, np.uint64).view(np.int64)).cuda()


def out_host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


_cases = {}


def case(n_in, L, blocks):
    """Random bytes 0..255 (only & 1 may count), with one block of even bytes where there
    are several, the seeded key string and the model's output; computed once and shared,
    never modified."""
    key = (n_in, L, blocks)
    if key not in _cases:
        rng = np.random.default_rng(n_in * 131 + L * 7 + blocks)
        keys = rng.integers(0, 256, (blocks, n_in)).astype(np.uint8)
        if blocks > 1:
            keys[blocks // 2] &= 0xFE
        R = PM.splitmix_words(SEED, PM.key_words(n_in, L))
        want = PM.model_hash(R, keys, L)
        if blocks > 1:
            assert not want[blocks // 2].any()              # the all-zero key
            assert want[0].any()
        if L % 64:
            assert not (want[:, -1] >> np.uint64(L % 64)).any()
        for a in (keys, R, want):
            a.setflags(write=False)
        _cases[key] = dict(keys=keys, R=R, want=want, d=dev(keys))
    return _cases[key]


# ---- 1. shapes under each pass count --------------------------------------------------

SMALL = [(1, 1, 1), (70, 70, 33), (193, 64, 3), (194, 64, 3), (333, 65, 31), (10240, 4096, 33), (20011, 20011, 3)]
LARGE = [(M20 - 3, 130, 2), (M20 + 1, 1, 1), (M20 + 77, 192, 2)]


@pytest.mark.parametrize("cap", [None, 3, 5])
@pytest.mark.parametrize("n_in,L,blocks", SMALL)
def test_small_shapes(Q, qkd_opt, n_in, L, blocks, cap):
    """2^13 points a workgroup (one pass up to 2^13, else two), 2^5 (two or three passes at a
    few hundred points, more above) and 2^3 (three passes and more)."""
    qkd_opt("QKD_PRIVACY_NTT_LOG2", cap)
    check_shape(Q, n_in, L, blocks)


@pytest.mark.parametrize("n_in,L,blocks", LARGE)
def test_large_shapes(Q, n_in, L, blocks):
    """Below the old limit and the first shapes past it: transforms of 2^20 and 2^21 points."""
    check_shape(Q, n_in, L, blocks)


def check_shape(Q, n_in, L, blocks):
    c = case(n_in, L, blocks)
    assert Q.privacy_long_key_words(n_in, L) == PM.key_words(n_in, L)
    assert (Q.privacy_long_expand_key(SEED, n_in, L) == c["R"]).all()
    seeded = Q.privacy_amplify_long(c["d"], L, hash_seed=SEED)
    assert seeded.shape == (blocks, (L + 63) // 64) and seeded.dtype == torch.int64
    got = out_host(seeded)
    assert (got == c["want"]).all()
    if blocks > 1:
        assert not got[blocks // 2].any()
    if L % 64:
        assert not (got[:, -1] >> np.uint64(L % 64)).any()
    worded = Q.privacy_amplify_long(c["d"], L, hash_seed=1, hash_words=words_dev(c["R"]))
    assert (out_host(worded) == c["want"]).all()


# ---- 2. equality with the existing kernels --------------------------------------------

@pytest.mark.parametrize("form", ["direct", "table"])
@pytest.mark.parametrize("n_in,L,blocks", [(10240, 4096, 33), (M20 - 3, 130, 2)])
def test_equals_existing_kernels(Q, qkd_opt, n_in, L, blocks, form):
    c = case(n_in, L, blocks)
    qkd_opt("QKD_PRIVACY_KERNEL", form)
    assert (out_host(Q.privacy_amplify_long(c["d"], L, hash_seed=SEED)) ==
            out_host(Q.privacy_amplify(c["d"], L, hash_seed=SEED))).all()
    R = np.random.default_rng(L).integers(0, 2**64, PM.key_words(n_in, L), dtype=np.uint64)
    w = words_dev(R)
    long_form = out_host(Q.privacy_amplify_long(c["d"], L, hash_words=w))
    assert (long_form == out_host(Q.privacy_amplify(c["d"], L, hash_words=w))).all()
    assert long_form.any() and (long_form != c["want"]).any()          # (another string)


# ---- 3. a long output without a model -------------------------------------------------

def tiled_hash(Q, keys, L, words, chunk=M20, tile=2**19):
    """The hash of one long block from the existing kernels: the XOR over chunks of the
    input of the hashes of output tiles, each under the slice of the key string that
    starts at bit p0 + o0 (both multiples of 64). keys [1, n_in]; -> int64 [1, ceil(L / 64)]."""
    n_in = keys.shape[1]
    out = torch.zeros(1, (L + 63) // 64, dtype=torch.int64, device=keys.device)
    for o0 in range(0, L, tile):
        lt = min(tile, L - o0)
        for p0 in range(0, n_in, chunk):
            nc = min(chunk, n_in - p0)
            w0 = (p0 + o0) // 64
            assert lt <= nc and (p0 + o0) % 64 == 0
            part = Q.privacy_amplify(keys[:, p0:p0 + nc].contiguous(), lt,
                                     hash_words=words[w0:w0 + Q.privacy_key_words(nc, lt)])
            out[:, o0 // 64:o0 // 64 + part.shape[1]] ^= part
    return out


def test_long_output_equals_tiled_existing_kernels(Q):
    n_in, L = 3 * M20, 2 * M20 + 320
    rng = np.random.default_rng(3)
    keys = dev(rng.integers(0, 256, (1, n_in)).astype(np.uint8))
    R = rng.integers(0, 2**64, PM.key_words(n_in, L), dtype=np.uint64)
    w = words_dev(R)
    got = out_host(Q.privacy_amplify_long(keys, L, hash_words=w))
    want = out_host(tiled_hash(Q, keys, L, w))
    assert got.shape == (1, (L + 63) // 64)
    assert (got == want).all()
    assert L % 64 == 0 and got[:, -5:].all()          # (the last tile, 320 bits, is there)


# ---- 4. the largest size --------------------------------------------------------------

def test_largest_size(Q):
    """n_in = 2^26 + 1, L = 2^26: a transform of 2^27 points. (a) All-ones input under an
    all-ones key string: every count is n_in, the largest residue the design meets, and odd,
    so every output bit is 1. (b) The last input bit alone: the output is the key string's
    bits p .. p + L - 1, p = n_in - 1."""
    n_in, L = 2**26 + 1, 2**26
    wp, wo = PM.key_words(n_in, L), L // 64
    assert Q.privacy_long_key_words(n_in, L) == wp == 2**21
    need = Q.privacy_long_scratch_bytes(n_in, L)
    assert 2**30 < need < 2**30 + 2**20
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    try:
        ones = torch.ones(1, n_in, dtype=torch.uint8, device="cuda")
        all_words = torch.full((wp,), -1, dtype=torch.int64, device="cuda")
        got = out_host(Q.privacy_amplify_long(ones, L, hash_words=all_words, scratch=scratch))
        assert got.shape == (1, wo)
        assert (got == np.uint64(2**64 - 1)).all()
        del ones, all_words

        p = n_in - 1
        R = np.random.default_rng(4).integers(0, 2**64, wp, dtype=np.uint64)
        one = torch.zeros(1, n_in, dtype=torch.uint8, device="cuda")
        one[0, p] = 0xFF
        got = out_host(Q.privacy_amplify_long(one, L, hash_words=words_dev(R), scratch=scratch))
        lo = R[p // 64:p // 64 + wo] >> np.uint64(p % 64)
        hi = np.append(R[p // 64 + 1:p // 64 + wo], np.uint64(0)) << np.uint64(64 - p % 64) if p % 64 else np.uint64(0)
        assert (got[0] == (lo | hi)).all()
        del one
    finally:
        del scratch
        torch.cuda.empty_cache()


# ---- 5. bookkeeping -------------------------------------------------------------------

def test_keep_is_per_block(Q):
    c = case(333, 65, 31)
    keys = c["d"][:3]
    got = out_host(Q.privacy_amplify_long(keys, 65, hash_seed=SEED, keep=dev(np.array([1, 0, 1]))))
    assert not got[1].any() and c["want"][1].any()
    assert (got[[0, 2]] == c["want"][[0, 2]]).all()
    got = out_host(Q.privacy_amplify_long(keys, 65, hash_seed=SEED, keep=dev(np.array([0, 9, 0]))))
    assert not got[[0, 2]].any() and (got[1] == c["want"][1]).all()


def test_misaligned_keys(Q):
    c = case(333, 65, 31)
    buf = torch.empty(c["d"].numel() + 1, dtype=torch.uint8, device="cuda")
    odd = buf[1:].view(c["d"].shape)
    odd.copy_(c["d"])
    assert odd.data_ptr() % 2 == 1 and odd.is_contiguous()
    assert (out_host(Q.privacy_amplify_long(odd, 65, hash_seed=SEED)) == c["want"]).all()


def test_non_default_stream(Q):
    c = case(10240, 4096, 33)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = Q.privacy_amplify_long(c["d"], 4096, hash_seed=SEED, stream=s)
        raw = Q.privacy_amplify_long(c["d"], 4096, hash_seed=SEED, stream=s.cuda_stream)
    s.synchronize()
    assert (out_host(got) == c["want"]).all() and (out_host(raw) == c["want"]).all()


def test_scratch_reused_and_too_short(Q):
    """One scratch over two calls of different sizes (at an odd base address: any
    alignment); a scratch one byte short is refused."""
    a, b = case(10240, 4096, 33), case(333, 65, 31)
    need = Q.privacy_long_scratch_bytes(10240, 4096)
    assert need >= Q.privacy_long_scratch_bytes(333, 65) > 0
    scratch = torch.full((need + 1,), 0xA5, dtype=torch.uint8, device="cuda")[1:]
    for _ in range(2):
        assert (out_host(Q.privacy_amplify_long(a["d"], 4096, hash_seed=SEED, scratch=scratch)) == a["want"]).all()
        assert (out_host(Q.privacy_amplify_long(b["d"], 65, hash_seed=SEED, scratch=scratch)) == b["want"]).all()
    with pytest.raises(Q.QkdError) as ei:
        Q.privacy_amplify_long(a["d"], 4096, hash_seed=SEED, scratch=scratch[:need - 1])
    assert ei.value.status == Q._native.ERR_INVALID_ARG and "scratch_bytes" in str(ei.value)
    for bad in (scratch.cpu(), scratch.to(torch.int32)):
        with pytest.raises(Q.QkdError):
            Q.privacy_amplify_long(b["d"], 65, hash_seed=SEED, scratch=bad)


@pytest.mark.parametrize("n_in,L,blocks", [(1, 1, 1), (333, 65, 31), (20011, 20011, 3)])
def test_output_bounds(Q, n_in, L, blocks):
    """The C entry on a buffer of all-ones patterns with sentinel words before and after:
    every word overwritten, the bits at and above L zero, the sentinels intact."""
    c = case(n_in, L, blocks)
    wo, guard = (L + 63) // 64, 64
    buf = torch.full((guard + blocks * wo + guard,), -1, dtype=torch.int64, device="cuda")
    need = Q.privacy_long_scratch_bytes(n_in, L)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    N = Q._native
    N.check(N.lib().qkd_privacy_amplify_long_batch(0, c["d"].data_ptr(), blocks, n_in, L, SEED, None, None,
                                                   buf.data_ptr() + 8 * guard, scratch.data_ptr(), need,
                                                   torch.cuda.current_stream().cuda_stream))
    got = out_host(buf)
    assert (got[:guard] == np.uint64(2**64 - 1)).all() and (got[guard + blocks * wo:] == np.uint64(2**64 - 1)).all()
    body = got[guard:guard + blocks * wo].reshape(blocks, wo)
    assert (body == c["want"]).all()
    if L % 64:
        assert not (body[:, -1] >> np.uint64(L % 64)).any()


def test_same_bits_on_every_run(Q):
    c = case(M20 + 77, 192, 2)
    first = out_host(Q.privacy_amplify_long(c["d"], 192, hash_seed=SEED))
    again = out_host(Q.privacy_amplify_long(c["d"], 192, hash_seed=SEED))
    assert (first == again).all() and (first == c["want"]).all()


def test_linearity(Q):
    rng = np.random.default_rng(6)
    x, y = rng.integers(0, 256, (2, 1, M20 + 77)).astype(np.uint8)
    hx, hy, hxy = (out_host(Q.privacy_amplify_long(dev(v), 192, hash_seed=SEED)) for v in (x, y, x ^ y))
    assert hx.any() and hy.any()
    assert (hxy == hx ^ hy).all()


# ---- 6. forwarding --------------------------------------------------------------------

def test_privacy_amplify_forwards_past_the_old_limit(Q):
    c = case(M20 + 77, 192, 2)
    assert Q.privacy_key_words(M20 + 77, 192) == 0
    got = Q.privacy_amplify(c["d"], 192, hash_seed=SEED)
    assert got.shape == (2, 3) and got.dtype == torch.int64
    assert (out_host(got) == out_host(Q.privacy_amplify_long(c["d"], 192, hash_seed=SEED))).all()
    assert (out_host(got) == c["want"]).all()
    kept = out_host(Q.privacy_amplify(c["d"], 192, hash_words=words_dev(c["R"]), keep=dev(np.array([1, 0]))))
    assert (kept[0] == c["want"][0]).all() and not kept[1].any()
    with pytest.raises(Q.QkdError):
        Q.privacy_amplify(torch.zeros(1, 2**27 + 1, dtype=torch.uint8, device="cuda"), 1)
