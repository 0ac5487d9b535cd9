"""Privacy amplification of the kept frames of a block (qkd_privacy_amplify_kept_batch /
Q.privacy_amplify_kept) by exact equality. The expected words are always the numpy model of
the hash (tests/privacy_model.py) on the kept frames compacted in numpy and padded with
zeros to the block's length, never anything the code under test computed: over shapes that
straddle frames inside a lane, fill the output, cross the scan's chunks and take several
strided passes; over flag patterns mixed within one call; against privacy_amplify_long on
the same buffer (all kept) and on the compacted frames at the shorter length (the prefix
rule); with dropped frames overwritten; between guard bytes; captured in a graph whose
replay follows the flags' new contents; and at the end of the chain reconcile -> verify ->
privacy amplification on the golden code."""
import os

import numpy as np
import pytest

from tests import privacy_model as PM

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 0x10F6B10C5EED2026
GUARD = 0xA5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATTERNS = ("all", "none", "first", "last", "alternating", "random")


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import qkd_ldpc_amd as Q
    return Q


def dev(x, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(x).astype(dtype)).cuda()


def words_dev(R):
    return torch.from_numpy(np.array(R, np.uint64).view(np.int64)).cuda()          # (a copy: R may be read-only)


def out_host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def flags_of(pattern, B, rng, p_keep=0.9):
    """[B] uint8: 0 for a dropped frame, one of 1, 2, 255 for a kept one. "random" keeps about
    p_keep of the frames, and with two frames or more drops at least one and keeps at least one."""
    f = np.arange(B)
    on = {"all": f >= 0, "none": f < 0, "first": f == 0, "last": f == B - 1, "alternating": (f & 1) == 1,
          "random": rng.random(B) < p_keep}[pattern]
    if pattern == "random" and B >= 2:
        if on.all():
            on[B // 2] = False
        if not on.any():
            on[B // 3] = True
    return np.where(on, rng.choice(np.array([1, 2, 255], np.uint8), B), 0).astype(np.uint8)


def compacted(frames, flags):
    """frames [nb, B, N] bytes, flags [nb, B] -> (the kept frames of each block set end to end
    in frame order with zeros behind them, [nb, B * N]; the kept counts [nb])."""
    nb, B, N = frames.shape
    x = np.zeros((nb, B * N), np.uint8)
    kept = np.zeros(nb, np.int32)
    for b in range(nb):
        rows = frames[b][flags[b] != 0]
        kept[b] = rows.shape[0]
        x[b, :rows.size] = rows.ravel()
    return x, kept


def expected(R, frames, flags, L):
    x, kept = compacted(frames, flags)
    return PM.model_hash(R, x, L), kept


def first_bits(words, count):
    """Bits 0 .. count - 1 of each row of uint64 words."""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1, bitorder="little")[..., :count]


_cases = {}


def case(N, B, L):
    """One block per flag pattern: random bytes 0..255 (only & 1 may count), the flags, the
    seeded key string and the model's words and counts; computed once and shared, never
    modified. The calls of a test take their blocks from these."""
    key = (N, B, L)
    if key not in _cases:
        rng = np.random.default_rng(N * 131 + B * 17 + L * 7)
        frames = rng.integers(0, 256, (len(PATTERNS), B, N)).astype(np.uint8)
        flags = np.stack([flags_of(p, B, rng) for p in PATTERNS])
        R = PM.splitmix_words(SEED, PM.key_words(B * N, L))
        want, kept = expected(R, frames, flags, L)
        assert not want[PATTERNS.index("none")].any() and kept[PATTERNS.index("none")] == 0
        assert kept[PATTERNS.index("all")] == B and want[PATTERNS.index("all")].any() or N * B < 8
        if L % 64:
            assert not (want[:, -1] >> np.uint64(L % 64)).any()
        for a in (frames, flags, R, want, kept):
            a.setflags(write=False)
        _cases[key] = dict(frames=frames, flags=flags, R=R, want=want, kept=kept)
    return _cases[key]


def calls_of(n_blocks):
    """Block selections that put different patterns side by side and cover every pattern."""
    return [[(c + i) % len(PATTERNS) for i in range(n_blocks)] for c in range(0, len(PATTERNS), n_blocks)]


def on_device(c, rows):
    N = c["frames"].shape[2]
    return dev(c["frames"][rows].reshape(-1, N)), dev(c["flags"][rows].reshape(-1))


def raw_call(Q, frames_d, keep_d, N, B, L, n_blocks, out_ptr, kept_ptr, scratch, seed=SEED, words=None):
    Nn = Q._native
    Nn.check(Nn.lib().qkd_privacy_amplify_kept_batch(0, frames_d.data_ptr(), n_blocks, N, B, L, seed,
                                                     None if words is None else words.data_ptr(), keep_d.data_ptr(),
                                                     out_ptr, kept_ptr, scratch.data_ptr(), scratch.numel(),
                                                     torch.cuda.current_stream().cuda_stream))


# ---- 1. shapes and flag patterns under each pass count -----------------------------------

SHAPES = [(1, 1, 1, 1), (70, 1, 70, 2), (193, 3, 64, 3), (333, 33, 65, 2), (7, 9, 63, 2), (3, 2500, 64, 2),
          (10240, 33, 4096, 2)]


@pytest.mark.parametrize("cap", [None, 3, 5])
@pytest.mark.parametrize("N,B,L,n_blocks", SHAPES)
def test_shapes_and_patterns(Q, qkd_opt, N, B, L, n_blocks, cap):
    """Words and kept equal the model's; the bits at and above L are zero; kept = NULL (the C
    entry) gives the same words; the seeded and the hash_words form agree."""
    qkd_opt("QKD_PRIVACY_NTT_LOG2", cap)
    c = case(N, B, L)
    wo = (L + 63) // 64
    assert Q.privacy_long_key_words(B * N, L) == c["R"].size
    R_d = words_dev(c["R"])
    for rows in calls_of(n_blocks):
        frames_d, keep_d = on_device(c, rows)
        out, kept = Q.privacy_amplify_kept(frames_d, keep_d, L, frames_per_block=B, hash_seed=SEED)
        assert out.shape == (n_blocks, wo) and out.dtype == torch.int64
        assert kept.shape == (n_blocks,) and kept.dtype == torch.int32
        got = out_host(out)
        assert (kept.cpu().numpy() == c["kept"][rows]).all(), (rows, kept.cpu().numpy(), c["kept"][rows])
        assert (got == c["want"][rows]).all(), rows
        if L % 64:
            assert not (got[:, -1] >> np.uint64(L % 64)).any()
        worded, kept_w = Q.privacy_amplify_kept(frames_d, keep_d, L, frames_per_block=B, hash_seed=1, hash_words=R_d)
        assert (out_host(worded) == c["want"][rows]).all() and (kept_w.cpu().numpy() == c["kept"][rows]).all()
        # kept == NULL
        need = Q.privacy_kept_scratch_bytes(N, B, L, n_blocks)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        raw = torch.full((n_blocks, wo), -1, dtype=torch.int64, device="cuda")
        raw_call(Q, frames_d, keep_d, N, B, L, n_blocks, raw.data_ptr(), None, scratch)
        assert (out_host(raw) == c["want"][rows]).all(), rows


# ---- 2. equalities with the long form ----------------------------------------------------

@pytest.mark.parametrize("N,B,L", [(333, 33, 65), (7, 9, 63), (3, 2500, 64), (10240, 33, 4096)])
def test_all_kept_is_the_long_form(Q, N, B, L):
    c = case(N, B, L)
    row = PATTERNS.index("all")
    frames_d, keep_d = on_device(c, [row])
    out, kept = Q.privacy_amplify_kept(frames_d, keep_d, L, hash_seed=SEED)
    long_form = Q.privacy_amplify_long(frames_d.view(1, B * N), L, hash_seed=SEED)
    assert (out_host(out) == out_host(long_form)).all() and (out_host(out) == c["want"][[row]]).all()
    assert kept.cpu().tolist() == [B]


@pytest.mark.parametrize("N,B,L", [(333, 33, 65), (7, 9, 63), (3, 2500, 64), (10240, 33, 4096)])
def test_prefix_rule_against_the_long_form(Q, N, B, L):
    """The first L' bits equal privacy_amplify_long of the compacted frames alone, at
    n_in = kept * N and out_bits = L', under the same seed and under the first words of the
    same string: for L' = min(L, kept * N) (kept * N itself where that is <= L) and for a
    shorter L'."""
    c = case(N, B, L)
    row = PATTERNS.index("random")
    mask = c["flags"][row] != 0
    k = int(mask.sum())
    assert 0 < k < B and k == c["kept"][row]
    frames_d, keep_d = on_device(c, [row])
    out, kept = Q.privacy_amplify_kept(frames_d, keep_d, L, hash_seed=SEED)
    got = out_host(out)
    assert (got == c["want"][[row]]).all() and kept.cpu().tolist() == [k]
    short = frames_d[torch.from_numpy(mask).cuda()].reshape(1, k * N)
    top = min(L, k * N)
    if N == 7:
        assert top == k * N < L                      # the case "kept * N <= L"
    for lp in sorted({top, max(1, top // 2)}):
        want_bits = first_bits(got, lp)
        seeded = out_host(Q.privacy_amplify_long(short, lp, hash_seed=SEED))
        assert (first_bits(seeded, lp) == want_bits).all(), lp
        words = words_dev(c["R"][:Q.privacy_long_key_words(k * N, lp)])
        worded = out_host(Q.privacy_amplify_long(short, lp, hash_words=words))
        assert (worded == seeded).all(), lp
        assert want_bits.any() or lp < 8


# ---- 3. dropped frames do not matter -------------------------------------------------------

@pytest.mark.parametrize("N,B,L,n_blocks", [(193, 3, 64, 3), (333, 33, 65, 2), (3, 2500, 64, 2)])
def test_dropped_frames_do_not_matter(Q, N, B, L, n_blocks):
    c = case(N, B, L)
    rows = [PATTERNS.index("random"), PATTERNS.index("alternating"), PATTERNS.index("first")][:n_blocks]
    frames = c["frames"][rows].copy()
    flags = c["flags"][rows]
    dropped = flags == 0
    assert dropped.any()
    before = out_host(Q.privacy_amplify_kept(dev(frames.reshape(-1, N)), dev(flags.reshape(-1)), L, frames_per_block=B,
                                             hash_seed=SEED)[0])
    rng = np.random.default_rng(99)
    other = rng.integers(0, 256, frames.shape).astype(np.uint8)
    frames[dropped] = (other[dropped] & 0xFE) | ((frames[dropped] & 1) ^ 1)      # every dropped key bit flipped
    after = out_host(Q.privacy_amplify_kept(dev(frames.reshape(-1, N)), dev(flags.reshape(-1)), L, frames_per_block=B,
                                            hash_seed=SEED)[0])
    assert (before == after).all() and (before == c["want"][rows]).all()


# ---- 4. writes stay in bounds ----------------------------------------------------------------

@pytest.mark.parametrize("N,B,L,n_blocks", [(1, 1, 1, 1), (333, 33, 65, 2), (7, 9, 63, 2), (3, 2500, 64, 2)])
def test_writes_stay_in_bounds(Q, N, B, L, n_blocks):
    """Guard words around out_words and kept, and a scratch of exactly
    privacy_kept_scratch_bytes bytes at an odd address inside one allocation with guard
    bytes on both sides."""
    c = case(N, B, L)
    rows = calls_of(n_blocks)[-1]
    frames_d, keep_d = on_device(c, rows)
    wo, guard = (L + 63) // 64, 64
    out_buf = torch.full((guard + n_blocks * wo + guard,), -1, dtype=torch.int64, device="cuda")
    kept_buf = torch.full((guard + n_blocks + guard,), -1, dtype=torch.int32, device="cuda")
    need = Q.privacy_kept_scratch_bytes(N, B, L, n_blocks)
    alloc = torch.full((1 + need + 4096,), GUARD, dtype=torch.uint8, device="cuda")
    scratch = alloc[1:1 + need]
    assert scratch.data_ptr() % 2 == 1 and scratch.numel() == need
    raw_call(Q, frames_d, keep_d, N, B, L, n_blocks, out_buf.data_ptr() + 8 * guard, kept_buf.data_ptr() + 4 * guard,
             scratch)
    got = out_host(out_buf)
    ones = np.uint64(2**64 - 1)
    assert (got[:guard] == ones).all() and (got[guard + n_blocks * wo:] == ones).all()
    assert (got[guard:guard + n_blocks * wo].reshape(n_blocks, wo) == c["want"][rows]).all()
    k = kept_buf.cpu().numpy()
    assert (k[:guard] == -1).all() and (k[guard + n_blocks:] == -1).all()
    assert (k[guard:guard + n_blocks] == c["kept"][rows]).all()
    a = alloc.cpu().numpy()
    assert a[0] == GUARD and (a[1 + need:] == GUARD).all()
    with pytest.raises(Q.QkdError) as ei:
        Q.privacy_amplify_kept(frames_d, keep_d, L, frames_per_block=B, hash_seed=SEED, scratch=scratch[:need - 1])
    assert ei.value.status == Q._native.ERR_INVALID_ARG and "scratch_bytes" in str(ei.value)


# ---- 5. past 2^20 bits: several strided passes -------------------------------------------------

def test_past_the_short_forms_limit(Q):
    N, B, L = 10240, 103, 192
    assert B * N > 2**20
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (1, B, N)).astype(np.uint8)
    flags = flags_of("random", B, rng, p_keep=0.95)[None]
    R = PM.splitmix_words(SEED, PM.key_words(B * N, L))
    want, kept_want = expected(R, frames, flags, L)              # (the model's row-block form)
    assert 0 < B - kept_want[0] < 16 and want.any()
    out, kept = Q.privacy_amplify_kept(dev(frames.reshape(B, N)), dev(flags[0]), L, hash_seed=SEED)
    assert (out_host(out) == want).all() and kept.cpu().tolist() == kept_want.tolist()


# ---- 6. stream capture ---------------------------------------------------------------------------

def test_stream_capture_follows_the_flags(Q):
    """One call captured in a graph after a warm call; the flags are then changed in place,
    the outputs filled with a guard value and the graph replayed once: words and kept are the
    model's for the NEW flags, so the host never read them."""
    N, B, L, n_blocks = 333, 33, 65, 2
    rng = np.random.default_rng(6)
    frames = rng.integers(0, 256, (n_blocks, B, N)).astype(np.uint8)
    old = np.stack([flags_of("random", B, rng), flags_of("all", B, rng)])
    new = np.stack([flags_of("alternating", B, rng), flags_of("random", B, rng, p_keep=0.5)])
    R = PM.splitmix_words(SEED, PM.key_words(B * N, L))
    want_old, kept_old = expected(R, frames, old, L)
    want_new, kept_new = expected(R, frames, new, L)
    assert (want_old != want_new).any() and (kept_old != kept_new).all()
    frames_d, keep_d = dev(frames.reshape(-1, N)), dev(old.reshape(-1))
    scratch = torch.empty(Q.privacy_kept_scratch_bytes(N, B, L, n_blocks), dtype=torch.uint8, device="cuda")

    def call():
        return Q.privacy_amplify_kept(frames_d, keep_d, L, frames_per_block=B, hash_seed=SEED, scratch=scratch)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm_out, warm_kept = call()
    torch.cuda.current_stream().wait_stream(side)
    assert (out_host(warm_out) == want_old).all() and (warm_kept.cpu().numpy() == kept_old).all()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, kept = call()
    torch.cuda.synchronize()
    keep_d.copy_(dev(new.reshape(-1)))
    for t in (out, kept):
        t.view(torch.uint8).fill_(GUARD)
    graph.replay()
    assert (out_host(out) == want_new).all()
    assert (kept.cpu().numpy() == kept_new).all()
    del graph


# ---- 7. the chain: reconcile -> verify -> privacy amplification ------------------------------------

def test_chain_hashes_only_the_verified_frames(Q):
    """The golden code, 8 frames at QBER 0.02, one of Alice's tags corrupted: Bob's verified
    flags drop exactly that frame, and Bob (corrected bits) and Alice (her frames) hash the
    other seven to the same words, which are not those of all eight."""
    H = Q.HMatrix.from_alist(os.path.join(GOLDEN, "alist_n10240.txt"))
    seeds = torch.from_numpy(np.ascontiguousarray(Q.make_seeds(777, 8), np.uint64).view(np.int64)).cuda()
    alice, bob, q = Q.keygen(H, seeds, 0.02)
    syn = Q.calculate_syndrome(H, alice)
    tags = Q.verify_tags(H, alice, hash_seed=SEED ^ 0x5A5A)     # (its own string, not the privacy hash's)
    tags[3] ^= 1
    r = Q.reconcile(H, bob, syn, float(q[0]), hash_seed=SEED ^ 0x5A5A, alice_tags=tags)
    torch.cuda.synchronize()
    assert r.verified.cpu().tolist() == [1, 1, 1, 0, 1, 1, 1, 1]
    out_bob, kept_bob = Q.privacy_amplify_kept(r.bits, r.verified, 4096, hash_seed=SEED)
    out_alice, kept_alice = Q.privacy_amplify_kept(alice, r.verified, 4096, hash_seed=SEED)
    assert kept_bob.cpu().tolist() == [7] and kept_alice.cpu().tolist() == [7]
    got = out_host(out_bob)
    assert got.shape == (1, 64) and got.any()
    assert (got == out_host(out_alice)).all()
    all8 = out_host(Q.privacy_amplify_kept(alice, torch.ones_like(r.verified), 4096, hash_seed=SEED)[0])
    assert (all8 != got).any()
    # ... and the model agrees with both
    flags = r.verified.cpu().numpy()[None]
    want, _ = expected(PM.splitmix_words(SEED, PM.key_words(8 * 10240, 4096)), alice.cpu().numpy()[None], flags, 4096)
    assert (got == want).all()


# ---- 8. the wrapper's shape checks, on device tensors ----------------------------------------------

def test_wrapper_shape_checks(Q):
    Nn = Q._native
    frames = torch.zeros(6, 8, dtype=torch.uint8, device="cuda")
    keep = torch.ones(6, dtype=torch.uint8, device="cuda")
    words = torch.zeros(Q.privacy_long_key_words(48, 4), dtype=torch.int64, device="cuda")
    out, kept = Q.privacy_amplify_kept(frames, keep, 4, hash_words=words)
    assert out.shape == (1, 1) and out.dtype == torch.int64 and kept.shape == (1,) and kept.dtype == torch.int32
    assert kept.cpu().tolist() == [6] and out.cpu().tolist() == [[0]]
    out, kept = Q.privacy_amplify_kept(frames, keep, 4, frames_per_block=2)
    assert out.shape == (3, 1) and kept.cpu().tolist() == [2, 2, 2]
    assert words.numel() == 1
    bad_calls = [
        dict(frames_per_block=4), dict(frames_per_block=0), dict(frames_per_block=-2), dict(frames_per_block=2.0),
        dict(frames_per_block=12), dict(out_bits=0), dict(out_bits=49), dict(out_bits=17, frames_per_block=2),
        dict(out_bits=4.0), dict(keep=None), dict(keep=keep[:5]), dict(keep=keep.cpu()), dict(keep=keep.to(torch.int32)),
        dict(keep=keep.bool()), dict(hash_words=words.repeat(2)), dict(hash_words=words.cpu()),
        dict(hash_words=words.to(torch.int32)),
        dict(scratch=torch.empty(Q.privacy_kept_scratch_bytes(8, 6, 4, 1) - 1, dtype=torch.uint8, device="cuda")),
        dict(scratch=torch.empty(4096, dtype=torch.uint8)), dict(scratch=torch.empty(4096, dtype=torch.int32, device="cuda")),
        dict(frames=frames[:, :4]), dict(frames=frames[0]), dict(frames=frames[:0]),
    ]
    for bad in bad_calls:
        kw = dict(frames=frames, keep=keep, out_bits=4)
        kw.update(bad)
        with pytest.raises(Q.QkdError) as ei:
            Q.privacy_amplify_kept(**kw)
        assert ei.value.status == Nn.ERR_INVALID_ARG, bad
