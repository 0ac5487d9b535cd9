"""Key verification tags (qkd_verify_key_words, qkd_verify_expand_key,
qkd_verify_tags_batch, qkd_reconcile_verify_batch) at the ABI and wrapper
level, without a GPU: the symbols and their argument counts, the word count
and the seeded key string against known answers and a numpy SplitMix64, the
argument validation, the Python wrappers' tensor checks, and the hash and the
argument checks as a stand-alone host program, plain and under
AddressSanitizer + UBSan."""
import os
import subprocess
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "verify_hash_check.cpp")

GOLDEN_GAMMA = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def N():
    from qkd_ldpc_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        from qkd_ldpc_amd.build import build
        build()
    return _native


def splitmix_words(seed, count):
    """R[k] = mix(seed + (k + 1) * golden) mod 2^64, in numpy uint64 (wrapping)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(count, dtype=np.uint64) + np.uint64(1)) * np.uint64(GOLDEN_GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def test_library_exports_verify(N):
    names = {"qkd_verify_key_words": 1, "qkd_verify_expand_key": 3, "qkd_verify_tags_batch": 8,
             "qkd_reconcile_verify_batch": 20}
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, argc in names.items():
        assert name in N.EXPORTS
        assert name in exported
        assert len(getattr(N.lib(), name).argtypes) == argc, name
    # qkd_reconcile_batch's arguments first, in the same order
    assert (N.lib().qkd_reconcile_verify_batch.argtypes[:13] == N.lib().qkd_reconcile_batch.argtypes[:13])
    assert len(N.lib().qkd_reconcile_batch.argtypes) == 14
    assert N.lib().qkd_abi_version() == 1          # additive change


def test_key_words(N):
    L = N.lib()
    want = {1: 1, 2: 2, 64: 2, 65: 2, 66: 3, 10240: 161, 131072: 2049}
    for n, w in want.items():
        assert w == (n + 63 + 63) // 64            # ceil((N + 63) / 64)
        assert L.qkd_verify_key_words(n) == w, n
    import qkd_ldpc_amd as Q
    assert Q.verify_key_words(10240) == 161


def test_expand_key(N):
    import qkd_ldpc_amd as Q
    r = Q.verify_expand_key(0, 129)
    assert r.dtype == np.uint64 and r.size == 3
    assert [int(x) for x in r] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [int(x) for x in splitmix_words(0, 3)] == [int(x) for x in r]      # the model itself
    for seed in (0xC0FFEE1234567, 2**64 - 1):
        r = Q.verify_expand_key(seed, 10240)
        assert r.size == 161
        assert (r == splitmix_words(seed, 161)).all()
    # exactly W words are written
    buf = np.full(8, 0x5555555555555555, np.uint64)
    assert N.lib().qkd_verify_expand_key(7, 66, buf.ctypes.data) == N.OK
    assert (buf[:3] == splitmix_words(7, 3)).all() and (buf[3:] == 0x5555555555555555).all()
    assert N.lib().qkd_verify_expand_key(7, 66, None) == N.ERR_INVALID_ARG
    assert N.lib().qkd_verify_expand_key(7, 0, buf.ctypes.data) == N.ERR_INVALID_ARG


def test_verify_tags_null_arguments(N):
    """NULL code or arrays, tag_bits 0 and 65: QKD_ERR_INVALID_ARG before anything
    touches a device (the code pointer is never dereferenced)."""
    L = N.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    fake_code = p

    def call(code, bits, tags, t=64, frames=1):
        return L.qkd_verify_tags_batch(code, bits, frames, 5, None, t, tags, None)

    assert call(None, p, p) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()
    assert call(fake_code, None, p) == N.ERR_INVALID_ARG
    assert call(fake_code, p, None) == N.ERR_INVALID_ARG
    assert call(fake_code, p, p, t=0) == N.ERR_INVALID_ARG
    assert "tag_bits" in N.last_error()
    assert call(fake_code, p, p, t=65) == N.ERR_INVALID_ARG
    assert call(fake_code, p, p, frames=0) == N.ERR_INVALID_ARG


def test_reconcile_verify_null_arguments(N):
    L = N.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    fake_code = p          # never dereferenced: every call below is rejected first

    def call(code=fake_code, bob=p, syn=p, bits=p, iters=p, ok=p, t=64, alice=p, tags=p, ver=p):
        return L.qkd_reconcile_verify_batch(code, None, bob, syn, 1, 0.02, 50, 100.0, N.FLAG_THRESHOLD,
                                            bits, iters, ok, None, 5, None, t, alice, tags, ver, None)

    for kw in ("code", "bob", "syn", "bits", "iters", "ok"):
        assert call(**{kw: None}) == N.ERR_INVALID_ARG, kw
        assert "null" in N.last_error()
    assert call(t=0) == N.ERR_INVALID_ARG
    assert "tag_bits" in N.last_error()
    assert call(t=65) == N.ERR_INVALID_ARG
    assert call(ver=None) == N.ERR_INVALID_ARG                     # alice_tags without verified
    assert "verified" in N.last_error()
    assert call(ver=None, tags=None) == N.ERR_INVALID_ARG
    assert call(alice=None, tags=None, ver=None) == N.ERR_INVALID_ARG      # nothing to give or compare
    assert "neither" in N.last_error()
    assert call(alice=None, tags=None) == N.ERR_INVALID_ARG


def test_verify_wrappers_reject_host_tensors_and_dtypes(N):
    import torch
    import qkd_ldpc_amd as Q
    for name in ("verify_key_words", "verify_expand_key", "verify_tags"):
        assert name in Q.__all__
    H = types.SimpleNamespace(num_bit_nodes=8, num_check_nodes=4, device=0, handle=None)
    bits = torch.zeros(2, 8, dtype=torch.uint8)
    for b in (bits, bits.numpy(), bits.double(), bits.to(torch.int32), None):
        with pytest.raises(Q.QkdError) as ei:
            Q.verify_tags(H, b)
        assert ei.value.status == N.ERR_INVALID_ARG
    syn = torch.zeros(2, 4, dtype=torch.uint8)
    with pytest.raises(Q.QkdError) as ei:
        Q.reconcile(H, bits, syn, 0.02, alice_tags=torch.zeros(2, dtype=torch.int64))
    assert ei.value.status == N.ERR_INVALID_ARG
    # the tag and key-string checks themselves: host tensors, wrong dtypes, wrong counts
    for t in (torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.float64), np.zeros(2, np.uint64), [1, 2]):
        with pytest.raises(Q.QkdError) as ei:
            Q._need_tags(t, 2, "alice_tags", H)
        assert ei.value.status == N.ERR_INVALID_ARG
    with pytest.raises(Q.QkdError):
        Q._verify_key(H, 0, torch.zeros(2, dtype=torch.int64))
    assert Q._verify_key(H, None, None) == (0, None)
    assert Q._verify_key(H, -1, None) == (2**64 - 1, None)
    r = Q.ReconcileResult(1, 2, 3, 4)
    assert r.tags is None and r.verified is None


@pytest.mark.gpu
def test_verify_wrappers_reject_dtypes_and_shapes(golden_code):
    import torch
    import qkd_ldpc_amd as Q
    g = golden_code
    H = Q.HMatrix.from_check_lists(10240, g["chk_off"], g["chk_idx"])
    bits = torch.zeros(4, 10240, dtype=torch.uint8, device="cuda")
    syn = torch.zeros(4, 5231, dtype=torch.uint8, device="cuda")
    tags = torch.zeros(4, dtype=torch.int64, device="cuda")
    words = torch.zeros(161, dtype=torch.int64, device="cuda")
    cases = [
        lambda: Q.verify_tags(H, bits.cpu()),
        lambda: Q.verify_tags(H, bits.to(torch.int32)),
        lambda: Q.verify_tags(H, bits[:, :10239]),
        lambda: Q.verify_tags(H, bits, tag_bits=0),
        lambda: Q.verify_tags(H, bits, tag_bits=65),
        lambda: Q.verify_tags(H, bits, hash_words=words[:160]),                 # W - 1 words
        lambda: Q.verify_tags(H, bits, hash_words=words.cpu()),
        lambda: Q.verify_tags(H, bits, hash_words=words.to(torch.float64)),
        lambda: Q.reconcile(H, bits, syn, 0.02, alice_tags=tags[:3]),           # F - 1 tags
        lambda: Q.reconcile(H, bits, syn, 0.02, alice_tags=tags.cpu()),
        lambda: Q.reconcile(H, bits, syn, 0.02, alice_tags=tags.to(torch.int32)),
        lambda: Q.reconcile(H, bits, syn, 0.02, alice_tags=tags, tag_bits=0),
        lambda: Q.reconcile(H, bits, syn, 0.02, want_tags=True, tag_bits=65),
        lambda: Q.reconcile(H, bits, syn, 0.02, hash_seed=1, hash_words=words[:5]),
    ]
    for call in cases:
        with pytest.raises(Q.QkdError) as ei:
            call()
        assert ei.value.status == Q._native.ERR_INVALID_ARG
    torch.cuda.synchronize()


# ---- the hash and the argument checks, stand-alone -----------------------------------

def _build(tmp_path_factory, name, extra):
    out = str(tmp_path_factory.mktemp("native") / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-o", out, SRC])
    return out


def _run(binary):
    r = subprocess.run([binary], text=True, capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0", r.stdout + r.stderr


def test_verify_hash_check(tmp_path_factory):
    _run(_build(tmp_path_factory, "verify_hash_check", []))


def test_verify_hash_check_sanitized(tmp_path_factory):
    _run(_build(tmp_path_factory, "verify_hash_check_san",
                ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]))
