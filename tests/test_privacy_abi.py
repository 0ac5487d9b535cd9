"""Privacy amplification (qkd_privacy_key_words, qkd_privacy_expand_key,
qkd_privacy_amplify_batch) at the ABI and wrapper level, without a GPU: the
symbols and their argument counts, the word count against known answers, the
seeded key string against a numpy SplitMix64, the argument validation, the
Python wrapper's tensor checks, and the hash and the argument check as a
stand-alone host program, plain and under AddressSanitizer + UBSan."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "privacy_hash_check.cpp")


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
        z = np.uint64(seed) + (np.arange(count, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def test_library_exports_privacy(N):
    names = {"qkd_privacy_key_words": 2, "qkd_privacy_expand_key": 4, "qkd_privacy_amplify_batch": 10}
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, argc in names.items():
        assert name in N.EXPORTS
        assert name in exported
        assert len(getattr(N.lib(), name).argtypes) == argc, name
    assert N.lib().qkd_abi_version() == 1          # additive change


def test_key_words(N):
    L = N.lib()
    want = [(1, 1, 1), (64, 1, 1), (64, 2, 2), (10240, 64, 161), (0, 1, 0), (5, 6, 0), (2**20 + 1, 1, 0)]
    for n_in, bits, w in want:
        assert L.qkd_privacy_key_words(n_in, bits) == w, (n_in, bits)
    assert L.qkd_privacy_key_words(2**20, 2**20) == 32768
    assert L.qkd_privacy_key_words(10240, 64) == L.qkd_verify_key_words(10240)
    import qkd_ldpc_amd as Q
    assert Q.privacy_key_words(10240, 4096) == (10240 + 4096 - 1 + 63) // 64
    assert Q.privacy_key_words(5, 6) == 0 and Q.privacy_key_words(-1, 1) == 0


def test_expand_key(N):
    import qkd_ldpc_amd as Q
    r = Q.privacy_expand_key(0, 129, 64)
    assert r.dtype == np.uint64 and r.size == 3
    assert [int(x) for x in r] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    for seed in (0xC0FFEE1234567, 2**64 - 1):
        r = Q.privacy_expand_key(seed, 10240, 4096)
        assert r.size == 224
        assert (r == splitmix_words(seed, 224)).all()
        assert (r[:161] == Q.verify_expand_key(seed, 10240)).all()      # the same counter form
    # exactly Wp words are written
    buf = np.full(8, 0x5555555555555555, np.uint64)
    assert N.lib().qkd_privacy_expand_key(7, 100, 93, buf.ctypes.data) == N.OK
    assert (buf[:3] == splitmix_words(7, 3)).all() and (buf[3:] == 0x5555555555555555).all()
    assert N.lib().qkd_privacy_expand_key(7, 100, 93, None) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()
    for n_in, bits in ((0, 1), (5, 6), (5, 0), (2**20 + 1, 1)):
        assert N.lib().qkd_privacy_expand_key(7, n_in, bits, buf.ctypes.data) == N.ERR_INVALID_ARG, (n_in, bits)
        assert "out_bits" in N.last_error()
        with pytest.raises(Q.QkdError) as ei:
            Q.privacy_expand_key(7, n_in, bits)
        assert ei.value.status == N.ERR_INVALID_ARG
    assert (buf[3:] == 0x5555555555555555).all()


def test_amplify_null_and_limit_arguments(N):
    """NULL arrays, no frames and sizes outside 1 <= out_bits <= n_in <= 2^20:
    QKD_ERR_INVALID_ARG with a message, before anything touches a device."""
    L = N.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data

    def call(keys=p, frames=1, n_in=8, bits=8, out=p, device=0):
        return L.qkd_privacy_amplify_batch(device, keys, frames, n_in, bits, 5, None, None, out, None)

    assert call(keys=None) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()
    assert call(out=None) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()
    assert call(frames=0) == N.ERR_INVALID_ARG
    assert "n_frames" in N.last_error()
    assert call(frames=2**32) == N.ERR_INVALID_ARG
    assert "n_frames" in N.last_error()
    assert call(n_in=0, bits=0) == N.ERR_INVALID_ARG
    assert "n_in" in N.last_error()
    assert call(n_in=2**20 + 1, bits=1) == N.ERR_INVALID_ARG
    assert "n_in" in N.last_error()
    assert call(bits=0) == N.ERR_INVALID_ARG
    assert "out_bits" in N.last_error()
    assert call(bits=9) == N.ERR_INVALID_ARG
    assert "out_bits" in N.last_error()
    if L.qkd_device_count() > 0:
        assert call(device=-1) == N.ERR_INVALID_ARG
        assert "device" in N.last_error()


def test_privacy_kernel_option_is_known(N):
    L = N.lib()
    for v in (b"direct", b"table", None):
        assert L.qkd_debug_set_option(None, b"QKD_PRIVACY_KERNEL", v) == N.OK


def test_privacy_wrapper_rejects_host_tensors_and_dtypes(N):
    import torch
    import qkd_ldpc_amd as Q
    for name in ("privacy_key_words", "privacy_expand_key", "privacy_amplify"):
        assert name in Q.__all__
    keys = torch.zeros(2, 8, dtype=torch.uint8)
    for k in (keys, keys.numpy(), keys.double(), keys.to(torch.int32), None):
        with pytest.raises(Q.QkdError) as ei:
            Q.privacy_amplify(k, 4)
        assert ei.value.status == N.ERR_INVALID_ARG


@pytest.mark.gpu
def test_privacy_wrapper_rejects_dtypes_and_shapes():
    import torch
    import qkd_ldpc_amd as Q
    keys = torch.zeros(4, 333, dtype=torch.uint8, device="cuda")
    wp = Q.privacy_key_words(333, 65)
    assert wp == 7
    words = torch.zeros(wp, dtype=torch.int64, device="cuda")
    keep = torch.ones(4, dtype=torch.uint8, device="cuda")
    cases = [
        lambda: Q.privacy_amplify(keys.cpu(), 65),
        lambda: Q.privacy_amplify(keys.to(torch.int32), 65),
        lambda: Q.privacy_amplify(keys[:, :300], 65),                           # rows not contiguous
        lambda: Q.privacy_amplify(keys.view(-1), 65),                           # not [F, n_in]
        lambda: Q.privacy_amplify(keys.view(2, 2, 333), 65),
        lambda: Q.privacy_amplify(keys[:0], 65),                                # no frames
        lambda: Q.privacy_amplify(keys, 0),
        lambda: Q.privacy_amplify(keys, 334),
        lambda: Q.privacy_amplify(keys, 65.0),
        lambda: Q.privacy_amplify(keys, 65, hash_words=words[:wp - 1]),         # Wp - 1 words
        lambda: Q.privacy_amplify(keys, 65, hash_words=words.cpu()),
        lambda: Q.privacy_amplify(keys, 65, hash_words=words.to(torch.float64)),
        lambda: Q.privacy_amplify(keys, 65, keep=keep[:3]),                     # F - 1 flags
        lambda: Q.privacy_amplify(keys, 65, keep=keep.cpu()),
        lambda: Q.privacy_amplify(keys, 65, keep=keep.to(torch.int32)),
    ]
    for k, call in enumerate(cases):
        with pytest.raises(Q.QkdError) as ei:
            call()
        assert ei.value.status == Q._native.ERR_INVALID_ARG, k
    out = Q.privacy_amplify(keys, 65, hash_words=words, keep=keep)
    torch.cuda.synchronize()
    assert out.shape == (4, 2) and out.dtype == torch.int64 and not out.any()


# ---- the hash and the argument check, stand-alone ------------------------------------

def _build(tmp_path_factory, name, extra):
    out = str(tmp_path_factory.mktemp("native") / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-o", out, SRC])
    return out


def _run(binary):
    r = subprocess.run([binary], text=True, capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0", r.stdout + r.stderr


def test_privacy_hash_check(tmp_path_factory):
    _run(_build(tmp_path_factory, "privacy_hash_check", []))


def test_privacy_hash_check_sanitized(tmp_path_factory):
    _run(_build(tmp_path_factory, "privacy_hash_check_san",
                ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]))
