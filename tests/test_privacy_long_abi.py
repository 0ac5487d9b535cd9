"""Long-block privacy amplification (qkd_privacy_long_key_words,
qkd_privacy_long_expand_key, qkd_privacy_long_scratch_bytes,
qkd_privacy_amplify_long_batch) at the ABI and wrapper level, without a GPU: the
symbols and their argument counts, the word count against known answers, the seeded
key string against the short form's, the scratch size, the argument validation, the
debug option, the Python wrapper's tensor checks, and the modular arithmetic, the hash
by transforms and the argument check as a stand-alone host program, plain and under
AddressSanitizer + UBSan."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ntt_mod_check.cpp")


@pytest.fixture(scope="module")
def N():
    from qkd_ldpc_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        from qkd_ldpc_amd.build import build
        build()
    return _native


def test_library_exports_privacy_long(N):
    names = {"qkd_privacy_long_key_words": 2, "qkd_privacy_long_expand_key": 4, "qkd_privacy_long_scratch_bytes": 2,
             "qkd_privacy_amplify_long_batch": 12}
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, argc in names.items():
        assert name in N.EXPORTS
        assert name in exported
        assert len(getattr(N.lib(), name).argtypes) == argc, name
    assert N.lib().qkd_abi_version() == 1          # additive change


def test_long_key_words(N):
    L = N.lib()
    want = [(1, 1, 1), (2**20 + 1, 1, 16385), (2**26 + 1, 2**26, 2**21), (2**27, 1, 2**21), (2**27, 2, 0), (5, 6, 0),
            (0, 1, 0)]
    for n_in, bits, w in want:
        assert L.qkd_privacy_long_key_words(n_in, bits) == w, (n_in, bits)
    assert L.qkd_privacy_key_words(2**20 + 1, 1) == 0          # the short form keeps its limit
    import qkd_ldpc_amd as Q
    for n_in, bits, w in want:
        assert Q.privacy_long_key_words(n_in, bits) == w, (n_in, bits)
    assert Q.privacy_long_key_words(-1, 1) == 0 and Q.privacy_long_key_words(2**32, 1) == 0


def test_long_expand_key(N):
    import qkd_ldpc_amd as Q
    for seed, n_in, bits in ((0, 129, 64), (0xC0FFEE1234567, 10240, 4096), (2**64 - 1, 2**20, 2**20), (7, 1, 1)):
        r = Q.privacy_long_expand_key(seed, n_in, bits)
        assert r.dtype == np.uint64 and r.size == Q.privacy_key_words(n_in, bits)
        assert (r == Q.privacy_expand_key(seed, n_in, bits)).all()
    # past the short form's range: the same counter form, longer
    r = Q.privacy_long_expand_key(5, 2**20 + 77, 192)
    assert r.size == (2**20 + 77 + 192 - 1 + 63) // 64
    assert r.size == 16389 and (r == Q.privacy_expand_key(5, 2**20, 2**20)[:r.size]).all()
    # exactly Wp words are written
    buf = np.full(8, 0x5555555555555555, np.uint64)
    assert N.lib().qkd_privacy_long_expand_key(7, 100, 93, buf.ctypes.data) == N.OK
    assert (buf[:3] == Q.privacy_expand_key(7, 100, 93)).all() and (buf[3:] == 0x5555555555555555).all()
    assert N.lib().qkd_privacy_long_expand_key(7, 100, 93, None) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()
    for n_in, bits in ((0, 1), (5, 6), (5, 0), (2**27, 2), (2**27 + 1, 1)):
        assert N.lib().qkd_privacy_long_expand_key(7, n_in, bits, buf.ctypes.data) == N.ERR_INVALID_ARG, (n_in, bits)
        assert "out_bits" in N.last_error()
        with pytest.raises(Q.QkdError) as ei:
            Q.privacy_long_expand_key(7, n_in, bits)
        assert ei.value.status == N.ERR_INVALID_ARG
    assert (buf[3:] == 0x5555555555555555).all()


def test_long_scratch_bytes(N):
    L = N.lib()
    import qkd_ldpc_amd as Q
    for n_in, bits in ((0, 1), (5, 6), (5, 0), (2**27, 2), (2**27 + 1, 1), (2**26 + 1, 2**26 + 1)):
        assert L.qkd_privacy_long_scratch_bytes(n_in, bits) == 0, (n_in, bits)
        assert Q.privacy_long_scratch_bytes(n_in, bits) == 0
    for n_in, bits in ((1, 1), (70, 70), (2**20 + 1, 1), (2**26 + 1, 2**26), (2**27, 1), (10**8, 34 * 10**6)):
        t = 64
        while t < n_in + bits - 1:
            t *= 2
        got = L.qkd_privacy_long_scratch_bytes(n_in, bits)
        assert got == Q.privacy_long_scratch_bytes(n_in, bits)
        assert 8 * t < got <= 8 * t + 8 * 2**14 + 16, (n_in, bits)      # two arrays of T residues and a small table
    assert Q.privacy_long_scratch_bytes(-1, 1) == 0


def test_amplify_long_null_and_limit_arguments(N):
    """NULL arrays, no blocks, sizes outside the range and a short scratch:
    QKD_ERR_INVALID_ARG naming the argument, before anything touches a device."""
    L = N.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    need = L.qkd_privacy_long_scratch_bytes(8, 8)
    assert need > 0

    def call(keys=p, blocks=1, n_in=8, bits=8, out=p, scratch=p, sbytes=need, device=0):
        return L.qkd_privacy_amplify_long_batch(device, keys, blocks, n_in, bits, 5, None, None, out, scratch, sbytes,
                                                None)

    for bad in (dict(keys=None), dict(out=None), dict(scratch=None)):
        assert call(**bad) == N.ERR_INVALID_ARG
        assert "null" in N.last_error()
    assert call(blocks=0) == N.ERR_INVALID_ARG
    assert "n_blocks" in N.last_error()
    assert call(blocks=2**32) == N.ERR_INVALID_ARG
    assert "n_blocks" in N.last_error()
    big = L.qkd_privacy_long_scratch_bytes(2**26 + 1, 2**26)
    assert call(n_in=0, bits=0, sbytes=big) == N.ERR_INVALID_ARG
    assert "n_in" in N.last_error()
    assert call(n_in=2**27 + 1, bits=1, sbytes=big) == N.ERR_INVALID_ARG
    assert "n_in" in N.last_error()
    assert call(n_in=2**27, bits=2, sbytes=big) == N.ERR_INVALID_ARG
    assert "n_in + out_bits - 1" in N.last_error()
    assert call(bits=0) == N.ERR_INVALID_ARG
    assert "out_bits" in N.last_error()
    assert call(bits=9) == N.ERR_INVALID_ARG
    assert "out_bits" in N.last_error()
    assert call(sbytes=need - 1) == N.ERR_INVALID_ARG
    assert "scratch_bytes" in N.last_error()
    assert call(n_in=2**26 + 1, bits=2**26, sbytes=big - 1) == N.ERR_INVALID_ARG
    assert "scratch_bytes" in N.last_error()
    if L.qkd_device_count() > 0:
        assert call(device=-1) == N.ERR_INVALID_ARG
        assert "device" in N.last_error()


def test_privacy_ntt_option_is_known(N):
    L = N.lib()
    for v in (b"3", b"5", b"13", None):
        assert L.qkd_debug_set_option(None, b"QKD_PRIVACY_NTT_LOG2", v) == N.OK
    assert L.qkd_debug_set_option(None, b"QKD_PRIVACY_NTT", b"3") == N.ERR_INVALID_ARG


def test_privacy_long_wrapper_rejects_host_tensors_and_dtypes(N):
    import torch
    import qkd_ldpc_amd as Q
    for name in ("privacy_long_key_words", "privacy_long_expand_key", "privacy_long_scratch_bytes",
                 "privacy_amplify_long"):
        assert name in Q.__all__
    keys = torch.zeros(2, 8, dtype=torch.uint8)
    for k in (keys, keys.numpy(), keys.double(), keys.to(torch.int32), None):
        with pytest.raises(Q.QkdError) as ei:
            Q.privacy_amplify_long(k, 4)
        assert ei.value.status == N.ERR_INVALID_ARG


# ---- the arithmetic, the hash by transforms and the argument check, stand-alone -------

def _build(tmp_path_factory, name, extra):
    out = str(tmp_path_factory.mktemp("native") / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-o", out, SRC])
    return out


def _run(binary):
    r = subprocess.run([binary], text=True, capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0", r.stdout + r.stderr


def test_ntt_mod_check(tmp_path_factory):
    _run(_build(tmp_path_factory, "ntt_mod_check", []))


def test_ntt_mod_check_sanitized(tmp_path_factory):
    _run(_build(tmp_path_factory, "ntt_mod_check_san",
                ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]))
