"""Privacy amplification of the kept frames of a block (qkd_privacy_kept_scratch_bytes,
qkd_privacy_amplify_kept_batch) at the ABI and wrapper level, without a GPU: the symbols and
their argument counts, the scratch size against the long form's plus the documented tables,
the argument validation, the Python wrapper's tensor and shape checks, and the index
arithmetic the kernels share with the host (the reciprocal division, a lane's positions, the
scan's list, the gathered input and the prefix rule) with the argument check as a stand-alone
host program, plain and under AddressSanitizer + UBSan."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "privacy_kept_check.cpp")


@pytest.fixture(scope="module")
def N():
    from qkd_ldpc_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        from qkd_ldpc_amd.build import build
        build()
    return _native


def test_library_exports_privacy_kept(N):
    names = {"qkd_privacy_kept_scratch_bytes": 4, "qkd_privacy_amplify_kept_batch": 14}
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, argc in names.items():
        assert name in N.EXPORTS
        assert name in exported
        assert len(getattr(N.lib(), name).argtypes) == argc, name
    assert N.lib().qkd_abi_version() == 1          # additive change


def test_kept_scratch_bytes(N):
    """The long form's bytes for a block of B * N bits, 4 bytes per frame of the call, a byte
    per block and 16 bytes of slack; 0 outside the range."""
    L = N.lib()
    import qkd_ldpc_amd as Q
    for n, b, bits, blocks in ((1, 1, 1, 1), (70, 1, 70, 2), (193, 3, 64, 3), (333, 33, 65, 2), (7, 9, 63, 2),
                               (3, 2500, 64, 2), (10240, 33, 4096, 2), (10240, 103, 192, 1),
                               (10240, 9765, 34 * 10**6, 1), (1, 2**27, 1, 1), (2**26 + 1, 1, 2**26, 5),
                               (1, 1, 1, 2**32 - 1), (7, 9, 63, (2**32 - 1) // 9)):
        base = L.qkd_privacy_long_scratch_bytes(n * b, bits)
        assert base > 0, (n, b, bits)
        got = L.qkd_privacy_kept_scratch_bytes(n, b, bits, blocks)
        assert got == base + 4 * blocks * b + blocks + 16, (n, b, bits, blocks)
        assert Q.privacy_kept_scratch_bytes(n, b, bits, blocks) == got
    # the size follows n_blocks, which the long form's does not
    assert L.qkd_privacy_kept_scratch_bytes(10240, 33, 4096, 3) - L.qkd_privacy_kept_scratch_bytes(10240, 33, 4096, 2) \
        == 4 * 33 + 1
    assert Q.privacy_kept_scratch_bytes(10240, 33, 4096) == Q.privacy_kept_scratch_bytes(10240, 33, 4096, 1)
    for n, b, bits, blocks in ((65536, 65536, 1, 1),             # B * N = 2^32: zero in 32 bits
                               (2**31, 2, 1, 1), (2**32 - 1, 2**32 - 1, 1, 1), (2**27 + 1, 1, 1, 1),
                               (1, 2**27 + 1, 1, 1), (3, 2**27 // 3 + 1, 1, 1), (0, 5, 1, 1), (5, 0, 1, 1),
                               (7, 9, 0, 1), (7, 9, 64, 1), (2**26, 2, 2, 1), (2**26 + 1, 1, 2**26 + 1, 1),
                               (7, 9, 63, 0), (7, 9, 63, 2**32), (7, 9, 63, (2**32 - 1) // 9 + 1), (7, 9, 63, 2**64 - 1),
                               (1, 1, 1, 2**32)):
        assert L.qkd_privacy_kept_scratch_bytes(n, b, bits, blocks) == 0, (n, b, bits, blocks)
        assert Q.privacy_kept_scratch_bytes(n, b, bits, blocks) == 0
    for bad in ((-1, 1, 1, 1), (1, 2**32, 1, 1), (1, 1, 1, -1), (1, 1, 1, 2**64), (1.0, 1, 1, 1)):
        assert Q.privacy_kept_scratch_bytes(*bad) == 0


def test_amplify_kept_null_and_limit_arguments(N):
    """Every clause of the validation: QKD_ERR_INVALID_ARG with a message naming the
    argument, before anything touches a device (this runs where there is none)."""
    L = N.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    need = L.qkd_privacy_kept_scratch_bytes(4, 2, 8, 1)
    assert need > 0

    def call(frames=p, blocks=1, n=4, b=2, bits=8, keep=p, out=p, kept=p, scratch=p, sbytes=need, device=0):
        return L.qkd_privacy_amplify_kept_batch(device, frames, blocks, n, b, bits, 5, None, keep, out, kept, scratch,
                                                sbytes, None)

    def refused(word, **kw):
        assert call(**kw) == N.ERR_INVALID_ARG, kw
        assert word in N.last_error(), (kw, N.last_error())

    for bad in (dict(frames=None), dict(keep=None), dict(out=None), dict(scratch=None)):
        refused("null", **bad)
    refused("n_blocks must be > 0", blocks=0)
    refused("below 2^32", blocks=2**32, b=1)
    refused("below 2^32", blocks=2**31)                        # n_blocks * B = 2^32
    refused("below 2^32", blocks=2**64 - 1)
    refused("must be >= 1", n=0)
    refused("must be >= 1", b=0)
    big = L.qkd_privacy_kept_scratch_bytes(2**26 + 1, 1, 2**26, 1)
    assert big > 2**30
    refused("frame_bits * frames_per_block must be in", n=65536, b=65536, bits=1, sbytes=big)      # 2^32 in 64 bits
    refused("frame_bits * frames_per_block must be in", n=2**32 - 1, b=2**32 - 1, bits=1, sbytes=big)
    refused("frame_bits * frames_per_block must be in", n=2**27 + 1, b=1, bits=1, sbytes=big)
    refused("frame_bits * frames_per_block must be in", n=10240, b=13108, bits=1, sbytes=big)       # 2^27 + 5632
    refused("out_bits must be in", bits=0)
    refused("out_bits must be in", bits=9)
    refused("+ out_bits - 1 exceeds", n=2**26, b=2, bits=2, sbytes=big)
    refused("+ out_bits - 1 exceeds", n=2**26 + 1, b=1, bits=2**26 + 1, sbytes=big)
    refused("scratch_bytes", sbytes=need - 1)
    refused("scratch_bytes", sbytes=0)
    refused("scratch_bytes", sbytes=L.qkd_privacy_long_scratch_bytes(8, 8))       # the long form's is too small
    refused("scratch_bytes", blocks=2, n=2, sbytes=L.qkd_privacy_kept_scratch_bytes(2, 2, 4, 2) - 1, bits=4)
    refused("scratch_bytes", n=2**26 + 1, b=1, bits=2**26, sbytes=big - 1)
    if L.qkd_device_count() > 0:
        refused("device", device=-1)
    else:
        # kept may be NULL: with everything else in order the call gets past the validation
        # (never where there is a device: these are host addresses)
        assert call(kept=None) == N.ERR_DEVICE


def test_privacy_kept_wrapper_checks(N):
    """The wrapper's own checks need no device: tensors on the host, wrong dtypes and shapes,
    a frame count the block size does not divide."""
    import torch
    import qkd_ldpc_amd as Q
    for name in ("privacy_kept_scratch_bytes", "privacy_amplify_kept"):
        assert name in Q.__all__
    frames = torch.zeros(6, 8, dtype=torch.uint8)
    keep = torch.ones(6, dtype=torch.uint8)
    for f in (frames, frames.numpy(), frames.double(), frames.to(torch.int32), None):
        with pytest.raises(Q.QkdError) as ei:
            Q.privacy_amplify_kept(f, keep, 4)
        assert ei.value.status == N.ERR_INVALID_ARG
    with pytest.raises(Q.QkdError) as ei:
        Q.privacy_amplify_kept(frames, keep, 4, frames_per_block=4)
    assert ei.value.status == N.ERR_INVALID_ARG


# ---- the index arithmetic and the argument check, stand-alone ---------------------------

def _build(tmp_path_factory, name, extra):
    out = str(tmp_path_factory.mktemp("native") / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-o", out, SRC])
    return out


def _run(binary):
    r = subprocess.run([binary], text=True, capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0", r.stdout + r.stderr


def test_privacy_kept_check(tmp_path_factory):
    _run(_build(tmp_path_factory, "privacy_kept_check", []))


def test_privacy_kept_check_sanitized(tmp_path_factory):
    _run(_build(tmp_path_factory, "privacy_kept_check_san",
                ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]))
