"""qkd_reconcile_batch (Bob-side reconciliation from a received syndrome) at the
ABI and wrapper level, without a GPU: the symbol, its argument validation, the
Python wrapper's tensor checks, and the host-only argument check as a
stand-alone program, plain and under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "reconcile_args_check.cpp")


@pytest.fixture(scope="module")
def N():
    from qkd_ldpc_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        from qkd_ldpc_amd.build import build
        build()
    return _native


def test_library_exports_reconcile(N):
    assert "qkd_reconcile_batch" in N.EXPORTS
    assert hasattr(N.lib(), "qkd_reconcile_batch")
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    assert any(line.split()[-1] == "qkd_reconcile_batch" and " T " in line for line in out.splitlines())
    assert len(N.lib().qkd_reconcile_batch.argtypes) == 14
    assert N.lib().qkd_abi_version() == 1          # additive change


def test_reconcile_null_arguments(N):
    """NULL code or NULL arrays: QKD_ERR_INVALID_ARG before anything touches a device."""
    L = N.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    fake_code = p          # never dereferenced: every call below has a NULL array

    def call(code, bob, syn, bits, iters, ok):
        return L.qkd_reconcile_batch(code, None, bob, syn, 1, 0.02, 50, 100.0, N.FLAG_THRESHOLD,
                                     bits, iters, ok, None, None)

    assert call(None, p, p, p, p, p) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()
    assert call(fake_code, None, p, p, p, p) == N.ERR_INVALID_ARG
    assert call(fake_code, p, None, p, p, p) == N.ERR_INVALID_ARG
    assert call(fake_code, p, p, None, p, p) == N.ERR_INVALID_ARG      # bits_out is required
    assert call(fake_code, p, p, p, None, p) == N.ERR_INVALID_ARG
    assert call(fake_code, p, p, p, p, None) == N.ERR_INVALID_ARG
    assert call(None, None, None, None, None, None) == N.ERR_INVALID_ARG


def test_reconcile_wrapper_rejects_host_tensors(N):
    import torch
    import qkd_ldpc_amd as Q
    assert "reconcile" in Q.__all__ and "ReconcileResult" in Q.__all__
    H = types.SimpleNamespace(num_bit_nodes=8, num_check_nodes=4, device=0, handle=None)
    bob = torch.zeros(2, 8, dtype=torch.uint8)
    syn = torch.zeros(2, 4, dtype=torch.uint8)
    for b, s in [(bob, syn), (bob.numpy(), syn.numpy()), (bob.double(), syn), (None, syn)]:
        with pytest.raises(Q.QkdError) as ei:
            Q.reconcile(H, b, s, 0.02)
        assert ei.value.status == N.ERR_INVALID_ARG


@pytest.mark.gpu
def test_reconcile_wrapper_rejects_dtypes_and_shapes(golden_code):
    import torch
    import qkd_ldpc_amd as Q
    g = golden_code
    H = Q.HMatrix.from_check_lists(10240, g["chk_off"], g["chk_idx"])
    bob = torch.zeros(4, 10240, dtype=torch.uint8, device="cuda")
    syn = torch.zeros(4, 5231, dtype=torch.uint8, device="cuda")
    cases = [
        lambda: Q.reconcile(H, bob.cpu(), syn, 0.02),                       # host bob
        lambda: Q.reconcile(H, bob, syn.cpu(), 0.02),                       # host syndrome
        lambda: Q.reconcile(H, bob.to(torch.int32), syn, 0.02),             # wrong dtype
        lambda: Q.reconcile(H, bob, syn.to(torch.float64), 0.02),
        lambda: Q.reconcile(H, bob, syn[:3], 0.02),                         # fewer syndromes than keys
        lambda: Q.reconcile(H, bob[:, :10239], syn, 0.02),                  # not contiguous, wrong width
        lambda: Q.reconcile(H, bob.view(-1)[:-5], syn, 0.02),               # not a multiple of N
        lambda: Q.reconcile(H, bob, syn.view(-1)[:4 * 5230], 0.02),         # flat, wrong width
        lambda: Q.reconcile(H, syn, bob, 0.02),                             # swapped
        lambda: Q.reconcile(H, bob, syn, 0.0),                              # QBER outside (0, 1)
        lambda: Q.reconcile(H, bob, syn, 1.0),
        lambda: Q.reconcile(H, bob, syn, 0.02, max_iterations=0),
    ]
    for call in cases:
        with pytest.raises(Q.QkdError) as ei:
            call()
        assert ei.value.status == Q._native.ERR_INVALID_ARG
    torch.cuda.synchronize()


# ---- the host-only argument check, stand-alone ---------------------------------------

def _build(tmp_path_factory, name, extra):
    out = str(tmp_path_factory.mktemp("native") / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-o", out, SRC])
    return out


def _run(binary):
    r = subprocess.run([binary], text=True, capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0", r.stdout + r.stderr


def test_reconcile_args_check(tmp_path_factory):
    _run(_build(tmp_path_factory, "reconcile_args_check", []))


def test_reconcile_args_check_sanitized(tmp_path_factory):
    _run(_build(tmp_path_factory, "reconcile_args_check_san",
                ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]))
