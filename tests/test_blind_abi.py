"""qkd_reconcile_blind_batch (blind reconciliation: per-frame reveal rounds) at the ABI
and wrapper level: the symbol, its argument validation before any device work, the
Python wrapper's tensor checks, the model's LLRs, and the host-only argument check as a
stand-alone program, plain and under AddressSanitizer + UBSan."""
import os
import subprocess
import types

import numpy as np
import pytest

from tests import adapt_model as AM
from tests import blind_model as BM

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "blind_args_check.cpp")


@pytest.fixture(scope="module")
def N():
    from qkd_ldpc_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        from qkd_ldpc_amd.build import build
        build()
    return _native


def test_library_exports_blind(N):
    import qkd_ldpc_amd as Q
    assert "qkd_reconcile_blind_batch" in N.EXPORTS
    assert hasattr(N.lib(), "qkd_reconcile_blind_batch")
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    assert any(line.split()[-1] == "qkd_reconcile_blind_batch" and " T " in line for line in out.splitlines())
    assert len(N.lib().qkd_reconcile_blind_batch.argtypes) == 23
    assert len(N.lib().qkd_reconcile_adaptive_batch.argtypes) == 17      # unchanged
    assert N.lib().qkd_abi_version() == 1          # additive change
    assert "reconcile_blind" in Q.__all__ and "BlindResult" in Q.__all__


def test_blind_arguments_before_any_device_work(N):
    """NULL arrays, a NULL plan, NULL n_revealed, no round, no step from two rounds on:
    QKD_ERR_INVALID_ARG before the code or the plan is looked at (both are fake)."""
    L = N.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data

    def call(code=p, plan=p, bob=p, syn=p, revealed=p, nrev=p, skip=None, step=1, max_rounds=1,
             payload=p, frames=None, iters=p, ok=p, corrected=None, rounds=None, n_frames=1, qber=0.02):
        return L.qkd_reconcile_blind_batch(code, None, plan, bob, syn, n_frames, qber, 100.0, 50, 100.0,
                                           N.FLAG_THRESHOLD, revealed, nrev, skip, step, max_rounds,
                                           payload, frames, iters, ok, corrected, rounds, None)

    for name in ("code", "plan", "bob", "syn", "nrev", "payload", "iters", "ok"):
        assert call(**{name: None}) == N.ERR_INVALID_ARG, name
        assert "null" in N.last_error(), name
        # ... whatever else is wrong, and with every optional array given or not
        assert call(**{name: None}, max_rounds=0, step=0, skip=p, frames=p, corrected=p, rounds=p) \
            == N.ERR_INVALID_ARG, name
        assert "null" in N.last_error(), name
    assert call(n_frames=0) == N.ERR_INVALID_ARG
    for q in (0.0, 1.0, float("nan")):
        assert call(qber=q) == N.ERR_INVALID_ARG
    for step in (0, 1, 256):
        assert call(max_rounds=0, step=step) == N.ERR_INVALID_ARG
        assert "max_rounds" in N.last_error()
    for rounds in (2, 6, 2**32 - 1):
        assert call(max_rounds=rounds, step=0) == N.ERR_INVALID_ARG
        assert "step" in N.last_error()
    assert call(code=None, plan=None, bob=None, syn=None, revealed=None, nrev=None, payload=None, iters=None,
                ok=None) == N.ERR_INVALID_ARG


def test_blind_wrapper_rejects_host_tensors(N):
    import torch
    import qkd_ldpc_amd as Q
    H = types.SimpleNamespace(num_bit_nodes=8, num_check_nodes=4, device=0, handle=None)
    plan = types.SimpleNamespace(n_bits=8, n_payload=6, n_punctured=2, n_shortened=0, device=0, handle=None)
    bob = torch.zeros(2, 6, dtype=torch.uint8)
    syn = torch.zeros(2, 4, dtype=torch.uint8)
    rev = torch.zeros(2, 2, dtype=torch.uint8)
    for b, s in [(bob, syn), (bob.numpy(), syn.numpy()), (bob.double(), syn), (None, syn)]:
        with pytest.raises(Q.QkdError) as ei:
            Q.reconcile_blind(H, plan, b, s, 0.02, rev)
        assert ei.value.status == N.ERR_INVALID_ARG


@pytest.mark.gpu
def test_blind_wrapper_rejects_dtypes_and_shapes(golden_code):
    import torch
    import qkd_ldpc_amd as Q
    g = golden_code
    H = Q.HMatrix.from_check_lists(10240, g["chk_off"], g["chk_idx"])
    plan = Q.AdaptPlan(H, [5, 9, 2], [7])
    plain = Q.AdaptPlan(H, [], [7])
    npay = plan.n_payload
    bob = torch.zeros(4, npay, dtype=torch.uint8, device="cuda")
    syn = torch.zeros(4, 5231, dtype=torch.uint8, device="cuda")
    rev = torch.zeros(4, 3, dtype=torch.uint8, device="cuda")
    nrev = torch.zeros(4, dtype=torch.int32, device="cuda")
    skip = torch.zeros(4, dtype=torch.uint8, device="cuda")
    B = Q.reconcile_blind
    cases = [
        lambda: B(H, plan, bob.cpu(), syn, 0.02, rev),                        # host tensors
        lambda: B(H, plan, bob, syn.cpu(), 0.02, rev),
        lambda: B(H, plan, bob, syn, 0.02, rev.cpu()),
        lambda: B(H, plan, bob, syn, 0.02, rev, nrev.cpu()),
        lambda: B(H, plan, bob, syn, 0.02, rev, nrev, skip.cpu()),
        lambda: B(H, plan, bob.to(torch.int32), syn, 0.02, rev),              # wrong dtypes
        lambda: B(H, plan, bob, syn, 0.02, rev.to(torch.int32)),
        lambda: B(H, plan, bob, syn, 0.02, rev, nrev.to(torch.int64)),
        lambda: B(H, plan, bob, syn, 0.02, rev, nrev.to(torch.uint8)),
        lambda: B(H, plan, bob, syn, 0.02, rev, nrev, skip.to(torch.bool)),
        lambda: B(H, plan, bob, syn[:3], 0.02, rev),                          # wrong shapes
        lambda: B(H, plan, bob[:, :npay - 1], syn, 0.02, rev),
        lambda: B(H, plan, bob, syn, 0.02, rev[:3]),
        lambda: B(H, plan, bob, syn, 0.02, rev[:, :2]),
        lambda: B(H, plan, bob, syn, 0.02, torch.zeros(4, 4, dtype=torch.uint8, device="cuda")),
        lambda: B(H, plan, bob, syn, 0.02, rev, nrev[:3]),
        lambda: B(H, plan, bob, syn, 0.02, rev, nrev, skip[:3]),
        lambda: B(H, plan, bob, syn, 0.02),                                   # revealed missing with p > 0
        lambda: B(H, plain, torch.zeros(4, plain.n_payload, dtype=torch.uint8, device="cuda"), syn, 0.02,
                  rev),                                                       # revealed without p
        lambda: B(H, plan, bob, syn, 0.02, rev, max_rounds=0),
        lambda: B(H, plan, bob, syn, 0.02, rev, max_rounds=2),                # no step
        lambda: B(H, plan, bob, syn, 0.02, rev, step=-1),
        lambda: B(H, plan, bob, syn, 0.0, rev),                               # as reconcile_adaptive validates
        lambda: B(H, plan, bob, syn, 0.02, rev, known_llr=0.0),
        lambda: B(H, plan, bob, syn, 0.02, rev, max_iterations=0),
    ]
    for k, call in enumerate(cases):
        with pytest.raises(Q.QkdError) as ei:
            call()
        assert ei.value.status == Q._native.ERR_INVALID_ARG, k
    # the C entry itself: revealed exactly when p > 0, and the binary64 variant only
    N = Q._native
    out = torch.zeros(4 * npay, dtype=torch.uint8, device="cuda")
    it = torch.zeros(4, dtype=torch.int32, device="cuda")
    ok = torch.zeros(4, dtype=torch.uint8, device="cuda")

    def raw(pl, revealed, flags=N.FLAG_THRESHOLD):
        return N.lib().qkd_reconcile_blind_batch(
            H.handle, None, pl.handle, bob.data_ptr(), syn.data_ptr(), 4, 0.02, 100.0, 50, 100.0, flags,
            revealed, nrev.data_ptr(), None, 1, 1, out.data_ptr(), None, it.data_ptr(), ok.data_ptr(), None, None,
            None)

    assert raw(plan, None) == N.ERR_INVALID_ARG and "revealed" in N.last_error()
    assert raw(plain, rev.data_ptr()) == N.ERR_INVALID_ARG and "revealed" in N.last_error()
    assert raw(plan, rev.data_ptr(), N.FLAG_THRESHOLD | N.VARIANTS["sp_f32"]) == N.ERR_UNSUPPORTED
    # the call that all of these are variations of is valid, and leaves the caller's counts alone
    nrev[1] = 2
    r = B(H, plan, bob, syn, 0.02, rev, nrev, skip, step=1, max_rounds=2)
    torch.cuda.synchronize()
    assert r.syndromes_match.cpu().numpy().all() and not r.bits.cpu().numpy().any()
    assert nrev.cpu().tolist() == [0, 2, 0, 0] and r.n_revealed.cpu().tolist() == [0, 2, 0, 0]
    assert r.n_revealed.data_ptr() != nrev.data_ptr()
    assert r.rounds.cpu().tolist() == [1, 1, 1, 1]
    assert r.leak_bits.dtype == torch.int32 and r.leak_bits.cpu().tolist() == [5231 - 3 + k for k in (0, 2, 0, 0)]
    for x in (plan, plain):
        x.close()
    H.close()


def test_model_llrs():
    """blind_model.frame_llrs: the revealed prefix is known, the rest stays erased, and
    nothing past the count is looked at."""
    pu, sh = [7, 2, 5], [0]
    bob = np.array([1, 0, 0, 1], np.uint8)
    base, pay = AM.frame_llrs(8, pu, sh, bob, 0.1, 50.0)
    got, pay2 = BM.frame_llrs(8, pu, sh, bob, 0.1, 50.0, [1, 0xA4, 0xA5], 2)
    assert (pay == pay2).all() and pay.tolist() == [1, 3, 4, 6]
    want = base.copy()
    want[7], want[2] = -50.0, 50.0
    assert (got == want).all() and got[5] == 0.0 and not np.signbit(got[5])
    assert (BM.frame_llrs(8, pu, sh, bob, 0.1, 50.0, None, 0)[0] == base).all()
    over = BM.frame_llrs(8, pu, sh, bob, 0.1, 50.0, [1, 0, 1], 9)[0]           # past p counts as p
    assert over[7] == -50.0 and over[2] == 50.0 and over[5] == -50.0


# ---- the host-only argument check, stand-alone ---------------------------------------

def _build(tmp_path_factory, name, extra):
    out = str(tmp_path_factory.mktemp("native") / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-o", out, SRC])
    return out


def _run(binary):
    r = subprocess.run([binary], text=True, capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0", r.stdout + r.stderr


def test_blind_args_check(tmp_path_factory):
    _run(_build(tmp_path_factory, "blind_args_check", []))


def test_blind_args_check_sanitized(tmp_path_factory):
    _run(_build(tmp_path_factory, "blind_args_check_san",
                ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]))
