"""Key verification inside rate-adaptive and blind reconciliation
(qkd_adapt_verify_tags_batch, qkd_reconcile_adaptive_verify_batch,
qkd_reconcile_blind_verify_batch) at the ABI and wrapper level: the symbols, their
argument validation before any device work, the Python wrappers' tensor checks, the
model's tag against the bit-by-bit definition, the model's round loop against
blind_model's, and the host-only argument checks as a stand-alone program, plain and
under AddressSanitizer + UBSan."""
import os
import subprocess
import types

import numpy as np
import pytest

from tests import adapt_model as AM
from tests import adapt_verify_model as VM
from tests import blind_model as BM

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "adapt_verify_args_check.cpp")
NEW = ("qkd_adapt_verify_tags_batch", "qkd_reconcile_adaptive_verify_batch", "qkd_reconcile_blind_verify_batch")


@pytest.fixture(scope="module")
def N():
    from qkd_ldpc_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        from qkd_ldpc_amd.build import build
        build()
    return _native


def test_library_exports_adapt_verify(N):
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert name in N.EXPORTS and hasattr(N.lib(), name) and name in defined, name
    assert len(N.lib().qkd_adapt_verify_tags_batch.argtypes) == 8
    assert len(N.lib().qkd_reconcile_adaptive_verify_batch.argtypes) == 17 + 6
    assert len(N.lib().qkd_reconcile_blind_verify_batch.argtypes) == 23 + 6
    assert len(N.lib().qkd_reconcile_adaptive_batch.argtypes) == 17      # unchanged
    assert len(N.lib().qkd_reconcile_blind_batch.argtypes) == 23
    assert len(N.lib().qkd_verify_tags_batch.argtypes) == 8
    assert N.lib().qkd_abi_version() == 1          # additive change


def test_tags_arguments_before_any_device_work(N):
    L = N.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data

    def call(plan=p, payload=p, n_frames=1, words=None, tag_bits=64, tags=p):
        return L.qkd_adapt_verify_tags_batch(plan, payload, n_frames, 5, words, tag_bits, tags, None)

    for name in ("plan", "payload", "tags"):
        assert call(**{name: None}) == N.ERR_INVALID_ARG, name
        assert "null" in N.last_error(), name
        assert call(**{name: None}, n_frames=0, tag_bits=0, words=p) == N.ERR_INVALID_ARG, name
        assert "null" in N.last_error(), name
    assert call(n_frames=0) == N.ERR_INVALID_ARG and "n_frames" in N.last_error()
    assert call(n_frames=2**32) == N.ERR_INVALID_ARG and "n_frames" in N.last_error()
    for t in (0, 65, 2**32 - 1):
        assert call(tag_bits=t) == N.ERR_INVALID_ARG and "tag_bits" in N.last_error(), t


def verify_cases(call, N, p):
    """The six verification arguments' rules, whatever entry `call` is."""
    for t in (0, 65, 2**32 - 1):
        assert call(tag_bits=t) == N.ERR_INVALID_ARG and "tag_bits" in N.last_error(), t
    assert call(alice=None, tags=None, verified=None) == N.ERR_INVALID_ARG
    assert "neither" in N.last_error()
    assert call(alice=None, tags=None) == N.ERR_INVALID_ARG and "neither" in N.last_error()
    assert call(verified=None) == N.ERR_INVALID_ARG and "without verified" in N.last_error()
    assert call(tags=None, verified=None) == N.ERR_INVALID_ARG and "without verified" in N.last_error()
    assert call(alice=None) == N.ERR_INVALID_ARG and "without alice_tags" in N.last_error()


def test_adaptive_verify_arguments_before_any_device_work(N):
    """NULL arrays, a NULL plan, the tag width and the tag arguments' rules:
    QKD_ERR_INVALID_ARG before the code or the plan is looked at (both are fake)."""
    L = N.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data

    def call(code=p, plan=p, bob=p, syn=p, payload=p, frames=None, iters=p, ok=p, corrected=None, n_frames=1,
             qber=0.02, words=None, tag_bits=64, alice=p, tags=p, verified=p):
        return L.qkd_reconcile_adaptive_verify_batch(code, None, plan, bob, syn, n_frames, qber, 100.0, 50, 100.0,
                                                     N.FLAG_THRESHOLD, payload, frames, iters, ok, corrected, 7,
                                                     words, tag_bits, alice, tags, verified, None)

    for name in ("code", "plan", "bob", "syn", "payload", "iters", "ok"):
        assert call(**{name: None}) == N.ERR_INVALID_ARG, name
        assert "null" in N.last_error(), name
        assert call(**{name: None}, tag_bits=0, alice=None, tags=None, frames=p, corrected=p, words=p) \
            == N.ERR_INVALID_ARG, name
        assert "null" in N.last_error(), name
    assert call(n_frames=0) == N.ERR_INVALID_ARG
    for q in (0.0, 1.0, float("nan")):
        assert call(qber=q) == N.ERR_INVALID_ARG
    verify_cases(call, N, p)


def test_blind_verify_arguments_before_any_device_work(N):
    L = N.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data

    def call(code=p, plan=p, bob=p, syn=p, revealed=p, nrev=p, skip=None, step=1, max_rounds=1, payload=p,
             frames=None, iters=p, ok=p, corrected=None, rounds=None, n_frames=1, qber=0.02, words=None,
             tag_bits=64, alice=p, tags=p, verified=p):
        return L.qkd_reconcile_blind_verify_batch(code, None, plan, bob, syn, n_frames, qber, 100.0, 50, 100.0,
                                                  N.FLAG_THRESHOLD, revealed, nrev, skip, step, max_rounds,
                                                  payload, frames, iters, ok, corrected, rounds, 7, words,
                                                  tag_bits, alice, tags, verified, None)

    for name in ("code", "plan", "bob", "syn", "nrev", "payload", "iters", "ok"):
        assert call(**{name: None}) == N.ERR_INVALID_ARG, name
        assert "null" in N.last_error(), name
        assert call(**{name: None}, max_rounds=0, step=0, skip=p, frames=p, corrected=p, rounds=p, tag_bits=0,
                    alice=None, tags=None) == N.ERR_INVALID_ARG, name
        assert "null" in N.last_error(), name
    assert call(n_frames=0) == N.ERR_INVALID_ARG
    for q in (0.0, 1.0, float("nan")):
        assert call(qber=q) == N.ERR_INVALID_ARG
    for step in (0, 1, 256):
        assert call(max_rounds=0, step=step, tag_bits=0) == N.ERR_INVALID_ARG
        assert "max_rounds" in N.last_error()
    for rounds in (2, 6, 2**32 - 1):
        assert call(max_rounds=rounds, step=0, tag_bits=0) == N.ERR_INVALID_ARG
        assert "step" in N.last_error()
    verify_cases(call, N, p)
    verify_cases(lambda **kw: call(max_rounds=6, step=256, skip=p, rounds=p, **kw), N, p)


def test_wrappers_reject_host_tensors(N):
    import torch
    import qkd_ldpc_amd as Q
    H = types.SimpleNamespace(num_bit_nodes=8, num_check_nodes=4, device=0, handle=None)
    plan = types.SimpleNamespace(n_bits=8, n_payload=6, n_punctured=2, n_shortened=0, device=0, handle=None)
    bob = torch.zeros(2, 6, dtype=torch.uint8)
    syn = torch.zeros(2, 4, dtype=torch.uint8)
    rev = torch.zeros(2, 2, dtype=torch.uint8)
    tags = torch.zeros(2, dtype=torch.int64)
    words = torch.zeros(VM.key_words(6), dtype=torch.int64)
    calls = [
        lambda: Q.verify_tags(plan, bob),                                      # host tensors
        lambda: Q.verify_tags(plan, bob.numpy()),
        lambda: Q.verify_tags(plan, bob.double()),                             # wrong dtype
        lambda: Q.verify_tags(plan, None),
        lambda: Q.reconcile_adaptive(H, plan, bob, syn, 0.02, alice_tags=tags),
        lambda: Q.reconcile_adaptive(H, plan, bob, syn, 0.02, want_tags=True),
        lambda: Q.reconcile_adaptive(H, plan, bob, syn, 0.02, hash_words=words),
        lambda: Q.reconcile_blind(H, plan, bob, syn, 0.02, rev, alice_tags=tags),
        lambda: Q.reconcile_blind(H, plan, bob, syn, 0.02, rev, hash_seed=1),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(Q.QkdError) as ei:
            call()
        assert ei.value.status == N.ERR_INVALID_ARG, k
    assert "ReconcileResult" in Q.__all__ and "verify_tags" in Q.__all__


@pytest.mark.gpu
def test_wrappers_reject_dtypes_and_shapes(golden_code):
    import torch
    import qkd_ldpc_amd as Q
    g = golden_code
    H = Q.HMatrix.from_check_lists(10240, g["chk_off"], g["chk_idx"])
    plan = Q.AdaptPlan(H, [5, 9, 2], [7])
    npay = plan.n_payload
    bob = torch.zeros(4, npay, dtype=torch.uint8, device="cuda")
    syn = torch.zeros(4, 5231, dtype=torch.uint8, device="cuda")
    rev = torch.zeros(4, 3, dtype=torch.uint8, device="cuda")
    at = torch.zeros(4, dtype=torch.int64, device="cuda")
    w = torch.zeros(Q.verify_key_words(npay), dtype=torch.int64, device="cuda")
    assert Q.verify_key_words(npay) == VM.key_words(npay)
    A = lambda **kw: Q.reconcile_adaptive(H, plan, bob, syn, 0.02, **kw)
    B = lambda **kw: Q.reconcile_blind(H, plan, bob, syn, 0.02, rev, **kw)
    cases = []
    for E in (A, B):
        cases += [
            lambda E=E: E(alice_tags=at.cpu()),                                   # host tensors
            lambda E=E: E(hash_words=w.cpu()),
            lambda E=E: E(alice_tags=at.to(torch.int32)),                         # wrong dtypes
            lambda E=E: E(alice_tags=at.double()),
            lambda E=E: E(hash_words=w.to(torch.uint8)),
            lambda E=E: E(alice_tags=at[:3]),                                     # wrong shapes
            lambda E=E: E(alice_tags=torch.zeros(5, dtype=torch.int64, device="cuda")),
            lambda E=E: E(hash_words=w[:-1]),
            lambda E=E: E(hash_words=torch.zeros(w.numel() + 1, dtype=torch.int64, device="cuda")),
            lambda E=E: E(alice_tags=at, tag_bits=0),                             # the C entry's rules
            lambda E=E: E(alice_tags=at, tag_bits=65),
            lambda E=E: E(want_tags=True, tag_bits=0),
        ]
    cases += [
        lambda: Q.verify_tags(plan, bob[:, :npay - 1]),
        lambda: Q.verify_tags(plan, torch.zeros(4, 10240, dtype=torch.uint8, device="cuda")),
        lambda: Q.verify_tags(plan, bob.to(torch.int32)),
        lambda: Q.verify_tags(plan, bob, hash_words=w[:-1]),
        lambda: Q.verify_tags(plan, bob, tag_bits=0),
        lambda: Q.verify_tags(plan, bob, tag_bits=65),
    ]
    for k, call in enumerate(cases):
        with pytest.raises(Q.QkdError) as ei:
            call()
        assert ei.value.status == Q._native.ERR_INVALID_ARG, k
    # the calls these are variations of are valid: the zero payload has tag 0 and verifies
    for E in (A, B):
        r = E(alice_tags=at, hash_words=w)
        torch.cuda.synchronize()
        assert r.syndromes_match.cpu().numpy().all() and r.verified.cpu().numpy().all()
        assert not r.tags.cpu().numpy().any() and not r.bits.cpu().numpy().any()
        r = E(want_tags=True)
        assert r.verified is None and r.tags is not None
        r = E()
        assert r.verified is None and r.tags is None
    torch.cuda.synchronize()
    assert not Q.verify_tags(plan, bob).cpu().numpy().any()
    # the C entries: another code's plan, the binary64 variant only
    N = Q._native
    out = torch.zeros(4 * npay, dtype=torch.uint8, device="cuda")
    it = torch.zeros(4, dtype=torch.int32, device="cuda")
    ok = torch.zeros(4, dtype=torch.uint8, device="cuda")
    tg = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = N.lib().qkd_reconcile_adaptive_verify_batch(
        H.handle, None, plan.handle, bob.data_ptr(), syn.data_ptr(), 4, 0.02, 100.0, 50, 100.0,
        N.FLAG_THRESHOLD | N.VARIANTS["sp_f32"], out.data_ptr(), None, it.data_ptr(), ok.data_ptr(), None, 0, None,
        64, None, tg.data_ptr(), None, None)
    assert st == N.ERR_UNSUPPORTED
    plan.close()
    H.close()


def test_payload_tag_definition():
    """payload_tag against the bit-by-bit definition, n_payload = 10, seed 12345: tag bit i
    = XOR over the set positions k of bit k + i of the key string."""
    n, seed = 10, 12345
    R = VM.expand_key(seed, n)
    assert len(R) == VM.key_words(n) == 2 and VM.key_words(1) == 1 and VM.key_words(2) == 2
    assert VM.key_words(65) == 2 and VM.key_words(66) == 3 and VM.key_words(9203) == 145
    r = [(R[k >> 6] >> (k & 63)) & 1 for k in range(128)]
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 2, (8, n)).astype(np.uint8)
    x[0] = 0
    x[1] = 1
    for row in x:
        want = 0
        for i in range(64):
            bit = 0
            for k in range(n):
                bit ^= r[k + i] & int(row[k])
            want |= bit << i
        for t in (1, 13, 64):
            assert VM.payload_tag(R, row, t) == want & ((1 << t) - 1)
        assert VM.payload_tag(R, row | 0xFE, 64) == want          # only byte & 1 counts
    assert VM.payload_tag(R, x[0]) == 0
    # a window at a word boundary needs no word past the string's end
    R65 = VM.expand_key(seed, 65)
    one = np.zeros(65, np.uint8)
    one[64] = 1
    assert VM.payload_tag(R65, one) == R65[1]


def test_model_loop_is_blind_models_when_tags_are_honest(dense_codes, oracle_mod):
    """With Alice's honest tag (or none) the loop closes where blind_model.blind_loop
    closes: the same record, plus tags and verified."""
    dense = next(d for d in dense_codes.values() if d.shape[1] == 10)
    g = AM.Graph.from_dense(dense)
    pu, sh = [3, 8], [0]
    pay = np.setdiff1d(np.arange(10), pu + sh)
    R = VM.expand_key(12345, pay.size)
    rng = np.random.default_rng(10)
    seen = set()
    for _ in range(24):
        frame = rng.integers(0, 2, 10).astype(np.uint8)
        frame[sh] = 0
        bob = frame[pay] ^ (rng.random(pay.size) < 0.15).astype(np.uint8)
        syn = g.syndrome(frame)
        want = BM.blind_loop(g, pu, sh, bob, syn, 0.1, oracle_mod.libm, frame[pu], 0, 1, 3)
        honest = want["last"]["sp_ok"] == bool((want["payload"] == frame[pay]).all())
        at = VM.payload_tag(R, frame[pay])
        for alice_tag in (at, None):
            got = VM.blind_loop(g, pu, sh, bob, syn, 0.1, oracle_mod.libm, frame[pu], R, 64, alice_tag, 0, 1, 3)
            if alice_tag is not None and not honest:
                continue                              # (a wrong word with Alice's syndrome: not this test's)
            for key in ("rounds", "n_revealed", "leak_bits", "corrected"):
                assert got[key] == want[key], key
            assert (got["payload"] == want["payload"]).all() and len(got["all"]) == len(want["all"])
            assert all((a["out"] == b["out"]).all() and a["iters"] == b["iters"] and a["sp_ok"] == b["sp_ok"]
                       for a, b in zip(got["all"], want["all"]))
            assert got["tags"] == [VM.payload_tag(R, r["out"][pay]) for r in got["all"]]
            if alice_tag is None:
                assert got["verified"] == [None] * got["rounds"]
            else:
                assert got["verified"] == [bool(r["sp_ok"]) for r in got["all"]]
        seen.add((want["rounds"], bool(want["last"]["sp_ok"]), honest))
    assert {r for r, _, _ in seen} >= {1, 2} and any(h for _, _, h in seen)


# ---- the host-only argument checks, stand-alone ----------------------------------------

def _build(tmp_path_factory, name, extra):
    out = str(tmp_path_factory.mktemp("native") / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-o", out, SRC])
    return out


def _run(binary):
    r = subprocess.run([binary], text=True, capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0", r.stdout + r.stderr


def test_adapt_verify_args_check(tmp_path_factory):
    _run(_build(tmp_path_factory, "adapt_verify_args_check", []))


def test_adapt_verify_args_check_sanitized(tmp_path_factory):
    _run(_build(tmp_path_factory, "adapt_verify_args_check_san",
                ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]))
