"""Rate adaptation at the ABI level, without a GPU: the new symbols, the host
helper qkd_adapt_positions against its Python restatement (tests/adapt_model.py),
and that model's decoder pinned to the oracle on frames without zero LLRs."""
import subprocess

import numpy as np
import pytest

from tests import adapt_model as AM

NEW = ["qkd_adapt_create", "qkd_adapt_destroy", "qkd_adapt_get_info", "qkd_adapt_positions",
       "qkd_adapt_embed_batch", "qkd_adapt_extract_batch", "qkd_reconcile_adaptive_batch"]


@pytest.fixture(scope="module")
def N():
    import os
    from qkd_ldpc_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        from qkd_ldpc_amd.build import build
        build()
    return _native


def test_library_exports_adapt(N):
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    defined = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert name in N.EXPORTS
        assert hasattr(N.lib(), name)
        assert name in defined
    assert len(N.lib().qkd_reconcile_adaptive_batch.argtypes) == 17
    assert N.FLAG_ERASURES == 0x2
    assert N.lib().qkd_abi_version() == 1          # additive change


def _graphs(golden_code, dense_codes):
    out = [("golden", AM.Graph(int(golden_code["dims"][0]), golden_code["chk_off"], golden_code["chk_idx"]))]
    out += [(name, AM.Graph.from_dense(d)) for name, d in sorted(dense_codes.items())]
    assert sorted(g.n for _, g in out) == [6, 7, 10, 10240]
    return out


def _positions(g, count, seed):
    import qkd_ldpc_amd as Q
    return Q.adapt_positions((g.n, g.cptr.astype(np.int32), g.cidx.astype(np.int32)), count, seed)


def test_positions(N, golden_code, dense_codes):
    for name, g in _graphs(golden_code, dense_codes):
        counts = sorted({0, 1, g.n // 5, g.n // 2, g.n})
        for count in counts:
            pos, unt = _positions(g, count, 7)
            want, want_unt = AM.positions(g, count, 7)
            assert (pos == want).all() and unt == want_unt, (name, count)
            assert len(pos) == count == len(set(pos.tolist()))
            assert ((pos >= 0) & (pos < g.n)).all()
            # the untainted picks pairwise share no check
            seen = set()
            for b in pos[:unt]:
                chk = set(g.chk_of[g.by_bit[g.bptr[b]:g.bptr[b + 1]]].tolist())
                assert not (chk & seen), (name, count, int(b))
                seen |= chk
            assert 0 <= unt <= count
            if count:
                assert unt >= 1
        full, _ = _positions(g, g.n, 7)
        assert sorted(full.tolist()) == list(range(g.n))           # count = N: a permutation
        again, _ = _positions(g, g.n, 7)
        other, _ = _positions(g, g.n, 8)
        assert (again == full).all()
        assert not (other == full).all()
        # a shorter list is a prefix of pass 1 while pass 1 lasts
        part, unt = _positions(g, max(1, g.n // 5), 7)
        full_unt = _positions(g, g.n, 7)[1]
        k = min(unt, full_unt)
        assert (part[:k] == full[:k]).all()


def test_positions_argument_errors(N, golden_code):
    import qkd_ldpc_amd as Q
    n = int(golden_code["dims"][0])
    csr = (n, golden_code["chk_off"], golden_code["chk_idx"])
    for count in (-1, n + 1):
        with pytest.raises(Q.QkdError) as e:
            Q.adapt_positions(csr, count, 1)
        assert e.value.status == N.ERR_INVALID_ARG


def test_null_arguments(N):
    """NULL plan / code / arrays: QKD_ERR_INVALID_ARG before anything touches a device."""
    import ctypes as C
    L = N.lib()
    st = C.c_int(0)
    assert not L.qkd_adapt_create(None, None, 0, None, 0, C.byref(st))
    assert st.value == N.ERR_INVALID_ARG
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    assert L.qkd_adapt_embed_batch(None, p, 1, None, p, None) == N.ERR_INVALID_ARG
    assert L.qkd_adapt_extract_batch(None, p, 1, p, None) == N.ERR_INVALID_ARG
    assert L.qkd_adapt_get_info(None, None) == N.ERR_INVALID_ARG
    # (a NULL array fails before the code or the plan is looked at)
    assert L.qkd_reconcile_adaptive_batch(p, None, p, None, p, 1, 0.02, 100.0, 50, 100.0, 1,
                                          p, None, p, p, None, None) == N.ERR_INVALID_ARG
    assert L.qkd_reconcile_adaptive_batch(None, None, None, p, p, 1, 0.02, 100.0, 50, 100.0, 1,
                                          p, None, p, p, None, None) == N.ERR_INVALID_ARG
    L.qkd_adapt_destroy(None)


def test_decoder_flags_erasures(N):
    import qkd_ldpc_amd as Q
    assert Q.decoder_flags(True, erasures=True) == (N.FLAG_THRESHOLD | N.FLAG_ERASURES)
    assert Q.decoder_flags(False, erasures=True) == N.FLAG_ERASURES
    assert Q.decoder_flags(True) == N.FLAG_THRESHOLD


def test_model_equals_oracle_without_zeros(golden_code, oracle_mod, oracle_code):
    """Pins the model, not the library: 3 golden frames per QBER, no zero LLR."""
    g = AM.Graph(int(golden_code["dims"][0]), golden_code["chk_off"], golden_code["chk_idx"])
    for q, thr, thr_on in ((0.02, 100.0, True), (0.08, 100.0, True), (0.02, 0.7, True), (0.02, 100.0, False)):
        rng = np.random.default_rng(11)
        alice = rng.integers(0, 2, (3, g.n)).astype(np.uint8)
        bob = alice ^ (rng.random((3, g.n)) < q).astype(np.uint8)
        lp = AM.log_p(q)
        for k in range(3):
            syn = g.syndrome(alice[k])
            assert (syn == oracle_code.syndrome(alice[k])).all()
            llr = np.where(bob[k] == 1, -lp, lp)
            for era in (True, False):
                got = AM.decode(g, llr, syn, oracle_mod.libm, 50, thr, thr_on, erasures=era)
                want = oracle_code.decode(llr, syn, 50, thr, thr_on)
                assert got["iters"] == want["iters"] and got["sp_ok"] == want["sp_ok"]
                assert (got["out"] == want["out"]).all()
                assert sum(got["z1"]) == 0 and sum(got["z2"]) == 0
