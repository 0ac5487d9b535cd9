"""The psi slots the folded first bit phase writes (qkd_spec.h psi_of_exact,
psi_of_exact2; debug-math forms 11 and 10): sign-magnitude, the low word
lo | sign << 31 (lo >= +0), the high word hi, NaN in both where the sign of
the exact b2c is not certain. Checked against a binary64 psi and a binary32
restatement of the certification rule (iv_of, then |.|lo > 1e-30).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32


def grid():
    rng = np.random.default_rng(8)
    e = 2.0 ** -20
    mags = [0.0, 5e-324, 1e-310, 1e-40, 1e-38, 1e-31, 1e-30 * (1 - e), 1e-30 * (1 + e), 1.0, 80.0, 100.0, np.inf]
    special = np.array([s * v for v in mags for s in (1.0, -1.0)] + [np.nan, np.nan])
    rnd = np.exp(rng.uniform(np.log(1e-30), np.log(100.0), 4096)) * rng.choice([-1.0, 1.0], 4096)
    x = np.concatenate([special, special[::-1], rnd])
    assert x.size % 2 == 0
    return x


def certified(b):
    """psi_of_exact's rule in binary32: the enclosing interval of b (iv_of: the
    rounding widened by 2^-22 relative and 1e-38) excludes 0 and its magnitude's
    lower bound exceeds 1e-30. (The fused multiply-adds are exact in binary64
    before their one rounding: 24-bit operands, 22 bits apart.)"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = b.astype(F32)
        a = np.abs(f)
        lo = (f.astype(np.float64) - a.astype(np.float64) * 2.0 ** -22).astype(F32) - F32(1e-38)
        hi = (f.astype(np.float64) + a.astype(np.float64) * 2.0 ** -22).astype(F32) + F32(1e-38)
        neg = hi < 0
        ax = np.where(neg, -hi, lo)
        return (neg | (lo > 0)) & (ax > F32(1e-30))


def psi64(x):
    """-log2(tanh(x / 2)) in binary64, x > 0 (past 1 through log1p: tanh rounds to 1)."""
    with np.errstate(over="ignore", divide="ignore"):
        small = -np.log2(np.tanh(np.minimum(x, 1.0) / 2))
        large = -np.log1p(-2.0 / (np.exp(np.maximum(x, 1.0)) + 1.0)) / np.log(2.0)
    return np.where(x < 1.0, small, large)


@pytest.fixture(scope="module")
def slots():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import qkd_ldpc_amd as Q
    x = grid()
    dx = torch.from_numpy(x).cuda()
    out = {}
    for which in (10, 11):
        dy = torch.empty_like(dx)
        Q._native.check(Q._native.lib().qkd_debug_math(which, dx.data_ptr(), dy.data_ptr(), dx.numel(), None))
        torch.cuda.synchronize()
        out[which] = dy.cpu().numpy().view(np.uint64)
    w = out[10]
    return {"x": x, "raw": out, "lo_word": (w & 0xFFFFFFFF).astype(np.uint32), "hi_word": (w >> 32).astype(np.uint32),
            "ok": certified(x)}


def test_forms_bit_equal(slots):
    bad = np.nonzero(slots["raw"][10] != slots["raw"][11])[0]
    assert bad.size == 0, (bad[:8], slots["x"][bad[:8]])


def test_nan_exactly_where_uncertain(slots):
    lo, hi = slots["lo_word"].view(F32), slots["hi_word"].view(F32)
    ok = slots["ok"]
    print(f"{ok.sum()} of {ok.size} inputs certified")
    assert ok.sum() > 4000 and (~ok).sum() >= 30
    bad = np.nonzero((np.isnan(lo) | np.isnan(hi)) != ~ok)[0]
    assert bad.size == 0, (bad[:8], slots["x"][bad[:8]])
    assert (np.isnan(lo) == np.isnan(hi)).all()


def test_sign_bit_is_the_sign_of_b2c(slots):
    ok, x = slots["ok"], slots["x"]
    sign = (slots["lo_word"] >> 31).astype(bool)
    bad = np.nonzero(ok & (sign != (x < 0)))[0]
    assert bad.size == 0, (bad[:8], x[bad[:8]])
    # the high word carries none: hi > 0
    assert ((slots["hi_word"][ok] >> 31) == 0).all()


def test_magnitude_bounds_enclose_psi(slots):
    ok, x = slots["ok"], slots["x"]
    lo = (slots["lo_word"] & np.uint32(0x7FFFFFFF)).view(F32).astype(np.float64)[ok]
    hi = slots["hi_word"].view(F32).astype(np.float64)[ok]
    p = psi64(np.abs(x[ok]))
    rel = np.max((hi - lo)[p > 1e-3] / p[p > 1e-3])
    print(f"largest relative width above psi = 1e-3: {rel:.3e}")
    bad = np.nonzero(~((lo <= p) & (p <= hi)))[0]
    assert bad.size == 0, (bad[:8], x[ok][bad[:8]], lo[bad[:8]], p[bad[:8]], hi[bad[:8]])
    assert (lo >= 0).all()
