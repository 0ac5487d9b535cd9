"""A numpy restatement of the reference decoder (qkd_ldpc_algorithm.cpp:175-345)
with the erasure rule of QKD_FLAG_ERASURES, and a Python restatement of
qkd_adapt_positions. A helper of tests/test_adapt*.py, not a test.

Every floating-point operation is the reference's, in its order: tanh and atanh
are glibc's (passed in as `libm`, the oracle's), a check's product runs over its
edges in ascending order starting from sigma, a bit's total is accumulated as
std::accumulate does (LLR first, then the bit's checks ascending), the clamp is
compare-based (NaN passes through).

The erasure rule, on the published t_k = tanh(b2c_k / 2) of one check, with z
the number of t_k equal to zero (either sign) and sigma = -1 if the check's
syndrome bit is set, else +1:
  z = 0   c2b_k = 2 atanh(P / t_k), P = sigma t_0 t_1 ...   (the reference)
  z = 1   the edge whose t is zero gets 2 atanh(P'), P' = sigma times the
          non-zero t in ascending order; every other edge gets +0.0
  z >= 2  every edge gets +0.0
"""
import math

import numpy as np

MASK64 = (1 << 64) - 1


class Graph:
    """Edge arrays of a check-side CSR (rows ascending), edges in check-major order."""

    def __init__(self, n, cptr, cidx):
        self.n = int(n)
        self.cptr = np.asarray(cptr, np.int64)
        self.cidx = np.asarray(cidx, np.int64)
        self.m = self.cptr.size - 1
        self.cdeg = np.diff(self.cptr)
        assert (self.cdeg >= 1).all()
        self.chk_of = np.repeat(np.arange(self.m), self.cdeg)
        # bit-major order: each bit's edges by ascending check (a stable sort keeps it)
        self.by_bit = np.argsort(self.cidx, kind="stable")
        self.bdeg = np.bincount(self.cidx, minlength=self.n)
        self.bptr = np.concatenate([[0], np.cumsum(self.bdeg)])

    @classmethod
    def from_dense(cls, dense):
        d = np.asarray(dense)
        ptr, idx = [0], []
        for row in d:
            idx.extend(np.nonzero(row)[0].tolist())
            ptr.append(len(idx))
        return cls(d.shape[1], ptr, idx)

    def syndrome(self, bits):
        return (np.add.reduceat(np.asarray(bits, np.int64)[self.cidx], self.cptr[:-1]) & 1).astype(np.uint8)


def clamp_msg(v, thr):
    return np.where(v > thr, thr, np.where(v < -thr, -thr, v))


def log_p(q):
    return math.log((1.0 - q) / q)


def decode(g, llr, syndrome, libm, max_it=50, thr=100.0, thr_on=True, erasures=True):
    """One frame. Returns a dict: iters, sp_ok, out (the last hard decision), nan (a NaN
    message or total was met), z1 / z2 (per executed iteration: checks with z = 1, z >= 2)."""
    llr = np.asarray(llr, np.float64)
    syn = (np.asarray(syndrome) != 0).astype(np.uint8)
    sigma = np.where(syn != 0, -1.0, 1.0)
    b2c = llr[g.cidx].copy()
    z1, z2 = [], []
    nan = False
    out = np.zeros(g.n, np.uint8)
    with np.errstate(all="ignore"):
        for it in range(max_it):
            t = libm("tanh", b2c / 2.0)
            P = sigma.copy()
            z = np.zeros(g.m, np.int64)
            for k in range(int(g.cdeg.max())):
                rows = np.nonzero(g.cdeg > k)[0]
                tk = t[g.cptr[rows] + k]
                zero = (tk == 0.0) if erasures else np.zeros(tk.size, bool)
                z[rows] += zero
                P[rows] = np.where(zero, P[rows], P[rows] * tk)
            ze = z[g.chk_of]
            Pe = P[g.chk_of]
            arg = np.where(ze == 0, Pe / t, Pe)
            c2b = 2.0 * libm("atanh", arg)
            c2b[(ze >= 2) | ((ze == 1) & (t != 0.0))] = 0.0
            z1.append(int((z == 1).sum()))
            z2.append(int((z >= 2).sum()))
            if thr_on:
                c2b = clamp_msg(c2b, thr)
            total = llr.copy()
            for k in range(int(g.bdeg.max())):
                bits = np.nonzero(g.bdeg > k)[0]
                total[bits] = total[bits] + c2b[g.by_bit[g.bptr[bits] + k]]
            nan = nan or bool(np.isnan(c2b).any() or np.isnan(total).any())
            out = (total <= 0).astype(np.uint8)
            if (g.syndrome(out) == syn).all():
                return {"iters": it + 1, "sp_ok": True, "out": out, "nan": nan, "z1": z1, "z2": z2}
            b2c = total[g.cidx] - c2b
            if thr_on:
                b2c = clamp_msg(b2c, thr)
    return {"iters": max_it, "sp_ok": False, "out": out, "nan": nan, "z1": z1, "z2": z2}


def mix(z):
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def positions(g, count, seed):
    """qkd_adapt_positions: (positions in the order taken, how many pass 1 took)."""
    n = g.n
    order = list(range(n))
    k = 0
    for i in range(n - 1, 0, -1):
        j = mix(seed + (k + 1) * 0x9E3779B97F4A7C15) % (i + 1)
        order[i], order[j] = order[j], order[i]
        k += 1
    checks = [g.chk_of[g.by_bit[g.bptr[b]:g.bptr[b + 1]]].tolist() for b in range(n)]
    tainted = set()
    taken, got = set(), []
    for b in order:
        if len(got) >= count:
            break
        if any(j in tainted for j in checks[b]):
            continue
        tainted.update(checks[b])
        taken.add(b)
        got.append(b)
    untainted = len(got)
    for b in order:
        if len(got) >= count:
            break
        if b not in taken:
            taken.add(b)
            got.append(b)
    return np.array(got, np.int32), untainted


def frame_llrs(n, punctured, shortened, bob_payload, q, known):
    """The LLRs of qkd_reconcile_adaptive_batch's contract for one frame."""
    lp = log_p(q)
    pay = np.setdiff1d(np.arange(n), np.concatenate([np.asarray(punctured, np.int64),
                                                     np.asarray(shortened, np.int64)]))
    llr = np.zeros(n, np.float64)
    llr[pay] = np.where(np.asarray(bob_payload) & 1, -lp, lp)
    llr[np.asarray(shortened, np.int64)] = known
    return llr, pay
