"""The contract of qkd_reconcile_blind_batch restated on tests/adapt_model.py: the
LLRs of a frame with revealed punctured bits, and the round loop. A helper of
tests/test_blind*.py, not a test."""
import numpy as np

from tests import adapt_model as AM


def frame_llrs(n, punctured, shortened, bob_payload, q, known, revealed=None, n_revealed=0):
    """adapt_model.frame_llrs with the first min(n_revealed, p) punctured positions (in
    the order of the punctured list) known: -+known from revealed[j] & 1. Only those
    entries of `revealed` are looked at."""
    llr, pay = AM.frame_llrs(n, punctured, shortened, bob_payload, q, known)
    pu = np.asarray(punctured, np.int64)
    r = min(int(n_revealed), pu.size)
    if r:
        vals = np.asarray(revealed)[:r].astype(np.int64) & 1
        llr[pu[:r]] = np.where(vals == 1, -known, known)
    return llr, pay


def blind_loop(g, punctured, shortened, bob_payload, syndrome, q, libm, revealed, n_revealed=0, step=0,
               max_rounds=1, known=100.0, max_it=50, thr=100.0, thr_on=True):
    """One frame that is not skipped. Returns a dict: rounds, n_revealed (what the last
    decode used), leak_bits, and the last decode's record (adapt_model.decode's dict) as
    `last`, every decode's as `all`, with the payload of the decision and its flips."""
    p = len(punctured)
    nr = min(int(n_revealed), p)
    recs = []
    for t in range(max_rounds):
        llr, pay = frame_llrs(g.n, punctured, shortened, bob_payload, q, known, revealed, nr)
        recs.append(AM.decode(g, llr, syndrome, libm, max_it, thr, thr_on))
        if recs[-1]["sp_ok"] or nr >= p:
            break
        if t + 1 < max_rounds:
            nr = min(p, nr + step)
    last = recs[-1]
    payload = last["out"][pay]
    return {"rounds": len(recs), "n_revealed": nr, "leak_bits": g.m - p + nr, "last": last, "all": recs,
            "payload": payload, "corrected": int((payload ^ (np.asarray(bob_payload) & 1)).sum())}
