"""The contract of qkd_adapt_verify_tags_batch, qkd_reconcile_adaptive_verify_batch and
qkd_reconcile_blind_verify_batch restated in numpy: the payload's tag straight from the
window definition of qkd_verify.h, and the blind round loop with its closing rule, on
tests/blind_model.frame_llrs and the decoder of tests/adapt_model.py. A helper of
tests/test_adapt_verify*.py, not a test."""
import numpy as np

from tests import adapt_model as AM
from tests import blind_model as BM

MASK64 = (1 << 64) - 1


def key_words(n_bits):
    """qkd_verify_key_words: ceil((n + 63) / 64)."""
    return (n_bits + 126) >> 6 if n_bits > 0 else 0


def expand_key(seed, n_bits):
    """The seeded key string (qkd_verify_expand_key): R[k] = mix(seed + (k + 1) * golden)."""
    return [AM.mix((seed + (k + 1) * 0x9E3779B97F4A7C15) & MASK64) for k in range(key_words(n_bits))]


def window(R, k):
    """W(k): the 64-bit word whose bit i is bit k + i of the string R (a list of ints)."""
    w, s = k >> 6, k & 63
    v = int(R[w]) >> s
    if s:
        v |= (int(R[w + 1]) << (64 - s)) & MASK64
    return v


def payload_tag(R, payload, tag_bits=64):
    """The XOR of W(k) over the payload indices k whose bit (byte & 1) is set, low tag_bits."""
    t = 0
    for k in np.nonzero(np.asarray(payload) & 1)[0].tolist():
        t ^= window(R, k)
    return t & (MASK64 >> (64 - tag_bits))


def blind_loop(g, punctured, shortened, bob_payload, syndrome, q, libm, revealed, R, tag_bits=64, alice_tag=None,
               n_revealed=0, step=0, max_rounds=1, known=100.0, max_it=50, thr=100.0, thr_on=True):
    """One frame that is not skipped, as blind_model.blind_loop, closed by `verified` when
    alice_tag is given (by sp_ok when it is None). Returns blind_loop's record plus tags
    and verified per round (verified: None without alice_tag), and `tag` / `ok` of the
    last round."""
    p = len(punctured)
    nr = min(int(n_revealed), p)
    mask = MASK64 >> (64 - tag_bits)
    recs, tags, verified = [], [], []
    for t in range(max_rounds):
        llr, pay = BM.frame_llrs(g.n, punctured, shortened, bob_payload, q, known, revealed, nr)
        rec = AM.decode(g, llr, syndrome, libm, max_it, thr, thr_on)
        recs.append(rec)
        tag = payload_tag(R, rec["out"][pay], tag_bits)
        tags.append(tag)
        ok = None if alice_tag is None else bool(rec["sp_ok"] and ((tag ^ int(alice_tag)) & mask) == 0)
        verified.append(ok)
        closed = rec["sp_ok"] if alice_tag is None else ok
        if closed or nr >= p:
            break
        if t + 1 < max_rounds:
            nr = min(p, nr + step)
    last = recs[-1]
    payload = last["out"][pay]
    return {"rounds": len(recs), "n_revealed": nr, "leak_bits": g.m - p + nr, "last": last, "all": recs,
            "payload": payload, "corrected": int((payload ^ (np.asarray(bob_payload) & 1)).sum()),
            "tags": tags, "verified": verified, "tag": tags[-1], "ok": verified[-1]}
