"""Rate-adaptive reconciliation on the GPU: the erasure-aware check rule
(QKD_FLAG_ERASURES), the plan object and its embed / extract kernels, and
qkd_reconcile_adaptive_batch, against the numpy model of tests/adapt_model.py
(pinned to the oracle by tests/test_adapt_abi.py), the oracle and each other, all
by exact equality. Inputs, seeds and QBERs were chosen on the CPU with the model;
each test asserts on the model's own record that it exercises what it is for."""
import numpy as np
import pytest

from tests import adapt_model as AM

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_GOLD, M_GOLD = 10240, 5231
VERIFY_SEED, PRIVACY_SEED = 0x1234ABCD, 0x9E3779B9


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import qkd_ldpc_amd as Q
    return Q


@pytest.fixture(scope="module")
def H(Q, golden_code):
    return Q.HMatrix.from_check_lists(int(golden_code["dims"][0]), golden_code["chk_off"],
                                      golden_code["chk_idx"])


@pytest.fixture(scope="module")
def G(golden_code):
    return AM.Graph(int(golden_code["dims"][0]), golden_code["chk_off"], golden_code["chk_idx"])


def dev(x, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(x).astype(dtype)).cuda()


def host_sp(r):
    """(iterations, syndromes_match as bool, bits) of an SPResult, on the host."""
    torch.cuda.synchronize()
    return r.iterations.cpu().numpy(), r.syndromes_match.cpu().numpy().astype(bool), r.bits.cpu().numpy()


def host_rec(r):
    """(iterations, syndromes_match, payload, corrected, frames) of a ReconcileResult."""
    torch.cuda.synchronize()
    return (r.iterations.cpu().numpy(), r.syndromes_match.cpu().numpy().astype(bool), r.bits.cpu().numpy(),
            None if r.corrected is None else r.corrected.cpu().numpy(),
            None if r.frames is None else r.frames.cpu().numpy())


def of_model(ms):
    return (np.array([m["iters"] for m in ms]), np.array([m["sp_ok"] for m in ms]),
            np.stack([m["out"] for m in ms]))


def assert_same(got, want):
    assert (got[0] == want[0]).all(), (got[0], want[0])
    assert (got[1] == np.asarray(want[1], bool)).all(), (got[1], want[1])
    assert (got[2] == want[2]).all()


def keys(seed, f, n, q):
    rng = np.random.default_rng(seed)
    alice = rng.integers(0, 2, (f, n)).astype(np.uint8)
    bob = alice ^ (rng.random((f, n)) < q).astype(np.uint8)
    return rng, alice, bob


# ---- 1. the flag is inert without zeros ------------------------------------------------

@pytest.mark.parametrize("q", [0.02, 0.08])
@pytest.mark.parametrize("thr,thr_on", [(100.0, True), (0.7, True), (100.0, False)])
def test_flag_inert_without_zeros(Q, H, G, oracle_code, q, thr, thr_on):
    _, alice, bob = keys(11, 3, N_GOLD, q)
    lp = AM.log_p(q)
    llr = np.where(bob == 1, -lp, lp)
    syn = np.stack([G.syndrome(x) for x in alice])
    d_llr, d_syn = dev(llr, np.float64), dev(syn)
    on = host_sp(Q.sum_product_decoding(H, d_llr, d_syn, 50, thr, thr_on, erasures=True))
    off = host_sp(Q.sum_product_decoding(H, d_llr, d_syn, 50, thr, thr_on, erasures=False))
    want = [oracle_code.decode(llr[k], syn[k], 50, thr, thr_on) for k in range(3)]
    want = ([w["iters"] for w in want], [w["sp_ok"] for w in want], np.stack([w["out"] for w in want]))
    assert_same(on, want)
    assert_same(off, want)


@pytest.mark.parametrize("variant", ["sp_f32", "minsum"])
def test_flag_needs_the_binary64_variant(Q, H, variant):
    from qkd_ldpc_amd import _native as N
    llr = torch.ones((1, N_GOLD), dtype=torch.float64, device="cuda")
    syn = torch.zeros((1, M_GOLD), dtype=torch.uint8, device="cuda")
    with pytest.raises(Q.QkdError) as e:
        Q.sum_product_decoding(H, llr, syn, variant=variant, erasures=True)
    assert e.value.status == N.ERR_INVALID_ARG


# ---- 2. the rule against the model -------------------------------------------------------

@pytest.fixture(scope="module")
def rule_case(G, oracle_mod):
    """Golden code, 3 frames at q = 0.02, 2048 random positions with LLR 0.0, and the
    model's results (seed chosen on the CPU so that the preconditions below hold)."""
    q = 0.02
    rng, alice, bob = keys(100, 3, N_GOLD, q)
    lp = AM.log_p(q)
    llr = np.where(bob == 1, -lp, lp)
    zeros = [rng.choice(N_GOLD, 2048, replace=False) for _ in range(3)]
    for k in range(3):
        llr[k, zeros[k]] = 0.0
    syn = np.stack([G.syndrome(x) for x in alice])
    model = [AM.decode(G, llr[k], syn[k], oracle_mod.libm) for k in range(3)]
    return llr, syn, zeros, model


def test_rule_against_model(Q, H, rule_case, qkd_opt):
    llr, syn, zeros, model = rule_case
    # preconditions, on the model's own record: the test cannot pass vacuously
    assert all(m["sp_ok"] for m in model)
    assert not any(m["nan"] for m in model)
    assert any(sum(m["z1"][1:]) > 0 for m in model)       # z = 1 checks in some iteration >= 2
    assert any(sum(m["z2"][1:]) > 0 for m in model)       # z >= 2 checks in some iteration >= 2
    want = of_model(model)
    d_llr, d_syn = dev(llr, np.float64), dev(syn)
    got = host_sp(Q.sum_product_decoding(H, d_llr, d_syn, erasures=True))
    assert_same(got, want)
    qkd_opt("QKD_SPEC_CAP", 0)
    assert_same(host_sp(Q.sum_product_decoding(H, d_llr, d_syn, erasures=True)), want)
    qkd_opt("QKD_SPEC_CAP", None)
    qkd_opt("QKD_DECODE_KERNEL", "classic")
    assert_same(host_sp(Q.sum_product_decoding(H, d_llr, d_syn, erasures=True)), want)
    qkd_opt("QKD_DECODE_KERNEL", None)
    # -0.0 in place of +0.0 at the punctured positions of one frame: the same decisions
    neg = llr[:1].copy()
    neg[0, zeros[0]] = -0.0
    assert np.signbit(neg[0, zeros[0]]).all()
    got_neg = host_sp(Q.sum_product_decoding(H, dev(neg, np.float64), d_syn[:1].contiguous(), erasures=True))
    assert_same(got_neg, tuple(w[:1] for w in want))


# ---- 3. other shapes ------------------------------------------------------------------------

def regular_3_12(n, seed):
    """A (3,12)-regular code of n bits (n / 4 checks): three layers, each giving every
    bit one check and every check four bits (the first in order, the others seeded
    permutations); a bit that would meet a check twice swaps its check with a random
    bit of the same layer until none does."""
    rng = np.random.default_rng(seed)
    m = n // 4
    layers = [np.arange(n) // 4]
    for _ in range(2):
        chk = np.empty(n, np.int64)
        chk[rng.permutation(n)] = np.arange(n) // 4
        while True:
            bad = np.nonzero(np.any([chk == l for l in layers], axis=0))[0]
            if bad.size == 0:
                break
            for b in bad:
                c = rng.integers(n)
                chk[b], chk[c] = chk[c], chk[b]
        layers.append(chk)
    rows = np.sort(np.concatenate([np.argsort(l, kind="stable").reshape(m, 4) for l in layers], axis=1), axis=1)
    assert (np.diff(rows, axis=1) > 0).all()
    ptr = (12 * np.arange(m + 1)).astype(np.int32)
    idx = rows.reshape(-1).astype(np.int32)
    assert (np.bincount(idx, minlength=n) == 3).all()
    return ptr, idx


def dense_cases(g, seed, cases=12):
    """LLRs of moderate size with a sign error here and there, one or two exact zeros
    (one of them -0.0 on odd cases) and one strong known bit per frame; syndromes of
    random words."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (cases, g.n)).astype(np.uint8)
    noisy = bits ^ (rng.random((cases, g.n)) < 0.1).astype(np.uint8)
    llr = np.where(noisy == 1, -1.0, 1.0) * rng.uniform(0.5, 3.0, (cases, g.n))
    for k in range(cases):
        pos = rng.choice(g.n, 3, replace=False)
        llr[k, pos[0]] = 0.0
        if k % 2:
            llr[k, pos[1]] = -0.0
        llr[k, pos[2]] = -100.0 if bits[k, pos[2]] else 100.0
    syn = np.stack([g.syndrome(x) for x in bits])
    return llr, syn


def test_dense_codes(Q, dense_codes, oracle_mod):
    assert sorted(d.shape[1] for d in dense_codes.values()) == [6, 7, 10]
    for name, dense in sorted(dense_codes.items()):
        g = AM.Graph.from_dense(dense)
        Hd = Q.HMatrix.from_dense_array(dense)
        llr, syn = dense_cases(g, 5 + g.n)
        model = [AM.decode(g, llr[k], syn[k], oracle_mod.libm, 20) for k in range(len(llr))]
        keep = [k for k, m in enumerate(model) if not m["nan"]]
        assert len(keep) * 4 >= len(model) * 3, name          # at most a quarter skipped
        assert any(sum(model[k]["z1"]) + sum(model[k]["z2"]) > 0 for k in keep)
        got = host_sp(Q.sum_product_decoding(Hd, dev(llr, np.float64), dev(syn), 20, erasures=True))
        want = of_model(model)
        assert_same(tuple(x[keep] for x in got), tuple(x[keep] for x in want))
        Hd.close()


Q_1024 = 0.01


@pytest.mark.parametrize("n", [1024, 24576])
def test_regular_code(Q, oracle_mod, qkd_opt, n):
    """(3,12)-regular codes (the check bucket of 16): a tenth punctured, a tenth
    shortened, through the LLR entry and through reconcile_adaptive, on the split kernel
    and on the classic one (N = 24576: its large-code form, bit totals in global memory)."""
    ptr, idx = regular_3_12(n, 3)
    g = AM.Graph(n, ptr, idx)
    assert int(g.cdeg.max()) == 12
    Hr = Q.HMatrix.from_check_lists(n, ptr, idx)
    cnt = n // 5
    plan = Q.AdaptPlan.choose(Hr, cnt, cnt // 2, 9)
    rng = np.random.default_rng(77)
    pay = np.setdiff1d(np.arange(n), np.concatenate([plan.punctured, plan.shortened]))
    frames = np.zeros((2, n), np.uint8)
    frames[:, pay] = rng.integers(0, 2, (2, pay.size))
    frames[:, plan.punctured] = rng.integers(0, 2, (2, cnt // 2))
    bob = frames[:, pay] ^ (rng.random((2, pay.size)) < Q_1024).astype(np.uint8)
    syn = np.stack([g.syndrome(x) for x in frames])
    llr = np.stack([AM.frame_llrs(n, plan.punctured, plan.shortened, bob[k], Q_1024, 100.0)[0] for k in range(2)])
    model = [AM.decode(g, llr[k], syn[k], oracle_mod.libm) for k in range(2)]
    assert all(m["sp_ok"] and not m["nan"] for m in model)
    assert all((m["out"] == frames[k]).all() for k, m in enumerate(model))
    assert any(sum(m["z1"][1:]) > 0 for m in model)
    want = of_model(model)
    for kernel in (None, "classic"):
        qkd_opt("QKD_DECODE_KERNEL", kernel)
        assert_same(host_sp(Q.sum_product_decoding(Hr, dev(llr, np.float64), dev(syn), erasures=True)), want)
        r = host_rec(Q.reconcile_adaptive(Hr, plan, dev(bob), dev(syn), Q_1024, want_frames=True))
        assert_same((r[0], r[1], r[4]), want)
        assert (r[2] == frames[:, pay]).all()
        assert (r[3] == (bob ^ frames[:, pay]).sum(axis=1)).all()
    plan.close()
    Hr.close()


# ---- 4. embed and extract -----------------------------------------------------------------

def guarded(nbytes, fill=0xA5):
    """A device buffer of nbytes at an odd address between two 64-byte guards."""
    buf = torch.full((nbytes + 129,), fill, dtype=torch.uint8, device="cuda")
    view = buf[65:65 + nbytes]
    assert view.data_ptr() % 2 == 1
    return buf, view


def guards_intact(buf, nbytes, fill=0xA5):
    b = buf.cpu().numpy()
    return (b[:65] == fill).all() and (b[65 + nbytes:] == fill).all()


@pytest.mark.parametrize("f", [1, 33])
@pytest.mark.parametrize("shape", ["none", "mixed", "all_but_one"])
def test_embed_extract(Q, H, f, shape):
    from qkd_ldpc_amd import _native as N
    n = N_GOLD
    rng = np.random.default_rng(f * 10 + len(shape))
    if shape == "none":
        pu, sh = np.zeros(0, np.int32), np.zeros(0, np.int32)
    elif shape == "mixed":
        pos = rng.permutation(n)[:1500].astype(np.int32)
        pu, sh = pos[:700], pos[700:]
    else:
        pos = rng.permutation(n)[:n - 1].astype(np.int32)
        pu, sh = pos[:4000], pos[4000:]
    plan = Q.AdaptPlan(H, pu, sh)
    p, npay = len(pu), n - len(pu) - len(sh)
    assert plan.n_payload == npay and plan.n_punctured == p and plan.n_shortened == len(sh)
    pay = np.setdiff1d(np.arange(n), np.concatenate([pu, sh]))
    bits = rng.integers(0, 2, (f, npay)).astype(np.uint8)
    # only byte & 1 counts: 0xFF is a 1, 0xFE a 0
    raw = np.where(bits == 1, rng.choice([1, 0xFF], (f, npay)), rng.choice([0, 0xFE], (f, npay))).astype(np.uint8)
    fill_bits = rng.integers(0, 2, (f, p)).astype(np.uint8)
    fill_raw = (fill_bits | (rng.integers(0, 2, (f, p)) * 0xFE)).astype(np.uint8)
    want = np.full((f, n), 0x55, np.uint8)
    want[:, pay] = bits
    if p:
        want[:, pu] = fill_bits                   # fill byte r goes to the r-th punctured position
    want[:, sh] = 0
    assert not (want == 0x55).any()
    # rows at an odd address, outputs between guards, through the C entry itself
    _, d_pay = guarded(f * npay)
    d_pay.copy_(dev(raw).reshape(-1))
    _, d_fill = guarded(max(f * p, 1))
    if p:
        d_fill[:f * p].copy_(dev(fill_raw).reshape(-1))
    fbuf, d_frames = guarded(f * n)
    stream = int(torch.cuda.current_stream().cuda_stream)
    N.check(N.lib().qkd_adapt_embed_batch(plan.handle, d_pay.data_ptr(), f, d_fill.data_ptr() if p else None,
                                          d_frames.data_ptr(), stream))
    torch.cuda.synchronize()
    assert (d_frames.cpu().numpy().reshape(f, n) == want).all()
    assert guards_intact(fbuf, f * n)
    obuf, d_out = guarded(f * npay)
    N.check(N.lib().qkd_adapt_extract_batch(plan.handle, d_frames.data_ptr(), f, d_out.data_ptr(), stream))
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy().reshape(f, npay) == want[:, pay]).all()          # numpy fancy indexing
    assert (d_out.cpu().numpy().reshape(f, npay) == bits).all()                   # extract(embed(x)) == x
    assert guards_intact(obuf, f * npay)
    # and the wrappers
    frames = Q.adapt_embed(plan, dev(raw), dev(fill_raw) if p else None)
    assert (frames.cpu().numpy() == want).all()
    assert (Q.adapt_extract(plan, frames).cpu().numpy() == bits).all()
    plan.close()


# ---- 5. reconcile_adaptive against its definition -------------------------------------------

Q_DEF = 0.03


def adaptive_case(Q, H, G, p, s, seed, q):
    """3 golden frames for AdaptPlan.choose(p + s, p): Alice's frames (embedded on the
    host), their syndromes, Bob's payload and the contract's LLRs for a known_llr."""
    plan = Q.AdaptPlan.choose(H, p + s, p, 5)
    rng = np.random.default_rng(seed)
    pay = np.setdiff1d(np.arange(G.n), np.concatenate([plan.punctured, plan.shortened]))
    assert pay.size == plan.n_payload == G.n - p - s
    frames = np.zeros((3, G.n), np.uint8)
    frames[:, pay] = rng.integers(0, 2, (3, pay.size))
    frames[:, plan.punctured] = rng.integers(0, 2, (3, p))
    bob = frames[:, pay] ^ (rng.random((3, pay.size)) < q).astype(np.uint8)
    syn = np.stack([G.syndrome(x) for x in frames])

    def llrs(known):
        return np.stack([AM.frame_llrs(G.n, plan.punctured, plan.shortened, bob[k], q, known)[0] for k in range(3)])
    return plan, pay, frames, bob, syn, llrs


def check_definition(Q, H, G, libm, case, known, thr_on):
    plan, pay, frames, bob, syn, llrs = case
    llr = llrs(known)
    assert (np.count_nonzero(llr == 0.0, axis=1) == plan.n_punctured).all()
    model = [AM.decode(G, llr[k], syn[k], libm, 50, 100.0, thr_on) for k in range(3)]
    assert not any(m["nan"] for m in model)
    want = of_model(model)
    d_syn = dev(syn)
    via_llr = host_sp(Q.sum_product_decoding(H, dev(llr, np.float64), d_syn, 50, 100.0, thr_on, erasures=True))
    assert_same(via_llr, want)
    r = host_rec(Q.reconcile_adaptive(H, plan, dev(bob), d_syn, Q_DEF, known, 50, 100.0, thr_on,
                                      want_frames=True))
    assert_same((r[0], r[1], r[4]), want)
    assert (r[2] == want[2][:, pay]).all()
    assert (r[3] == (want[2][:, pay] ^ bob).sum(axis=1)).all()
    # the optional outputs left out: the same payload
    r2 = host_rec(Q.reconcile_adaptive(H, plan, dev(bob), d_syn, Q_DEF, known, 50, 100.0, thr_on,
                                       want_corrected=False))
    assert r2[3] is None and r2[4] is None
    assert_same(r2[:3], r[:3])
    # the classic kernel (class bytes and payload map in the original bit order)
    Q.set_debug_option("QKD_DECODE_KERNEL", "classic")
    try:
        r3 = host_rec(Q.reconcile_adaptive(H, plan, dev(bob), d_syn, Q_DEF, known, 50, 100.0, thr_on,
                                           want_frames=True))
    finally:
        Q.set_debug_option("QKD_DECODE_KERNEL", None)
    assert_same(r3[:3], r[:3])
    assert (r3[3] == r[3]).all() and (r3[4] == r[4]).all()
    return model, r


@pytest.mark.parametrize("p,s", [(0, 0), (1024, 0), (0, 1024), (300, 724)])
def test_reconcile_adaptive_definition(Q, H, G, oracle_mod, p, s):
    case = adaptive_case(Q, H, G, p, s, 300 + p + s, Q_DEF)
    plan, pay, frames, bob, syn, _ = case
    model, r = check_definition(Q, H, G, oracle_mod.libm, case, 100.0, True)
    assert all(m["sp_ok"] for m in model)
    assert (r[2] == frames[:, pay]).all()                 # (these frames decode to Alice's)
    if p:
        assert any(sum(m["z1"][1:]) > 0 for m in model)    # zeros survive the first iteration
    if p == 0 and s == 0:
        torch.cuda.synchronize()
        rr = Q.reconcile(H, dev(bob), dev(syn), Q_DEF)
        torch.cuda.synchronize()
        assert (rr.iterations.cpu().numpy() == r[0]).all()
        assert (rr.syndromes_match.cpu().numpy().astype(bool) == r[1]).all()
        assert (rr.bits.cpu().numpy() == r[2]).all()
        assert (rr.corrected.cpu().numpy() == r[3]).all()
    plan.close()


@pytest.mark.parametrize("known,thr_on", [(100.0, False), (37.0, True)])
def test_reconcile_adaptive_threshold_off_and_known(Q, H, G, oracle_mod, known, thr_on):
    case = adaptive_case(Q, H, G, 300, 724, 1324, Q_DEF)
    check_definition(Q, H, G, oracle_mod.libm, case, known, thr_on)
    case[0].close()


# ---- 6. the capability -------------------------------------------------------------------

def test_capability(Q, H, G, oracle_mod):
    """QBER 0.10: the mother code alone fails; with 2048 shortened positions Bob gets
    Alice's payload. The model says both first."""
    q, seed = 0.10, 200
    _, alice, bob = keys(seed, 3, N_GOLD, q)
    plan = Q.AdaptPlan.choose(H, 2048, 0, seed)
    pay = np.setdiff1d(np.arange(N_GOLD), plan.shortened)
    lp = AM.log_p(q)
    syn_plain = np.stack([G.syndrome(x) for x in alice])
    plain = [AM.decode(G, np.where(bob[k] == 1, -lp, lp), syn_plain[k], oracle_mod.libm) for k in range(3)]
    assert not any(m["sp_ok"] for m in plain)
    frames = np.zeros_like(alice)
    frames[:, pay] = alice[:, pay]
    syn = np.stack([G.syndrome(x) for x in frames])
    short = [AM.decode(G, AM.frame_llrs(N_GOLD, [], plan.shortened, bob[k][pay], q, 100.0)[0], syn[k],
                       oracle_mod.libm) for k in range(3)]
    assert all(m["sp_ok"] and (m["out"] == frames[k]).all() for k, m in enumerate(short))
    r0 = Q.reconcile(H, dev(bob), dev(syn_plain), q)
    torch.cuda.synchronize()
    assert (r0.syndromes_match.cpu().numpy() == 0).all()
    assert (r0.iterations.cpu().numpy() == 50).all()
    # Alice's half on the device: embed, then the syndrome
    d_frames = Q.adapt_embed(plan, dev(alice[:, pay]))
    assert (d_frames.cpu().numpy() == frames).all()
    r = host_rec(Q.reconcile_adaptive(H, plan, dev(bob[:, pay]), Q.calculate_syndrome(H, d_frames), q))
    assert r[1].all()
    assert (r[2] == alice[:, pay]).all()
    assert (r[0] == [m["iters"] for m in short]).all()
    assert (r[3] == (alice[:, pay] ^ bob[:, pay]).sum(axis=1)).all()
    plan.close()


# ---- 7. the chain ---------------------------------------------------------------------------

def test_chain(Q, H, G):
    """embed -> syndrome -> tags | reconcile_adaptive -> tags -> verified -> privacy
    amplification; one frame's syndrome has 7 checks flipped and must leave as zeros."""
    q, p, s, out_bits = 0.03, 512, 512, 3000
    plan = Q.AdaptPlan.choose(H, p + s, p, 21)
    rng = np.random.default_rng(4)
    payload = rng.integers(0, 2, (3, plan.n_payload)).astype(np.uint8)
    fill = rng.integers(0, 2, (3, p)).astype(np.uint8)
    bob = payload ^ (rng.random(payload.shape) < q).astype(np.uint8)
    # Alice
    d_payload = dev(payload)
    syn = Q.calculate_syndrome(H, Q.adapt_embed(plan, d_payload, dev(fill)))
    alice_tags = Q.privacy_amplify(d_payload, 64, hash_seed=VERIFY_SEED)
    alice_secret = Q.privacy_amplify(d_payload, out_bits, hash_seed=PRIVACY_SEED)
    bad = syn.clone()
    flip = torch.from_numpy(rng.choice(M_GOLD, 7, replace=False)).cuda()
    bad[1, flip] ^= 1
    # Bob
    r = Q.reconcile_adaptive(H, plan, dev(bob), bad, q)
    tags = Q.privacy_amplify(r.bits, 64, hash_seed=VERIFY_SEED)
    verified = (r.syndromes_match.bool() & (tags[:, 0] == alice_tags[:, 0])).to(torch.uint8).contiguous()
    secret = Q.privacy_amplify(r.bits, out_bits, hash_seed=PRIVACY_SEED, keep=verified)
    torch.cuda.synchronize()
    v = verified.cpu().numpy().astype(bool)
    assert v.tolist() == [True, False, True]
    got, want = secret.cpu().numpy(), alice_secret.cpu().numpy()
    assert (got[v] == want[v]).all()
    assert (got[~v] == 0).all()
    assert (r.bits.cpu().numpy()[v] == payload[v]).all()
    assert want.any()
    plan.close()


# ---- 8. argument errors, before any device work --------------------------------------------

def test_argument_errors(Q, H, dense_codes):
    from qkd_ldpc_amd import _native as N

    def invalid(fn, *a, **kw):
        with pytest.raises(Q.QkdError) as e:
            fn(*a, **kw)
        assert e.value.status == N.ERR_INVALID_ARG, e.value

    invalid(Q.AdaptPlan, H, [1, 2, 2], [])                     # duplicate
    invalid(Q.AdaptPlan, H, [1, 2], [2, 3])                    # duplicate across the lists
    invalid(Q.AdaptPlan, H, [N_GOLD], [])                      # out of range
    invalid(Q.AdaptPlan, H, [], [-1])
    invalid(Q.AdaptPlan, H, np.arange(5000), np.arange(5000, N_GOLD))      # p + s = N
    plan = Q.AdaptPlan(H, [3, 1], [7])
    assert (plan.n_bits, plan.n_payload, plan.n_punctured, plan.n_shortened) == (N_GOLD, N_GOLD - 3, 2, 1)
    pay = torch.zeros((1, plan.n_payload), dtype=torch.uint8, device="cuda")
    syn = torch.zeros((1, M_GOLD), dtype=torch.uint8, device="cuda")
    invalid(Q.adapt_embed, plan, pay)                          # fill missing with p > 0
    plain = Q.AdaptPlan(H)
    invalid(Q.adapt_embed, plain, torch.zeros((1, N_GOLD), dtype=torch.uint8, device="cuda"),
            torch.zeros((1, 1), dtype=torch.uint8, device="cuda"))           # fill without p
    for known in (0.0, -1.0, float("nan"), float("inf")):
        invalid(Q.reconcile_adaptive, H, plan, pay, syn, 0.02, known)
    invalid(Q.reconcile_adaptive, H, plan, torch.zeros((1, N_GOLD), dtype=torch.uint8, device="cuda"), syn, 0.02)
    invalid(Q.adapt_embed, plan, torch.zeros((1, N_GOLD), dtype=torch.uint8, device="cuda"),
            torch.zeros((1, 2), dtype=torch.uint8, device="cuda"))
    invalid(Q.adapt_extract, plan, pay)
    invalid(Q.reconcile_adaptive, H, plan, pay, syn, 0.0)                      # as reconcile validates
    invalid(Q.reconcile_adaptive, H, plan, pay, syn, 0.02, 100.0, 0)
    # a plan created for another code (same sizes, so only the library can tell)
    cptr, cidx, _, _ = H.adjacency()
    H2 = Q.HMatrix.from_check_lists(N_GOLD, cptr, cidx)
    other = Q.AdaptPlan(H2, [3, 1], [7])
    invalid(Q.reconcile_adaptive, H, other, pay, syn, 0.02)
    # the call that all of these are variations of is valid
    r = Q.reconcile_adaptive(H, plan, pay, syn, 0.02)
    torch.cuda.synchronize()
    assert r.syndromes_match.cpu().numpy().all() and not r.bits.cpu().numpy().any()
    for x in (plan, plain, other):
        x.close()
    H2.close()
