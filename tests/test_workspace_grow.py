"""One workspace through its grow paths on the GPU: every entry point that
reserves workspace buffers (qkd_ldpc, reconcile, reconcile_adaptive and
reconcile_blind with the seeded key string and Alice's tags) at 2 frames, then 96
(every buffer is freed and reallocated), then 2 again (every buffer is reused),
once more with the checkpointed speculation forced on (its checkpoint and window
buffers), each output equal to the same call on a fresh workspace. Then the
workspace, the plan and the code are destroyed in that order and created again."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 12345
QBER = 0.02
FRAMES = (2, 96, 2)


def fields(r):
    out = {}
    for k in ("iterations", "syndromes_match", "keys_match", "bits", "corrected", "tags", "verified", "rounds",
              "n_revealed", "leak_bits"):
        v = getattr(r, k, None)
        if v is not None:
            out[k] = v.cpu().numpy()
    return out


def test_workspace_grows_shrinks_and_is_rebuilt(golden_code):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    import qkd_ldpc_amd as Q

    n = int(golden_code["dims"][0])
    rng = np.random.default_rng(77)
    big = max(FRAMES)

    def make():
        H = Q.HMatrix.from_check_lists(n, golden_code["chk_off"], golden_code["chk_idx"])
        return H, Q.AdaptPlan.choose(H, 1024, 512, 5), Q.Workspace(H)

    H, plan, W = make()
    dev = lambda a: torch.from_numpy(a).cuda()          # noqa: E731
    alice = rng.integers(0, 2, (big, n)).astype(np.uint8)
    bob = alice ^ (rng.random((big, n)) < QBER).astype(np.uint8)
    payload = rng.integers(0, 2, (big, plan.n_payload)).astype(np.uint8)
    fill = rng.integers(0, 2, (big, plan.n_punctured)).astype(np.uint8)
    bob_payload = payload ^ (rng.random(payload.shape) < QBER).astype(np.uint8)
    alice, bob, payload, fill, bob_payload = (dev(x) for x in (alice, bob, payload, fill, bob_payload))

    def inputs(H, plan):
        """Alice's announcements (they do not depend on any workspace)"""
        syn = Q.calculate_syndrome(H, alice)
        tags = Q.verify_tags(H, alice, hash_seed=SEED)
        syn_p = Q.calculate_syndrome(H, Q.adapt_embed(plan, payload, fill))
        tags_p = Q.verify_tags(plan, payload, hash_seed=SEED)
        return syn, tags, syn_p, tags_p

    NAMES = ("qkd_ldpc", "reconcile", "adaptive", "blind")

    def calls(H, plan, ws, f, ann):
        return {name: calls_one(H, plan, ws, f, ann, name) for name in NAMES}

    def fresh(H, plan, f, ann, ckpt):
        """the same calls, each on a workspace of its own"""
        out = {}
        for name in NAMES:
            ws = Q.Workspace(H)
            if ckpt:
                Q.set_debug_option("QKD_SPEC_CKPT", 1, workspace=ws)
            out[name] = calls_one(H, plan, ws, f, ann, name)
            ws.close()
        return out

    def calls_one(H, plan, ws, f, ann, name):
        syn, tags, syn_p, tags_p = ann
        if name == "qkd_ldpc":
            r = Q.qkd_ldpc(H, alice[:f], bob[:f], QBER, want_bits=True, workspace=ws)
        elif name == "reconcile":
            r = Q.reconcile(H, bob[:f], syn[:f], QBER, workspace=ws, hash_seed=SEED, alice_tags=tags[:f])
        elif name == "adaptive":
            r = Q.reconcile_adaptive(H, plan, bob_payload[:f], syn_p[:f], QBER, workspace=ws, hash_seed=SEED,
                                     alice_tags=tags_p[:f])
        else:
            r = Q.reconcile_blind(H, plan, bob_payload[:f], syn_p[:f], QBER, revealed=fill[:f], step=128,
                                  max_rounds=3, workspace=ws, hash_seed=SEED, alice_tags=tags_p[:f])
        torch.cuda.synchronize()
        return fields(r)

    def same(got, want, where):
        assert got.keys() == want.keys(), where
        for name in want:
            assert got[name].keys() == want[name].keys(), (where, name)
            for k in want[name]:
                assert np.array_equal(got[name][k], want[name][k]), (where, name, k)

    ann = inputs(H, plan)
    for ckpt in (False, True):
        if ckpt:
            Q.set_debug_option("QKD_SPEC_CKPT", 1, workspace=W)
        want = {f: fresh(H, plan, f, ann, ckpt) for f in sorted(set(FRAMES))}
        # (the inputs are decodable: the comparison below is not one of failures)
        assert want[big]["qkd_ldpc"]["keys_match"].mean() > 0.5 and want[big]["blind"]["verified"].mean() > 0.5
        for f in FRAMES:
            same(calls(H, plan, W, f, ann), want[f], (ckpt, f))
    small = want[2]

    W.close()
    plan.close()
    H.close()
    H, plan, W = make()
    Q.set_debug_option("QKD_SPEC_CKPT", 1, workspace=W)
    same(calls(H, plan, W, 2, inputs(H, plan)), small, "rebuilt")
    W.close()
    plan.close()
    H.close()
