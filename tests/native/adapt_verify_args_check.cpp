// Host build of the argument checks of qkd_adapt_verify_tags_batch,
// qkd_reconcile_adaptive_verify_batch and qkd_reconcile_blind_verify_batch
// (qkd_args.h adapt_verify_tags_args_error, reconcile_adaptive_verify_args_error,
// reconcile_blind_verify_args_error): the plan missing, the tag width, the
// tags to give or to compare with, verified exactly with alice_tags, the blind
// entry's round count and step, and the order of the answers. Prints the
// number of wrong answers ("0" when all hold). Built plain and under
// AddressSanitizer + UBSan by tests/test_adapt_verify_abi.py; a stand-alone
// program, host code only.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../qkd_ldpc_amd/csrc/qkd_args.h"

int main() {
    int plan_obj = 0;
    const void* plan = &plan_obj;
    uint8_t payload[8] = {0, 1, 0, 1, 1, 0, 1, 0};
    uint32_t nrev[2] = {0, 3};
    uint64_t alice[2] = {1, 2}, tags[2] = {0, 0};
    uint8_t verified[2] = {0, 0};
    int bad = 0;
    auto expect = [&](const char* got, const char* want, const char* what) {
        const bool same = (got == nullptr && want == nullptr) || (got && want && !strcmp(got, want));
        if (!same) {
            fprintf(stderr, "%s: got '%s', want '%s'\n", what, got ? got : "(ok)", want ? want : "(ok)");
            bad++;
        }
    };
    using qkda::adapt_verify_tags_args_error;
    using qkda::reconcile_adaptive_verify_args_error;
    using qkda::reconcile_blind_verify_args_error;
    const char* const kNull = "null argument";
    const char* const kFrames = "n_frames must be > 0";
    const char* const kMany = "n_frames too large";
    const char* const kBits = "tag_bits must be in 1..64";
    const char* const kNone = "neither alice_tags nor tags_out given";
    const char* const kNoVer = "alice_tags given without verified";
    const char* const kNoAlice = "verified given without alice_tags";
    const char* const kRounds = "max_rounds must be >= 1";
    const char* const kStep = "step must be >= 1 when max_rounds > 1";

    // Alice's half
    expect(adapt_verify_tags_args_error(plan, payload, 1, 64, tags), nullptr, "tags: valid");
    expect(adapt_verify_tags_args_error(plan, payload, 2, 1, tags), nullptr, "tags: one bit");
    expect(adapt_verify_tags_args_error(nullptr, payload, 1, 64, tags), kNull, "tags: plan");
    expect(adapt_verify_tags_args_error(plan, nullptr, 1, 64, tags), kNull, "tags: payload");
    expect(adapt_verify_tags_args_error(plan, payload, 1, 64, nullptr), kNull, "tags: tags");
    expect(adapt_verify_tags_args_error(nullptr, payload, 0, 0, tags), kNull, "tags: order");
    expect(adapt_verify_tags_args_error(plan, payload, 0, 64, tags), kFrames, "tags: no frame");
    expect(adapt_verify_tags_args_error(plan, payload, (size_t)0x100000000ull, 64, tags), kMany, "tags: too many");
    expect(adapt_verify_tags_args_error(plan, payload, 1, 0, tags), kBits, "tags: 0 bits");
    expect(adapt_verify_tags_args_error(plan, payload, 1, 65, tags), kBits, "tags: 65 bits");
    expect(adapt_verify_tags_args_error(plan, payload, 0, 65, tags), kFrames, "tags: frames before bits");

    // Bob's half, rate-adaptive
    expect(reconcile_adaptive_verify_args_error(plan, 64, alice, tags, verified), nullptr, "adaptive: all");
    expect(reconcile_adaptive_verify_args_error(plan, 13, alice, nullptr, verified), nullptr, "adaptive: compare only");
    expect(reconcile_adaptive_verify_args_error(plan, 1, nullptr, tags, nullptr), nullptr, "adaptive: tags only");
    expect(reconcile_adaptive_verify_args_error(nullptr, 64, alice, tags, verified), kNull, "adaptive: plan");
    expect(reconcile_adaptive_verify_args_error(nullptr, 0, nullptr, nullptr, nullptr), kNull, "adaptive: order");
    expect(reconcile_adaptive_verify_args_error(plan, 0, alice, tags, verified), kBits, "adaptive: 0 bits");
    expect(reconcile_adaptive_verify_args_error(plan, 65, alice, tags, verified), kBits, "adaptive: 65 bits");
    expect(reconcile_adaptive_verify_args_error(plan, 0xffffffffu, alice, tags, verified), kBits, "adaptive: huge");
    expect(reconcile_adaptive_verify_args_error(plan, 0, nullptr, nullptr, nullptr), kBits, "adaptive: bits first");
    expect(reconcile_adaptive_verify_args_error(plan, 64, nullptr, nullptr, nullptr), kNone, "adaptive: nothing");
    expect(reconcile_adaptive_verify_args_error(plan, 64, nullptr, nullptr, verified), kNone, "adaptive: verified alone");
    expect(reconcile_adaptive_verify_args_error(plan, 64, alice, tags, nullptr), kNoVer, "adaptive: no verified");
    expect(reconcile_adaptive_verify_args_error(plan, 64, alice, nullptr, nullptr), kNoVer, "adaptive: alice alone");
    expect(reconcile_adaptive_verify_args_error(plan, 64, nullptr, tags, verified), kNoAlice, "adaptive: no alice");

    // Bob's half, blind
    expect(reconcile_blind_verify_args_error(plan, nrev, 0, 1, 64, alice, tags, verified), nullptr, "blind: one round");
    expect(reconcile_blind_verify_args_error(plan, nrev, 256, 6, 13, alice, nullptr, verified), nullptr, "blind: six");
    expect(reconcile_blind_verify_args_error(plan, nrev, 1, 2, 1, nullptr, tags, nullptr), nullptr, "blind: tags only");
    expect(reconcile_blind_verify_args_error(plan, nrev, 0xffffffffu, 0xffffffffu, 64, alice, tags, verified), nullptr,
           "blind: the largest values");
    expect(reconcile_blind_verify_args_error(nullptr, nrev, 1, 1, 64, alice, tags, verified), kNull, "blind: plan");
    expect(reconcile_blind_verify_args_error(plan, nullptr, 1, 1, 64, alice, tags, verified), kNull, "blind: counts");
    expect(reconcile_blind_verify_args_error(nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr), kNull, "blind: order");
    expect(reconcile_blind_verify_args_error(plan, nrev, 0, 0, 0, nullptr, nullptr, nullptr), kRounds, "blind: no round");
    expect(reconcile_blind_verify_args_error(plan, nrev, 0, 2, 0, nullptr, nullptr, nullptr), kStep, "blind: no step");
    expect(reconcile_blind_verify_args_error(plan, nrev, 1, 2, 0, alice, tags, verified), kBits, "blind: 0 bits");
    expect(reconcile_blind_verify_args_error(plan, nrev, 1, 2, 65, alice, tags, verified), kBits, "blind: 65 bits");
    expect(reconcile_blind_verify_args_error(plan, nrev, 1, 2, 64, nullptr, nullptr, nullptr), kNone, "blind: nothing");
    expect(reconcile_blind_verify_args_error(plan, nrev, 1, 2, 64, alice, tags, nullptr), kNoVer, "blind: no verified");
    expect(reconcile_blind_verify_args_error(plan, nrev, 1, 2, 64, nullptr, tags, verified), kNoAlice, "blind: no alice");
    printf("%d\n", bad);
    return bad ? 1 : 0;
}
