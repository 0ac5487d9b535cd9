// Host build of what qkd_reconcile_blind_batch adds to the argument check of
// qkd_reconcile_adaptive_batch (qkd_args.h reconcile_blind_args_error and
// reconcile_blind_revealed_error): the plan or the reveal counts missing, the
// round count, the step (required from two rounds on, free with one), the
// revealed bytes against the punctured count, and the order of the answers.
// Prints the number of wrong answers ("0" when all hold). Built plain and
// under AddressSanitizer + UBSan by tests/test_blind_abi.py; a stand-alone
// program, host code only.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../qkd_ldpc_amd/csrc/qkd_args.h"

int main() {
    int plan_obj = 0;
    const void* plan = &plan_obj;
    uint32_t nrev[2] = {0, 3};
    uint8_t revealed[8] = {0, 1, 0, 1, 1, 0, 1, 0};
    int bad = 0;
    auto expect = [&](const char* got, const char* want, const char* what) {
        const bool same = (got == nullptr && want == nullptr) || (got && want && !strcmp(got, want));
        if (!same) {
            fprintf(stderr, "%s: got '%s', want '%s'\n", what, got ? got : "(ok)", want ? want : "(ok)");
            bad++;
        }
    };
    using qkda::reconcile_blind_args_error;
    using qkda::reconcile_blind_revealed_error;
    const char* const kNull = "null argument";
    const char* const kRounds = "max_rounds must be >= 1";
    const char* const kStep = "step must be >= 1 when max_rounds > 1";
    const char* const kRevealed = "revealed is required exactly when the plan punctures";
    expect(reconcile_blind_args_error(plan, nrev, 0, 1), nullptr, "one round, no step");
    expect(reconcile_blind_args_error(plan, nrev, 256, 1), nullptr, "one round, a step");
    expect(reconcile_blind_args_error(plan, nrev, 1, 2), nullptr, "two rounds");
    expect(reconcile_blind_args_error(plan, nrev, 0xffffffffu, 0xffffffffu), nullptr, "the largest values");
    expect(reconcile_blind_args_error(nullptr, nrev, 1, 1), kNull, "plan");
    expect(reconcile_blind_args_error(plan, nullptr, 1, 1), kNull, "n_revealed");
    expect(reconcile_blind_args_error(nullptr, nullptr, 1, 1), kNull, "both");
    // null arguments come first, whatever else is wrong
    expect(reconcile_blind_args_error(nullptr, nrev, 0, 0), kNull, "order: plan");
    expect(reconcile_blind_args_error(plan, nullptr, 0, 5), kNull, "order: n_revealed");
    expect(reconcile_blind_args_error(plan, nrev, 0, 0), kRounds, "no round");
    expect(reconcile_blind_args_error(plan, nrev, 7, 0), kRounds, "no round, a step");
    expect(reconcile_blind_args_error(plan, nrev, 0, 2), kStep, "two rounds, no step");
    expect(reconcile_blind_args_error(plan, nrev, 0, 0xffffffffu), kStep, "many rounds, no step");
    expect(reconcile_blind_revealed_error(4, revealed), nullptr, "p > 0 with revealed");
    expect(reconcile_blind_revealed_error(0, nullptr), nullptr, "p = 0 without");
    expect(reconcile_blind_revealed_error(4, nullptr), kRevealed, "p > 0 without");
    expect(reconcile_blind_revealed_error(0, revealed), kRevealed, "p = 0 with");
    expect(reconcile_blind_revealed_error(1, nullptr), kRevealed, "p = 1 without");
    printf("%d\n", bad);
    return bad ? 1 : 0;
}
