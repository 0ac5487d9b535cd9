// Host build of qkd_reconcile_batch's argument check (qkd_args.h
// reconcile_args_error): every required pointer missing in turn, the frame
// count limits, the QBER range (NaN and the end points included), and an
// acceptable call. Prints the number of wrong answers ("0" when all hold).
// Built plain and under AddressSanitizer + UBSan by
// tests/test_reconcile_abi.py; a stand-alone program, host code only.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../qkd_ldpc_amd/csrc/qkd_args.h"

int main() {
    int code_obj = 0;
    uint8_t bob[4] = {0, 1, 0, 1}, syn[2] = {1, 0}, bits[4] = {0, 0, 0, 0}, ok[1] = {0};
    uint32_t it[1] = {0};
    const void* code = &code_obj;
    int bad = 0;
    auto expect = [&](const char* got, const char* want, const char* what) {
        const bool same = (got == nullptr && want == nullptr) || (got && want && !strcmp(got, want));
        if (!same) {
            fprintf(stderr, "%s: got '%s', want '%s'\n", what, got ? got : "(ok)", want ? want : "(ok)");
            bad++;
        }
    };
    using qkda::reconcile_args_error;
    expect(reconcile_args_error(code, bob, syn, 1, 0.02, bits, it, ok), nullptr, "valid");
    expect(reconcile_args_error(nullptr, bob, syn, 1, 0.02, bits, it, ok), "null argument", "code");
    expect(reconcile_args_error(code, nullptr, syn, 1, 0.02, bits, it, ok), "null argument", "bob");
    expect(reconcile_args_error(code, bob, nullptr, 1, 0.02, bits, it, ok), "null argument", "syndrome");
    expect(reconcile_args_error(code, bob, syn, 1, 0.02, nullptr, it, ok), "null argument", "bits_out");
    expect(reconcile_args_error(code, bob, syn, 1, 0.02, bits, nullptr, ok), "null argument", "iterations");
    expect(reconcile_args_error(code, bob, syn, 1, 0.02, bits, it, nullptr), "null argument", "syndromes_match");
    // null arguments come first, whatever else is wrong
    expect(reconcile_args_error(nullptr, bob, syn, 0, 7.0, bits, it, ok), "null argument", "order");
    expect(reconcile_args_error(code, bob, syn, 0, 0.02, bits, it, ok), "n_frames must be > 0", "no frames");
    expect(reconcile_args_error(code, bob, syn, (size_t)0xffffffffull, 0.02, bits, it, ok), nullptr, "2^32 - 1 frames");
    if (sizeof(size_t) > 4)
        expect(reconcile_args_error(code, bob, syn, (size_t)0x100000000ull, 0.02, bits, it, ok), "n_frames too large",
               "2^32 frames");
    const double bad_q[] = {0.0, -0.0, 1.0, -0.1, 1.5, NAN, INFINITY, -INFINITY};
    for (double q : bad_q) expect(reconcile_args_error(code, bob, syn, 1, q, bits, it, ok), "QBER must be in (0,1)", "qber");
    const double good_q[] = {5e-324, 0.5, 0.7, 0.9999999999999999};
    for (double q : good_q) expect(reconcile_args_error(code, bob, syn, 1, q, bits, it, ok), nullptr, "qber ok");
    printf("%d\n", bad);
    return bad ? 1 : 0;
}
