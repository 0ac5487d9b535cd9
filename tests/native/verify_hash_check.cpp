// Host build of the key verification hash (qkd_verify.h) and of the argument
// checks of its two entry points (qkd_args.h): the tag taken the way the
// kernels take it (windows of the key string from two adjacent words, XORed
// per set key bit, masked; and the kernels' own inner step, runs of 1, 4 and 8
// positions in 32-bit operations) against the brute-force matrix form
// tag bit i = XOR_p r[p + i] x_p, at N = 1, 63, 64, 65, 127, 128, 10240 and
// t = 1, 13, 64, with a seeded and with an arbitrary key string; the nesting
// property (a t-bit tag is the low t bits of the 64-bit one); the word count;
// the SplitMix64 known answers. Prints the number of wrong answers ("0" when
// all hold). Built plain and under AddressSanitizer + UBSan by
// tests/test_verify_abi.py; a stand-alone program, host code only. The key
// string is held in exactly W words, so a window that read past it would be
// caught by the sanitizer.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../qkd_ldpc_amd/csrc/qkd_args.h"
#include "../../qkd_ldpc_amd/csrc/qkd_verify.h"

static int bad = 0;

static void expect(bool ok, const char* what, long a = 0, long b = 0) {
    if (!ok) {
        fprintf(stderr, "%s (%ld, %ld)\n", what, a, b);
        bad++;
    }
}

static void expect_msg(const char* got, const char* want, const char* what) {
    const bool same = (got == nullptr && want == nullptr) || (got && want && !strcmp(got, want));
    if (!same) {
        fprintf(stderr, "%s: got '%s', want '%s'\n", what, got ? got : "(ok)", want ? want : "(ok)");
        bad++;
    }
}

// the kernels' form: one window per set key bit (a key bit is byte & 1)
static uint64_t tag_windows(const std::vector<uint64_t>& R, const std::vector<uint8_t>& x, uint32_t t) {
    uint64_t acc = 0;
    for (size_t p = 0; p < x.size(); ++p) {
        const size_t w = p >> 6;
        const uint32_t s = (uint32_t)(p & 63);
        // (at s = 0 the window drops its second word, which may lie past the string)
        const uint64_t hi = s ? R[w + 1] : 0;
        acc ^= qkdv::verify_window(R[w], hi, s) & (0ull - (uint64_t)(x[p] & 1));
    }
    return acc & qkdv::verify_tag_mask(t);
}

// the kernels' inner step (verify_xor_run: CNT positions a call, 32-bit
// operations) over a key of n % CNT == 0 bits; the string padded by one word
template <int CNT>
static uint64_t tag_runs(std::vector<uint64_t> R, const std::vector<uint8_t>& x, uint32_t t) {
    R.push_back(0);
    std::vector<uint32_t> r32(2 * R.size());
    for (size_t k = 0; k < R.size(); ++k) {          // (the byte order of the host does not matter here)
        r32[2 * k] = (uint32_t)R[k];
        r32[2 * k + 1] = (uint32_t)(R[k] >> 32);
    }
    uint64_t acc = 0;
    for (size_t p = 0; p < x.size(); p += CNT) {
        uint64_t b = 0;
        for (int j = 0; j < CNT; ++j) b |= (uint64_t)x[p + j] << (8 * j);
        acc ^= qkdv::verify_xor_run<CNT>(r32.data(), (uint32_t)p, b);
    }
    return acc & qkdv::verify_tag_mask(t);
}

// the matrix form, bit by bit
static uint64_t tag_matrix(const std::vector<uint64_t>& R, const std::vector<uint8_t>& x, uint32_t t) {
    auto r = [&](size_t k) -> uint64_t { return (R[k >> 6] >> (k & 63)) & 1u; };
    uint64_t tag = 0;
    for (uint32_t i = 0; i < t; ++i) {
        uint64_t b = 0;
        for (size_t p = 0; p < x.size(); ++p) b ^= r(p + i) & (uint64_t)(x[p] & 1);
        tag |= b << i;
    }
    return tag;
}

int main() {
    using namespace qkdv;
    // SplitMix64, seed 0
    expect(verify_key_word(0, 0) == 0xE220A8397B1DCDAFull, "R[0]");
    expect(verify_key_word(0, 1) == 0x6E789E6AA1B965F4ull, "R[1]");
    expect(verify_key_word(0, 2) == 0x06C45D188009454Full, "R[2]");
    // W = ceil((N + 63) / 64): bits 0 .. N + 62 of the string exist
    const int32_t ns[] = {1, 2, 64, 65, 66, 10240, 131072};
    const size_t ws[] = {1, 2, 2, 2, 3, 161, 2049};
    for (int k = 0; k < 7; ++k) expect(verify_key_words(ns[k]) == ws[k], "key words", ns[k], (long)verify_key_words(ns[k]));
    expect(verify_key_words(0) == 0 && verify_key_words(-5) == 0, "key words of no bits");
    expect(verify_tag_mask(1) == 1ull && verify_tag_mask(13) == 0x1fffull && verify_tag_mask(64) == ~0ull, "mask");
    // the window at the shifts' ends
    expect(verify_window(0x8000000000000001ull, ~0ull, 0) == 0x8000000000000001ull, "window s = 0");
    expect(verify_window(0x8000000000000000ull, 1ull, 63) == 3ull, "window s = 63");
    expect(verify_window(0ull, 0x8000000000000001ull, 1) == 0x8000000000000000ull, "window s = 1");
    expect(verify_funnel(0x80000001u, 0x00000003u, 0) == 3u && verify_funnel(0x80000001u, 0x00000003u, 1) == 0x80000001u &&
               verify_funnel(0x80000001u, 0x00000003u, 31) == 2u, "funnel");

    const int32_t sizes[] = {1, 63, 64, 65, 127, 128, 10240};
    const uint32_t tbits[] = {1, 13, 64};
    uint64_t lcg = 0x243F6A8885A308D3ull;
    auto next = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg >> 11; };
    for (int32_t n : sizes) {
        for (int form = 0; form < 2; ++form) {
            std::vector<uint64_t> R(verify_key_words(n));
            for (size_t k = 0; k < R.size(); ++k) R[k] = form ? (next() << 32) ^ next() : verify_key_word(12345, k);
            // keys: all zero, all one, a single bit at either end, random bytes
            // with high bits set (only byte & 1 counts)
            for (int key = 0; key < 6; ++key) {
                std::vector<uint8_t> x((size_t)n, 0);
                if (key == 1) for (auto& b : x) b = 1;
                if (key == 2) x[0] = 1;
                if (key == 3) x[(size_t)n - 1] = 0xff;
                if (key >= 4) for (auto& b : x) b = (uint8_t)next();
                const uint64_t full = tag_windows(R, x, 64);
                if (key == 0) expect(full == 0, "all-zero key", n);
                if (key == 2) expect(full == R[0], "bit 0 alone gives R[0]", n);
                for (uint32_t t : tbits) {
                    const uint64_t a = tag_windows(R, x, t);
                    expect(a == tag_matrix(R, x, t), "windows != matrix", n, t);
                    expect(a == (full & verify_tag_mask(t)), "nesting", n, t);
                    expect(a == tag_runs<1>(R, x, t), "runs of 1", n, t);
                    if (n % 4 == 0) expect(a == tag_runs<4>(R, x, t), "runs of 4", n, t);
                    if (n % 8 == 0) expect(a == tag_runs<8>(R, x, t), "runs of 8", n, t);
                }
            }
        }
    }

    // argument checks
    int code_obj = 0;
    const void* code = &code_obj;
    uint8_t bits[4] = {0, 1, 0, 1}, ver[1] = {0};
    uint64_t tags[1] = {0};
    using qkda::reconcile_verify_args_error;
    using qkda::verify_tags_args_error;
    expect_msg(verify_tags_args_error(code, bits, 1, 64, tags), nullptr, "valid");
    expect_msg(verify_tags_args_error(code, bits, 1, 1, tags), nullptr, "one bit");
    expect_msg(verify_tags_args_error(nullptr, bits, 1, 64, tags), "null argument", "code");
    expect_msg(verify_tags_args_error(code, nullptr, 1, 64, tags), "null argument", "bits");
    expect_msg(verify_tags_args_error(code, bits, 1, 64, nullptr), "null argument", "tags");
    expect_msg(verify_tags_args_error(nullptr, bits, 0, 0, tags), "null argument", "order");
    expect_msg(verify_tags_args_error(code, bits, 0, 64, tags), "n_frames must be > 0", "no frames");
    if (sizeof(size_t) > 4)
        expect_msg(verify_tags_args_error(code, bits, (size_t)0x100000000ull, 64, tags), "n_frames too large", "2^32");
    expect_msg(verify_tags_args_error(code, bits, 1, 0, tags), "tag_bits must be in 1..64", "t = 0");
    expect_msg(verify_tags_args_error(code, bits, 1, 65, tags), "tag_bits must be in 1..64", "t = 65");
    expect_msg(verify_tags_args_error(code, bits, 1, 0xffffffffu, tags), "tag_bits must be in 1..64", "t = 2^32 - 1");

    expect_msg(reconcile_verify_args_error(64, tags, tags, ver), nullptr, "both");
    expect_msg(reconcile_verify_args_error(13, nullptr, tags, nullptr), nullptr, "tags only");
    expect_msg(reconcile_verify_args_error(1, tags, nullptr, ver), nullptr, "verdict only");
    expect_msg(reconcile_verify_args_error(0, tags, tags, ver), "tag_bits must be in 1..64", "t = 0");
    expect_msg(reconcile_verify_args_error(65, tags, tags, ver), "tag_bits must be in 1..64", "t = 65");
    expect_msg(reconcile_verify_args_error(64, nullptr, nullptr, nullptr), "neither alice_tags nor tags_out given", "none");
    expect_msg(reconcile_verify_args_error(64, nullptr, nullptr, ver), "neither alice_tags nor tags_out given", "none 2");
    expect_msg(reconcile_verify_args_error(64, tags, tags, nullptr), "alice_tags given without verified", "no verified");
    expect_msg(reconcile_verify_args_error(64, tags, nullptr, nullptr), "alice_tags given without verified", "no verified 2");
    expect_msg(reconcile_verify_args_error(64, nullptr, tags, ver), "verified given without alice_tags", "no alice");

    printf("%d\n", bad);
    return bad ? 1 : 0;
}
