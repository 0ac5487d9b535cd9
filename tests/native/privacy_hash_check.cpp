// Host build of the privacy amplification hash (qkd_privacy.h) and of the
// argument check of its entry point (qkd_args.h): the word counts, the key
// string's accessors (64- and 32-bit words, zero past the end), the output
// masks and the scalar reference hash against an independent bit-by-bit loop
// out_i = XOR_p r[p + i] x_p at (n_in, L) = (1, 1), (70, 70), (333, 65), with
// a seeded and with an arbitrary key string; the identity with the
// verification hash (n_in = N, L = 64: the output word is the 64-bit tag of
// qkdv::verify_xor_run<1> under the same string); every branch of the
// argument checker. Prints the number of wrong answers ("0" when all hold).
// Built plain and under AddressSanitizer + UBSan by tests/test_privacy_abi.py;
// a stand-alone program, host code only. The key string is held in exactly Wp
// words, so a read past it would be caught by the sanitizer.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../qkd_ldpc_amd/csrc/qkd_args.h"
#include "../../qkd_ldpc_amd/csrc/qkd_privacy.h"
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

// the definition, bit by bit, with its own word count and its own packing
static std::vector<uint64_t> hash_bits(const std::vector<uint64_t>& R, const std::vector<uint8_t>& x, uint32_t L) {
    auto r = [&](size_t k) -> uint64_t { return (R.at(k / 64) >> (k % 64)) & 1u; };
    std::vector<uint64_t> out((L + 63) / 64, 0);
    for (uint32_t i = 0; i < L; ++i) {
        uint64_t b = 0;
        for (size_t p = 0; p < x.size(); ++p)
            if (x[p] & 1) b ^= r(p + i);
        out[i / 64] |= b << (i % 64);
    }
    return out;
}

int main() {
    using namespace qkdv;
    // Wp = ceil((n_in + L - 1) / 64), 0 outside 1 <= L <= n_in <= 2^20
    const uint32_t kw[][3] = {{1, 1, 1}, {64, 1, 1}, {64, 2, 2}, {10240, 64, 161}, {0, 1, 0}, {5, 6, 0},
                              {(1u << 20) + 1, 1, 0}, {1u << 20, 1u << 20, 32768}, {5, 0, 0}, {70, 70, 3}, {333, 65, 7}};
    for (const auto& c : kw) expect(privacy_key_words(c[0], c[1]) == c[2], "key words", c[0], c[1]);
    expect(kPrivacyMaxBits == (1u << 20), "limit");
    for (int32_t n : {64, 65, 66, 10240, 131072})
        expect(privacy_key_words((uint32_t)n, 64) == verify_key_words(n), "verify's word count at L = 64", n);
    expect(privacy_out_words(1) == 1 && privacy_out_words(64) == 1 && privacy_out_words(65) == 2 &&
               privacy_out_words(1u << 20) == 16384, "out words");
    // masks of the 32-bit output words
    expect(privacy_word_mask32(1, 0) == 1u && privacy_word_mask32(1, 1) == 0u, "mask L = 1");
    expect(privacy_word_mask32(32, 0) == ~0u && privacy_word_mask32(32, 1) == 0u, "mask L = 32");
    expect(privacy_word_mask32(65, 0) == ~0u && privacy_word_mask32(65, 1) == ~0u && privacy_word_mask32(65, 2) == 1u &&
               privacy_word_mask32(65, 3) == 0u, "mask L = 65");
    expect(privacy_word_mask32(1u << 20, 32767) == ~0u && privacy_word_mask32(1u << 20, 32768) == 0u, "mask L = 2^20");
    // the accessors: seeded words are SplitMix64's, the caller's are the caller's, zero past the end
    {
        const uint64_t W[2] = {0x0123456789abcdefull, 0xfedcba9876543210ull};
        expect(privacy_key_word(5, W, 2, 0) == W[0] && privacy_key_word(5, W, 2, 1) == W[1] && privacy_key_word(5, W, 2, 2) == 0,
               "caller's words");
        expect(privacy_key_word(0, nullptr, 3, 0) == 0xE220A8397B1DCDAFull && privacy_key_word(0, nullptr, 3, 2) == 0x06C45D188009454Full &&
                   privacy_key_word(0, nullptr, 3, 3) == 0, "seeded words");
        expect(privacy_key_word32(5, W, 2, 0) == 0x89abcdefu && privacy_key_word32(5, W, 2, 1) == 0x01234567u &&
                   privacy_key_word32(5, W, 2, 3) == 0xfedcba98u && privacy_key_word32(5, W, 2, 4) == 0u, "32-bit words");
    }

    uint64_t lcg = 0x243F6A8885A308D3ull;
    auto next = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg >> 11; };
    const uint32_t shapes[][2] = {{1, 1}, {70, 70}, {333, 65}, {64, 64}, {65, 33}, {128, 1}};
    for (const auto& sh : shapes) {
        const uint32_t n = sh[0], L = sh[1];
        for (int form = 0; form < 2; ++form) {
            std::vector<uint64_t> R(privacy_key_words(n, L));
            expect(R.size() == (n + L - 1 + 63) / 64, "words of the shape", n, L);
            for (size_t k = 0; k < R.size(); ++k) R[k] = form ? (next() << 32) ^ next() : verify_key_word(12345, k);
            // keys: all zero, all one, a single bit at either end, random bytes
            // with high bits set (only byte & 1 counts)
            for (int key = 0; key < 6; ++key) {
                std::vector<uint8_t> x(n, 0);
                if (key == 1) for (auto& b : x) b = 1;
                if (key == 2) x[0] = 1;
                if (key == 3) x[n - 1] = 0xff;
                if (key >= 4) for (auto& b : x) b = (uint8_t)next();
                std::vector<uint64_t> got(privacy_out_words(L), ~0ull);
                privacy_hash_ref(R.data(), x.data(), n, L, got.data());
                const std::vector<uint64_t> want = hash_bits(R, x, L);
                expect(got == want, "reference hash != definition", n, key);
                if (key == 0)
                    for (uint64_t w : got) expect(w == 0, "all-zero key", n, L);
                if (key == 2 && L >= 64) expect(got[0] == R[0], "bit 0 alone gives R[0]", n, L);
                if (L % 64) expect((got.back() >> (L % 64)) == 0, "bits at and above L", n, L);
            }
        }
    }

    // L = 64: the verification tag under the same string
    for (uint32_t n : {64u, 70u, 333u, 10240u}) {
        std::vector<uint64_t> R(privacy_key_words(n, 64));
        expect(R.size() == verify_key_words((int32_t)n), "same word count", n);
        for (size_t k = 0; k < R.size(); ++k) R[k] = verify_key_word(0xC0FFEE, k);
        std::vector<uint8_t> x(n);
        for (auto& b : x) b = (uint8_t)next();
        uint64_t out = ~0ull;
        privacy_hash_ref(R.data(), x.data(), n, 64, &out);
        std::vector<uint64_t> Rp(R);
        Rp.push_back(0);                       // verify_xor_run reads one word past the string
        std::vector<uint32_t> r32(2 * Rp.size());
        for (size_t k = 0; k < Rp.size(); ++k) {
            r32[2 * k] = (uint32_t)Rp[k];
            r32[2 * k + 1] = (uint32_t)(Rp[k] >> 32);
        }
        uint64_t tag = 0;
        for (uint32_t p = 0; p < n; ++p) tag ^= verify_xor_run<1>(r32.data(), p, x[p]);
        expect(out == tag, "L = 64 is the verification tag", n);
    }

    // argument checks
    uint8_t keys[4] = {0, 1, 0, 1};
    uint64_t out[1] = {0};
    using qkda::privacy_amplify_args_error;
    const uint32_t big = 1u << 20;
    expect_msg(privacy_amplify_args_error(keys, 1, 4, 4, out), nullptr, "valid");
    expect_msg(privacy_amplify_args_error(keys, 4, 1, 1, out), nullptr, "one bit");
    expect_msg(privacy_amplify_args_error(keys, 1, big, big, out), nullptr, "the limit");
    expect_msg(privacy_amplify_args_error(nullptr, 1, 4, 4, out), "null argument", "keys");
    expect_msg(privacy_amplify_args_error(keys, 1, 4, 4, nullptr), "null argument", "out");
    expect_msg(privacy_amplify_args_error(nullptr, 0, 0, 0, out), "null argument", "order");
    expect_msg(privacy_amplify_args_error(keys, 0, 4, 4, out), "n_frames must be > 0", "no frames");
    if (sizeof(size_t) > 4)
        expect_msg(privacy_amplify_args_error(keys, (size_t)0x100000000ull, 4, 4, out), "n_frames too large", "2^32");
    expect_msg(privacy_amplify_args_error(keys, 1, 0, 1, out), "n_in must be in 1..QKD_PRIVACY_MAX_BITS", "n_in = 0");
    expect_msg(privacy_amplify_args_error(keys, 1, big + 1, 1, out), "n_in must be in 1..QKD_PRIVACY_MAX_BITS", "n_in past the limit");
    expect_msg(privacy_amplify_args_error(keys, 1, 0xffffffffu, 1, out), "n_in must be in 1..QKD_PRIVACY_MAX_BITS", "n_in = 2^32 - 1");
    expect_msg(privacy_amplify_args_error(keys, 1, 4, 0, out), "out_bits must be in 1..n_in", "L = 0");
    expect_msg(privacy_amplify_args_error(keys, 1, 4, 5, out), "out_bits must be in 1..n_in", "L = n_in + 1");
    expect_msg(privacy_amplify_args_error(keys, 1, 4, 0xffffffffu, out), "out_bits must be in 1..n_in", "L = 2^32 - 1");

    printf("%d\n", bad);
    return bad ? 1 : 0;
}
