// Host build of the long-block privacy amplification's arithmetic (qkd_ntt.h)
// and of the argument check of its entry point (qkd_args.h): the constants;
// the product mod P against the unsigned __int128 product on 0, 1, P - 1,
// P - 2, 2^31 and a few thousand random pairs, sum and difference at the wrap;
// the root of order 2^k for every k in 1..27 (w^(2^(k - 1)) = P - 1); the word
// counts, transform lengths and scratch sizes; the scalar reference that takes
// the hash by transforms (privacy_hash_ntt_ref) against the one that takes it
// directly (privacy_hash_ref), with n_in + L - 1 exactly a power of two, one
// past one, and below the shortest transform; every branch of the argument
// checker. Prints the number of wrong answers ("0" when all hold). Built plain
// and under AddressSanitizer + UBSan by tests/test_privacy_long_abi.py; a
// stand-alone program, host code only. Every array has exactly the size the
// headers state, so a read or write past one would be caught by the sanitizer.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../qkd_ldpc_amd/csrc/qkd_args.h"
#include "../../qkd_ldpc_amd/csrc/qkd_ntt.h"
#include "../../qkd_ldpc_amd/csrc/qkd_privacy.h"

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

static uint32_t mul128(uint32_t a, uint32_t b) {
    return (uint32_t)(((unsigned __int128)a * b) % qkdn::kP);
}

int main() {
    using namespace qkdn;
    const uint32_t P = 2013265921u;
    expect(kP == P && kP == 15u * (1u << 27) + 1u && kRoot == 31u && kMaxLog2 == 27, "constants");
    expect(kLongMaxBits == (1u << 27) && kMinLog2 == 6, "limits");
    expect((uint32_t)(kP * (0u - kNegPInv)) == 1u, "P^-1 mod 2^32");
    expect(kR1 == (uint32_t)(((unsigned __int128)1 << 32) % P) && kR2 == (uint32_t)(((unsigned __int128)1 << 64) % P), "R, R^2");

    // products
    uint64_t lcg = 0x243F6A8885A308D3ull;
    auto next = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg >> 11; };
    {
        const uint32_t edge[] = {0u, 1u, P - 1u, P - 2u, 1u << 31, 2u, 31u, P / 2u, P / 2u + 1u};
        std::vector<uint32_t> v;
        for (uint32_t e : edge) v.push_back(e % P);          // (2^31 as its residue: operands are in [0, P))
        for (int i = 0; i < 80; ++i) v.push_back((uint32_t)(next() % P));
        for (uint32_t a : v)
            for (uint32_t b : v) {
                expect(mul(a, b) == mul128(a, b), "mul", a, b);
                expect(mont_mul(to_mont(a), b) == mul128(a, b), "form * plain is plain", a, b);
                expect(from_mont(mont_mul(to_mont(a), to_mont(b))) == mul128(a, b), "form * form is a form", a, b);
                expect(add(a, b) == (uint32_t)(((uint64_t)a + b) % P), "add", a, b);
                expect(sub(a, b) == (uint32_t)(((uint64_t)a + P - b) % P), "sub", a, b);
            }
        // 2^31 itself, unreduced: the product's bound (high word below 2 P) holds up to there
        for (uint32_t b : v) expect(mul(1u << 31, b) == mul128(1u << 31, b) && mul(b, 1u << 31) == mul128(b, 1u << 31), "mul by 2^31", b);
        expect(mul(1u << 31, 1u << 31) == mul128(1u << 31, 1u << 31), "2^31 squared");
        expect(add(P - 1u, P - 1u) == P - 2u && add(P - 1u, 1u) == 0u && sub(0u, 1u) == P - 1u && sub(0u, P - 1u) == 1u &&
                   sub(5u, 5u) == 0u, "add / sub at the wrap");
        expect(mul(P - 1u, P - 1u) == 1u && mul(P - 1u, 2u) == P - 2u && mul(0u, P - 1u) == 0u, "mul at the wrap");
        expect(to_mont(1u) == kR1 && from_mont(kR1) == 1u && from_mont(to_mont(P - 1u)) == P - 1u, "Montgomery form");
    }

    // roots of unity: order exactly 2^k, each the square of the next
    expect(root_of_order_log2(0) == 1u && root_of_order_log2(1) == P - 1u, "orders 1 and 2");
    for (uint32_t k = 1; k <= 27; ++k) {
        const uint32_t w = root_of_order_log2(k);
        expect(w > 0 && w < P, "a residue", k);
        expect(from_mont(mont_pow(to_mont(w), 1u << (k - 1))) == P - 1u, "w^(2^(k - 1)) == -1", k);
        expect(mul(w, w) == root_of_order_log2(k - 1), "w_k^2 == w_(k - 1)", k);
        const uint32_t ti = inverse_of_length_log2(k);
        expect(mul(ti, (1u << k) % P) == 1u, "(2^k)^-1", k);
    }
    // 31 generates the group: P - 1 = 2^27 * 3 * 5, so 31^((P - 1) / q) != 1 for q = 2, 3, 5
    for (uint32_t q : {2u, 3u, 5u}) expect(from_mont(mont_pow(to_mont(kRoot), (P - 1u) / q)) != 1u, "primitive root", q);

    // word counts, lengths, scratch
    const uint32_t big = 1u << 27, h26 = 1u << 26, m20 = 1u << 20;
    const uint32_t kw[][3] = {{1, 1, 1}, {m20 + 1, 1, 16385}, {h26 + 1, h26, 1u << 21}, {big, 1, 1u << 21}, {big, 2, 0},
                              {5, 6, 0}, {0, 1, 0}, {5, 0, 0}, {0xffffffffu, 1, 0}, {0xffffffffu, 0xffffffffu, 0},
                              {70, 70, 3}, {333, 65, 7}};
    for (const auto& c : kw) {
        expect(long_key_words(c[0], c[1]) == c[2], "long key words", c[0], c[1]);
        expect((long_scratch_bytes(c[0], c[1]) != 0) == (c[2] != 0), "scratch bytes", c[0], c[1]);
        if (qkdv::privacy_key_words(c[0], c[1]))
            expect(long_key_words(c[0], c[1]) == qkdv::privacy_key_words(c[0], c[1]), "the short form's words", c[0], c[1]);
    }
    const uint32_t tl[][3] = {{1, 1, 6}, {33, 32, 6}, {33, 33, 7}, {193, 64, 8}, {194, 64, 9}, {m20 + 1, 1, 21},
                              {h26 + 1, h26, 27}, {big, 1, 27}, {100000000u, 34000000u, 27}};
    for (const auto& c : tl) {
        expect(transform_log2(c[0], c[1]) == c[2], "transform length", c[0], c[1]);
        const uint32_t q = table_split_log2(c[2]);
        expect(q <= c[2] && q >= c[2] - q, "table split", c[2]);
        expect(long_scratch_bytes(c[0], c[1]) == 4u * (((size_t)2 << c[2]) + ((size_t)1 << q) + ((size_t)1 << (c[2] - q))) + 16u,
               "scratch layout", c[0], c[1]);
    }

    // a transform and its mirror: 2^k times the identity
    for (uint32_t k : {1u, 2u, 6u, 9u}) {
        std::vector<uint32_t> d(1u << k), d0;
        for (auto& v : d) v = (uint32_t)(next() % P);
        d0 = d;
        const uint32_t w = root_of_order_log2(k);
        ntt_dif_ref(d.data(), k, w);
        ntt_dit_ref(d.data(), k, from_mont(mont_pow(to_mont(w), (1u << k) - 1u)));
        for (size_t i = 0; i < d.size(); ++i) expect(d[i] == mul(d0[i], (1u << k) % P), "dit(dif(d)) == 2^k d", k, (long)i);
    }

    // the hash by transforms against the hash taken directly
    const uint32_t shapes[][2] = {{1, 1}, {10, 7}, {70, 70}, {193, 64}, {194, 64}, {333, 65}, {1000, 25}};
    for (const auto& sh : shapes) {
        const uint32_t n = sh[0], L = sh[1];
        for (int form = 0; form < 2; ++form) {
            std::vector<uint64_t> R(long_key_words(n, L));
            expect(R.size() == qkdv::privacy_key_words(n, L), "words of the shape", n, L);
            for (size_t k = 0; k < R.size(); ++k) R[k] = form ? (next() << 32) ^ next() : qkdv::verify_key_word(12345, k);
            std::vector<uint32_t> work((size_t)2 << transform_log2(n, L));
            // keys: all zero, all one, a single bit at either end, random bytes 0..255
            for (int key = 0; key < 6; ++key) {
                std::vector<uint8_t> x(n, 0);
                if (key == 1) for (auto& b : x) b = 1;
                if (key == 2) x[0] = 1;
                if (key == 3) x[n - 1] = 0xff;
                if (key >= 4) for (auto& b : x) b = (uint8_t)next();
                std::vector<uint64_t> got(qkdv::privacy_out_words(L), ~0ull), want(got);
                privacy_hash_ntt_ref(R.data(), x.data(), n, L, got.data(), work.data());
                qkdv::privacy_hash_ref(R.data(), x.data(), n, L, want.data());
                expect(got == want, "hash by transforms != hash", n, key);
                if (L % 64) expect((got.back() >> (L % 64)) == 0, "bits at and above L", n, L);
            }
        }
    }

    // argument checks
    uint8_t keys[4] = {0, 1, 0, 1};
    uint64_t out[1] = {0};
    uint32_t scratch[1] = {0};
    using qkda::privacy_amplify_long_args_error;
    const size_t sb = long_scratch_bytes(4, 4), sbig = long_scratch_bytes(h26 + 1, h26);
    const char* range_n = "n_in must be in 1..QKD_PRIVACY_LONG_MAX_BITS";
    const char* range_l = "out_bits must be in 1..n_in";
    const char* range_t = "n_in + out_bits - 1 exceeds QKD_PRIVACY_LONG_MAX_BITS";
    const char* short_s = "scratch_bytes is below qkd_privacy_long_scratch_bytes(n_in, out_bits)";
    expect(sb == 4u * (128 + 8 + 8) + 16u && sbig > ((size_t)1 << 30), "scratch sizes");
    expect_msg(privacy_amplify_long_args_error(keys, 1, 4, 4, out, scratch, sb), nullptr, "valid");
    expect_msg(privacy_amplify_long_args_error(keys, 4, 1, 1, out, scratch, sb + 100), nullptr, "one bit");
    expect_msg(privacy_amplify_long_args_error(keys, 1, h26 + 1, h26, out, scratch, sbig), nullptr, "the limit");
    expect_msg(privacy_amplify_long_args_error(keys, 1, big, 1, out, scratch, sbig), nullptr, "n_in at the limit");
    expect_msg(privacy_amplify_long_args_error(nullptr, 1, 4, 4, out, scratch, sb), "null argument", "keys");
    expect_msg(privacy_amplify_long_args_error(keys, 1, 4, 4, nullptr, scratch, sb), "null argument", "out");
    expect_msg(privacy_amplify_long_args_error(keys, 1, 4, 4, out, nullptr, sb), "null argument", "scratch");
    expect_msg(privacy_amplify_long_args_error(nullptr, 0, 0, 0, out, scratch, 0), "null argument", "order");
    expect_msg(privacy_amplify_long_args_error(keys, 0, 4, 4, out, scratch, sb), "n_blocks must be > 0", "no blocks");
    if (sizeof(size_t) > 4)
        expect_msg(privacy_amplify_long_args_error(keys, (size_t)0x100000000ull, 4, 4, out, scratch, sb), "n_blocks too large", "2^32");
    expect_msg(privacy_amplify_long_args_error(keys, 1, 0, 1, out, scratch, sb), range_n, "n_in = 0");
    expect_msg(privacy_amplify_long_args_error(keys, 1, big + 1, 1, out, scratch, sbig), range_n, "n_in past the limit");
    expect_msg(privacy_amplify_long_args_error(keys, 1, 0xffffffffu, 1, out, scratch, sbig), range_n, "n_in = 2^32 - 1");
    expect_msg(privacy_amplify_long_args_error(keys, 1, 4, 0, out, scratch, sb), range_l, "L = 0");
    expect_msg(privacy_amplify_long_args_error(keys, 1, 4, 5, out, scratch, sb), range_l, "L = n_in + 1");
    expect_msg(privacy_amplify_long_args_error(keys, 1, 4, 0xffffffffu, out, scratch, sb), range_l, "L = 2^32 - 1");
    expect_msg(privacy_amplify_long_args_error(keys, 1, big, 2, out, scratch, sbig), range_t, "one past the limit");
    expect_msg(privacy_amplify_long_args_error(keys, 1, h26 + 1, h26 + 1, out, scratch, sbig), range_t, "2^27 + 1");
    expect_msg(privacy_amplify_long_args_error(keys, 1, 4, 4, out, scratch, sb - 1), short_s, "one byte short");
    expect_msg(privacy_amplify_long_args_error(keys, 1, 4, 4, out, scratch, 0), short_s, "no scratch bytes");
    expect_msg(privacy_amplify_long_args_error(keys, 1, h26 + 1, h26, out, scratch, sb), short_s, "a small shape's scratch");

    printf("%d\n", bad);
    return bad ? 1 : 0;
}
