// qkd_privacy.h — the privacy amplification hash of qkd_privacy_amplify_batch,
// shared by the kernels (privacy.hip), the host helpers qkd_privacy_key_words /
// qkd_privacy_expand_key and a stand-alone host program
// (tests/native/privacy_hash_check.cpp). Plain C++ for the host (no HIP
// headers needed), __host__ __device__ under hipcc.
//
// The hash is the Hankel (Toeplitz-family) matrix of qkd_verify.h with a long
// output: for an input of n_in bits x_p and an output of L bits,
//   out_i = XOR over the positions p with x_p = 1 of r[p + i],  0 <= i < L,
// r[k] = (R[k >> 6] >> (k & 63)) & 1 being bit k, 0 <= k <= n_in + L - 2, of a
// key string R of privacy_key_words(n_in, L) = ceil((n_in + L - 1) / 64) 64-bit
// words. The all-zero input hashes to all zeros; an input bit is byte & 1. The
// output is packed 64 bits a word, bit i in word i >> 6 at i & 63, the bits at
// and above L of the last word zero.
//
// With R truly random (the caller's hash_words) the family is universal, which
// is what the leftover hash lemma asks of privacy amplification. The seeded
// form (hash_words == NULL: R[k] = qkdv::verify_key_word(hash_seed, k),
// SplitMix64 in counter form) is a computational stand-in, NOT an
// information-theoretic one: R then has at most 64 bits of entropy.
//
// With n_in = N and L = 64 the one output word is qkd_verify.h's 64-bit tag
// under the same key string (privacy_key_words(N, 64) == verify_key_words(N)).
// A link must therefore NOT use its verification string for privacy
// amplification as well: the announced tag would be 64 bits of the secret key.
// The two strings (or seeds) have to be independent.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qkd_verify.h"

namespace qkdv {

// n_in and out_bits at most this (QKD_PRIVACY_MAX_BITS of the ABI header);
// longer blocks take the same hash by transforms (qkd_ntt.h, privacy_ntt.hip)
constexpr uint32_t kPrivacyMaxBits = 1u << 20;

// Wp: the words of the key string, 0 for arguments outside
// 1 <= out_bits <= n_in <= kPrivacyMaxBits
QKD_VHD size_t privacy_key_words(uint32_t n_in, uint32_t out_bits) {
    if (out_bits < 1 || out_bits > n_in || n_in > kPrivacyMaxBits) return 0;
    return ((size_t)n_in + out_bits - 1u + 63u) >> 6;
}

// Wo: the packed output words of one frame
QKD_VHD size_t privacy_out_words(uint32_t out_bits) { return ((size_t)out_bits + 63u) >> 6; }

// 64-bit word k of the key string: the caller's words or the seeded form, and
// zero past the string's end (the kernels stage whole stretches; what lies
// past bit n_in + L - 2 only ever meets positions or outputs that do not exist)
QKD_VHD uint64_t privacy_key_word(uint64_t seed, const uint64_t* words, uint32_t key_words, uint32_t k) {
    if (k >= key_words) return 0;
    return words ? words[k] : verify_key_word(seed, k);
}

// The same string as 32-bit words, low half of R[k] first
QKD_VHD uint32_t privacy_key_word32(uint64_t seed, const uint64_t* words, uint32_t key_words, uint32_t j) {
    return (uint32_t)(privacy_key_word(seed, words, key_words, j >> 1) >> (32u * (j & 1u)));
}

// The bits of 32-bit output word o (bits 32 o .. 32 o + 31) that lie below out_bits
QKD_VHD uint32_t privacy_word_mask32(uint32_t out_bits, uint32_t o) {
    const uint64_t lo = (uint64_t)o * 32u;
    if (lo >= out_bits) return 0u;
    const uint64_t left = out_bits - lo;
    return left >= 32u ? ~0u : (~0u >> (32u - (uint32_t)left));
}

// Scalar reference, the way the direct kernel takes the hash: per set input
// bit p, 32-bit output word o gets the funnel-shifted window r[p + 32 o ..].
// R: privacy_key_words(n_in, out_bits) words; out: privacy_out_words(out_bits).
inline void privacy_hash_ref(const uint64_t* R, const uint8_t* x, uint32_t n_in, uint32_t out_bits, uint64_t* out) {
    const uint32_t wp = (uint32_t)privacy_key_words(n_in, out_bits);
    const uint32_t wo = (uint32_t)privacy_out_words(out_bits);
    for (uint32_t w = 0; w < wo; ++w) out[w] = 0;
    for (uint32_t p = 0; p < n_in; ++p) {
        if (!(x[p] & 1)) continue;
        for (uint32_t o = 0; o < 2 * wo; ++o) {
            const uint32_t a = (p >> 5) + o;
            const uint32_t v = verify_funnel(privacy_key_word32(0, R, wp, a + 1), privacy_key_word32(0, R, wp, a), p & 31u);
            out[o >> 1] ^= (uint64_t)(v & privacy_word_mask32(out_bits, o)) << (32u * (o & 1u));
        }
    }
}

}  // namespace qkdv
