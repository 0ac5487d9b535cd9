// qkd_ntt.h — the modular arithmetic of the long-block privacy amplification
// (qkd_privacy_amplify_long_batch, privacy_ntt.hip), shared by the kernels,
// the host helpers qkd_privacy_long_* and a stand-alone host program
// (tests/native/ntt_mod_check.cpp). Plain C++ for the host (no HIP headers
// needed), __host__ __device__ under hipcc.
//
// The hash is qkd_privacy.h's: out_k = XOR over p with x_p = 1 of r[p + k].
// As an integer, c[k] = sum_p x_p r[p + k] has out_k = c[k] & 1 and
// 0 <= c[k] <= n_in. With x reversed cyclically, x'[(-p) mod T] = x_p, c is
// the cyclic convolution of x' and r at length T, a power of two at or above
// n_in + L - 1 (no index p + k reaches T, so nothing wraps), which a
// number-theoretic transform takes in O(T log T):
//   c = NTT^-1( NTT(x') . NTT(r) )     modulo P = 15 * 2^27 + 1 = 2013265921,
// a prime with primitive root 31, so that roots of unity of order 2^k exist
// for every k <= 27. n_in <= 2^27 < P: the canonical residue in [0, P) IS the
// integer c[k], and its parity is the output bit. (The parity of a lazily
// reduced or Montgomery-form value is not.)
//
// Products are Montgomery products with R = 2^32: mont_mul(a, b) = a b / R.
// Data stay plain residues in [0, P); every constant they meet (twiddles, the
// key string's transform with T^-1 folded in) is kept in Montgomery form
// (c R mod P), so that mont_mul(plain, form) is a plain, canonical residue.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qkd_privacy.h"

namespace qkdn {

constexpr uint32_t kP = 2013265921u;           // 15 * 2^27 + 1
constexpr uint32_t kRoot = 31u;                // generates the multiplicative group
constexpr uint32_t kMaxLog2 = 27;              // 2^27 divides P - 1
constexpr uint32_t kMinLog2 = 6;               // shortest transform: one packed output word
// n_in + out_bits - 1 at most this (QKD_PRIVACY_LONG_MAX_BITS of the ABI header)
constexpr uint32_t kLongMaxBits = 1u << kMaxLog2;

// -P^-1 mod 2^32 by Newton's iteration (x <- x (2 - P x) doubles the correct bits)
constexpr uint32_t neg_p_inv() {
    uint32_t x = 1;
    for (int i = 0; i < 6; ++i) x *= 2u - kP * x;
    return 0u - x;
}
constexpr uint32_t kNegPInv = neg_p_inv();
constexpr uint32_t kR1 = (uint32_t)((1ull << 32) % kP);                 // R mod P: 1 in Montgomery form
constexpr uint32_t kR2 = (uint32_t)(((uint64_t)kR1 * kR1) % kP);        // R^2 mod P
static_assert((uint32_t)(kP * (0u - kNegPInv)) == 1u, "P * P^-1 == 1 mod 2^32");

// a, b in [0, P) -> a + b, a - b mod P in [0, P) (2 P < 2^32: no overflow)
QKD_VHD uint32_t add(uint32_t a, uint32_t b) {
    const uint32_t s = a + b;
    return s >= kP ? s - kP : s;
}
QKD_VHD uint32_t sub(uint32_t a, uint32_t b) { return a >= b ? a - b : a + kP - b; }

// a b / R mod P in [0, P), a, b in [0, P): t + m P is a multiple of 2^32 below
// 2^62 + 2^63, and its high word is below 2 P
QKD_VHD uint32_t mont_mul(uint32_t a, uint32_t b) {
    const uint64_t t = (uint64_t)a * b;
    const uint32_t m = (uint32_t)t * kNegPInv;
    const uint32_t u = (uint32_t)((t + (uint64_t)m * kP) >> 32);
    return u >= kP ? u - kP : u;
}
QKD_VHD uint32_t to_mont(uint32_t a) { return mont_mul(a, kR2); }
QKD_VHD uint32_t from_mont(uint32_t a) { return mont_mul(a, 1u); }
// a b mod P, plain in and out
QKD_VHD uint32_t mul(uint32_t a, uint32_t b) { return mont_mul(mont_mul(a, b), kR2); }
// base^e with base and the result in Montgomery form
QKD_VHD uint32_t mont_pow(uint32_t base, uint32_t e) {
    uint32_t r = kR1;
    while (e) {
        if (e & 1u) r = mont_mul(r, base);
        base = mont_mul(base, base);
        e >>= 1;
    }
    return r;
}
// the root of unity of order 2^k, 0 <= k <= 27 (plain): 31^((P - 1) / 2^k)
QKD_VHD uint32_t root_of_order_log2(uint32_t k) {
    return from_mont(mont_pow(to_mont(kRoot), (kP - 1u) >> k));
}
// (2^k)^-1 mod P (plain): 2^k * ((P - 1) / 2^k) = -1
QKD_VHD uint32_t inverse_of_length_log2(uint32_t k) { return kP - ((kP - 1u) >> k); }

// Wp of the long form: the words of the key string, 0 for arguments outside
// 1 <= out_bits <= n_in, n_in + out_bits - 1 <= kLongMaxBits
QKD_VHD size_t long_key_words(uint32_t n_in, uint32_t out_bits) {
    if (out_bits < 1 || out_bits > n_in || (uint64_t)n_in + out_bits - 1u > kLongMaxBits) return 0;
    return ((size_t)n_in + out_bits - 1u + 63u) >> 6;
}

// log2 of the transform length T: the power of two at or above
// n_in + out_bits - 1, and at least 2^kMinLog2 = 64 points, so that a length
// is a whole number of packed output words and of the kernels' 4-point
// vector accesses. For sizes long_key_words accepts.
QKD_VHD uint32_t transform_log2(uint32_t n_in, uint32_t out_bits) {
    const uint64_t need = (uint64_t)n_in + out_bits - 1u;
    uint32_t k = kMinLog2;
    while (((uint64_t)1 << k) < need) ++k;
    return k;
}

// The twiddle table of a length 2^k: a power w^e, e < 2^k, of the root of
// order 2^k is the product of entry e >> q of its high half (w^(i 2^q),
// 2^(k - q) entries) and entry e & (2^q - 1) of its low half (w^i, 2^q
// entries), q = table_split_log2(k): about 2 sqrt(T) entries in all.
QKD_VHD uint32_t table_split_log2(uint32_t k) { return (k + 1u) >> 1; }

// The scratch of qkd_privacy_amplify_long_batch in bytes: the block's T
// residues, the key string's transform (T residues), the twiddle table, and
// 16 bytes to align a base of any alignment. 0 for sizes outside the range.
inline size_t long_scratch_bytes(uint32_t n_in, uint32_t out_bits) {
    if (long_key_words(n_in, out_bits) == 0) return 0;
    const uint32_t k = transform_log2(n_in, out_bits), q = table_split_log2(k);
    return 4u * (((size_t)2 << k) + ((size_t)1 << q) + ((size_t)1 << (k - q))) + 16u;
}

// In-place transform of length 2^k, decimation in frequency: natural order
// in, bit-reversed order out; w = the root of order 2^k (plain).
inline void ntt_dif_ref(uint32_t* d, uint32_t k, uint32_t w) {
    for (uint32_t t = k; t-- > 0;) {
        const uint32_t h = 1u << t;
        const uint32_t step = mont_pow(to_mont(w), 1u << (k - 1u - t));      // the root of order 2 h
        for (uint32_t base = 0; base < (1u << k); base += 2u * h) {
            uint32_t tw = kR1;
            for (uint32_t j = 0; j < h; ++j) {
                const uint32_t a = d[base + j], b = d[base + j + h];
                d[base + j] = add(a, b);
                d[base + j + h] = mont_mul(sub(a, b), tw);
                tw = mont_mul(tw, step);
            }
        }
    }
}

// ... and its mirror, decimation in time: bit-reversed order in, natural
// order out; w = the INVERSE root of order 2^k. Undoes ntt_dif_ref up to the
// factor 2^k.
inline void ntt_dit_ref(uint32_t* d, uint32_t k, uint32_t w) {
    for (uint32_t t = 0; t < k; ++t) {
        const uint32_t h = 1u << t;
        const uint32_t step = mont_pow(to_mont(w), 1u << (k - 1u - t));
        for (uint32_t base = 0; base < (1u << k); base += 2u * h) {
            uint32_t tw = kR1;
            for (uint32_t j = 0; j < h; ++j) {
                const uint32_t a = d[base + j], b = mont_mul(d[base + j + h], tw);
                d[base + j] = add(a, b);
                d[base + j + h] = sub(a, b);
                tw = mont_mul(tw, step);
            }
        }
    }
}

// Scalar reference, the way the transform kernels take the hash. R:
// long_key_words(n_in, out_bits) words; out: privacy_out_words(out_bits);
// work: 2 * 2^transform_log2(n_in, out_bits) words of scratch.
inline void privacy_hash_ntt_ref(const uint64_t* R, const uint8_t* x, uint32_t n_in, uint32_t out_bits, uint64_t* out,
                                 uint32_t* work) {
    const uint32_t k = transform_log2(n_in, out_bits), T = 1u << k;
    const uint32_t wp = (uint32_t)long_key_words(n_in, out_bits);
    uint32_t* xs = work;
    uint32_t* rs = work + T;
    for (uint32_t i = 0; i < T; ++i) {
        const uint32_t p = (T - i) & (T - 1u);               // x reversed cyclically
        xs[i] = p < n_in ? (uint32_t)(x[p] & 1) : 0u;
        rs[i] = (uint32_t)((qkdv::privacy_key_word(0, R, wp, i >> 6) >> (i & 63u)) & 1u);
    }
    const uint32_t w = root_of_order_log2(k);
    const uint32_t w_inv = from_mont(mont_pow(to_mont(w), T - 1u));
    ntt_dif_ref(xs, k, w);
    ntt_dif_ref(rs, k, w);
    // the key string's transform takes T^-1 and goes to Montgomery form
    const uint32_t scale = mont_mul(to_mont(inverse_of_length_log2(k)), kR2);
    for (uint32_t i = 0; i < T; ++i) xs[i] = mont_mul(xs[i], mont_mul(rs[i], scale));
    ntt_dit_ref(xs, k, w_inv);
    const uint32_t wo = (uint32_t)qkdv::privacy_out_words(out_bits);
    for (uint32_t o = 0; o < wo; ++o) out[o] = 0;
    for (uint32_t i = 0; i < out_bits; ++i) out[i >> 6] |= (uint64_t)(xs[i] & 1u) << (i & 63u);
}

}  // namespace qkdn
