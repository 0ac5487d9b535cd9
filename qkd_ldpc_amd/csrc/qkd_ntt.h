// qkd_ntt.h — the modular arithmetic of the long-block privacy amplification
// (qkd_privacy_amplify_long_batch, privacy_ntt.hip), shared by the kernels,
// the host helpers qkd_privacy_long_* and a stand-alone host program
// (tests/native/ntt_mod_check.cpp), and the index arithmetic of its
// kept-frames form (qkd_privacy_amplify_kept_batch;
// tests/native/privacy_kept_check.cpp). Plain C++ for the host (no HIP headers
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

// ---- the kept-frames form (qkd_privacy_amplify_kept_batch) ---------------------
// A block is B frames of N bits; the kept ones, in ascending order, are hashed
// as if they stood at the front of the block with zeros behind them. A scan
// writes list[rank] = the index in the block of the kept frame of that rank,
// and kKeptNone for the ranks from the kept count up to B; the input stage then
// reads position p of the compacted block from frame list[p / N] at bit p % N.

constexpr uint32_t kKeptNone = 0xffffffffu;    // list entry of a rank no kept frame has

// The scratch of qkd_privacy_amplify_kept_batch in bytes: the long form's for a
// block of B N bits, the frame list (n_blocks B 32-bit entries), one byte per
// block (nonzero when the block keeps a frame), and 16 bytes to start the list
// on a 16-byte boundary. 0 for sizes outside the range: B N in 64 bits not a
// long-form n_in for out_bits, no block, or n_blocks B at or above 2^32.
inline size_t kept_scratch_bytes(uint32_t frame_bits, uint32_t frames_per_block, uint32_t out_bits, size_t n_blocks) {
    const uint64_t n_in = (uint64_t)frame_bits * frames_per_block;
    if (n_in < 1 || n_in > kLongMaxBits) return 0;
    if (n_blocks < 1 || n_blocks > 0xffffffffull || (uint64_t)n_blocks * frames_per_block > 0xffffffffull) return 0;
    const size_t base = long_scratch_bytes((uint32_t)n_in, out_bits);
    if (base == 0) return 0;
    return base + 4u * (size_t)((uint64_t)n_blocks * frames_per_block) + n_blocks + 16u;
}

// floor(2^32 / n), n >= 1, held to 32 bits (2^32 - 1 for n = 1): the
// reciprocal kept_divmod multiplies by, computed once per call on the host
QKD_VHD uint32_t kept_reciprocal(uint32_t n) {
    const uint64_t m = ((uint64_t)1 << 32) / n;
    return m > 0xffffffffull ? 0xffffffffu : (uint32_t)m;
}

// *q = p / n, *r = p % n for any 32-bit p, by a multiply-high with
// recip = kept_reciprocal(n) and one correction: recip n = 2^32 - d with
// 0 <= d < n (d = 1 for n = 1), so p / n - p recip / 2^32 = p d / (n 2^32) < 1
// and the estimate is the quotient or one below it.
QKD_VHD void kept_divmod(uint32_t p, uint32_t n, uint32_t recip, uint32_t* q, uint32_t* r) {
    uint32_t qe = (uint32_t)(((uint64_t)p * recip) >> 32);
    uint32_t re = p - qe * n;
    if (re >= n) {
        ++qe;
        re -= n;
    }
    *q = qe;
    *r = re;
}

// The positions of the four residues a lane of the input stage owns, residue
// i = 4 g + j holding position p_j = (T - i) mod T (x reversed cyclically), as
// slot[j] = p_j / n and off[j] = p_j % n. T = 2^k >= 64, g < T / 4. One
// division, for p_1 = T - 4 g - 1 (never wraps: 3 <= p_1 < T); p_2 and p_3 lie
// one and two below it, p_0 one above it, or is 0 where g = 0, and a step of
// one position crosses at most one frame boundary.
QKD_VHD void kept_lane_positions(uint32_t T, uint32_t g, uint32_t n, uint32_t recip, uint32_t slot[4],
                                 uint32_t off[4]) {
    kept_divmod(T - 4u * g - 1u, n, recip, &slot[1], &off[1]);
    for (uint32_t j = 2; j < 4; ++j) {
        const bool wrap = off[j - 1u] == 0;
        slot[j] = slot[j - 1u] - (wrap ? 1u : 0u);
        off[j] = wrap ? n - 1u : off[j - 1u] - 1u;
    }
    if (g == 0) {
        slot[0] = 0;
        off[0] = 0;
    } else {
        const bool wrap = off[1] + 1u == n;
        slot[0] = slot[1] + (wrap ? 1u : 0u);
        off[0] = wrap ? 0u : off[1] + 1u;
    }
}

// Host restatement of the scan kernel: list[0 .. B) and the kept count of one
// block from its B flag bytes (a frame is kept when its byte is nonzero)
inline uint32_t kept_scan_ref(const uint8_t* keep, uint32_t frames_per_block, uint32_t* list) {
    uint32_t kept = 0;
    for (uint32_t f = 0; f < frames_per_block; ++f)
        if (keep[f]) list[kept++] = f;
    for (uint32_t r = kept; r < frames_per_block; ++r) list[r] = kKeptNone;
    return kept;
}

// Host restatement of the gathering input stage: the T residues of one block,
// d[i] = the bit at position (T - i) mod T of the compacted block, through the
// same index arithmetic as the kernel
inline void kept_gather_ref(uint32_t* d, uint32_t T, const uint8_t* frames, uint32_t frame_bits,
                            uint32_t frames_per_block, const uint32_t* list) {
    const uint32_t recip = kept_reciprocal(frame_bits);
    for (uint32_t g = 0; g < T / 4u; ++g) {
        uint32_t slot[4], off[4];
        kept_lane_positions(T, g, frame_bits, recip, slot, off);
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t f = slot[j] < frames_per_block ? list[slot[j]] : kKeptNone;
            d[4u * g + j] = f < frames_per_block ? (uint32_t)(frames[(size_t)f * frame_bits + off[j]] & 1) : 0u;
        }
    }
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
