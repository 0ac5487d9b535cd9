// qkd_verify.h — the key verification hash of qkd_verify_tags_batch and
// qkd_reconcile_verify_batch, shared by the kernels, the host helper
// qkd_verify_expand_key and a stand-alone host program
// (tests/native/verify_hash_check.cpp). Plain C++ for the host (no HIP
// headers needed), __host__ __device__ under hipcc.
//
// The hash is a Hankel (Toeplitz-family) matrix over GF(2) given by a key
// string R of verify_key_words(N) 64-bit words, bit k of the string being
// r[k] = (R[k >> 6] >> (k & 63)) & 1 for 0 <= k <= N + 62:
//   window  W(p), 0 <= p < N: the 64-bit word whose bit i is r[p + i]
//   tag(x) = XOR of W(p) over the positions p with x_p = 1, low tag_bits bits
// so tag bit i = XOR_p r[p + i] x_p, a t-bit tag is the low t bits of the
// 64-bit one, and the all-zero key has tag 0. Positions are the caller's
// original bit positions; a key bit is byte & 1.
//
// With R truly random (the caller's hash_words) the family is 2^-t universal:
// two different keys get the same t-bit tag with probability 2^-t over R.
// The seeded form (hash_words == NULL: R expanded from a 64-bit hash_seed by
// SplitMix64 in counter form) is a computational stand-in, NOT an
// information-theoretic one: R then has at most 64 bits of entropy, and the
// collision bound holds only against keys chosen without knowledge of the
// seed. Either way a tag discloses tag_bits bits of the key, which the
// caller's privacy amplification has to account for.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QKD_VHD __host__ __device__ __forceinline__
#else
#define QKD_VHD inline
#endif

namespace qkdv {

// W: the words of the key string of an N-bit key, ceil((N + 63) / 64)
QKD_VHD size_t verify_key_words(int32_t n_bits) { return n_bits > 0 ? ((size_t)n_bits + 126u) >> 6 : 0; }

// Word k of the seeded key string: SplitMix64 in counter form, so that every
// lane computes its own words. R[k] = mix(seed + (k + 1) * golden), mod 2^64.
QKD_VHD uint64_t verify_key_word(uint64_t seed, uint64_t k) {
    uint64_t z = seed + (k + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// W(p) from the two adjacent words lo = R[p >> 6], hi = R[(p >> 6) + 1] and
// s = p & 63. No branch: at s = 0 the two-step shift drops hi entirely, so hi
// may then be any value (the word past the string's end is never needed).
QKD_VHD uint64_t verify_window(uint64_t lo, uint64_t hi, uint32_t s) {
    return (lo >> s) | ((hi << 1) << (63u - s));
}

// The low tag_bits bits (1 <= tag_bits <= 64) set.
QKD_VHD uint64_t verify_tag_mask(uint32_t tag_bits) { return ~0ull >> (64u - tag_bits); }

// (hi:lo) >> sh, low 32 bits, 0 <= sh <= 31: one v_alignbit_b32 on the device.
QKD_VHD uint32_t verify_funnel(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, sh);      // (a variable sh would otherwise become a 64-bit shift)
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
#endif
}

// The kernels' inner step: XOR over j < CNT of W(p + j) & -(bit j), for CNT
// (1, 4 or 8) consecutive positions from p, p % CNT == 0; byte j of b holds
// position p + j's key bit in its bit 0. In 32-bit operations only (a 64-bit
// shift by a variable issues at a quarter of their rate on the device): the
// CNT windows lie in bits s .. s + CNT + 62 of three adjacent 32-bit words,
// s = p & 31 <= 32 - CNT, so one funnel shift by s aligns all of them and
// each window is two funnel shifts by a constant.
// r32: the key string as 32-bit words (low half of R[k] first, the layout of
// a little-endian uint64_t array), followed by one 64-bit word of padding:
// r32[(p >> 5) + 2] is read at every p < N, also where no window needs it.
template <int CNT>
QKD_VHD uint64_t verify_xor_run(const uint32_t* r32, uint32_t p, uint64_t b) {
    const uint32_t a = p >> 5, s = p & 31u;
    const uint32_t w0 = r32[a], w1 = r32[a + 1], w2 = r32[a + 2];
    const uint32_t v0 = verify_funnel(w1, w0, s), v1 = verify_funnel(w2, w1, s), v2 = w2 >> s;
    uint32_t lo = 0, hi = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < CNT; ++j) {
        const uint32_t m = 0u - ((uint32_t)(b >> (8 * j)) & 1u);
        lo ^= (j ? verify_funnel(v1, v0, (uint32_t)j) : v0) & m;
        hi ^= (j ? verify_funnel(v2, v1, (uint32_t)j) : v1) & m;
    }
    return ((uint64_t)hi << 32) | lo;
}

}  // namespace qkdv
