// privacy_ntt.hip — long-block privacy amplification
// (qkd_privacy_amplify_long_batch): the Hankel hash of qkd_privacy.h taken as
// a cyclic convolution by number-theoretic transforms modulo
// P = 15 * 2^27 + 1 (qkd_ntt.h), O(T log T) for T >= n_in + out_bits - 1
// where the kernels of privacy.hip do n_in * out_bits work.
//
// One transform of length T = 2^k is a chain of passes over the T residues in
// scratch, each pass a set of independent transforms of 2^s points held in
// LDS, with k = s_0 + ... + s_n:
//   strided pass i  the 2^s_i points a stride of 2^a_i apart
//                   (a_i = k - s_0 - ... - s_i), 2^c_i neighbouring columns
//                   per workgroup so that every row of its tile is
//                   2^c_i contiguous residues; then the twiddle factor
//                   w_(2^(a + s))^(column * frequency) of the four-step form
//   block pass      the last s_n = min(k, S) bits: 2^s_n contiguous points
// with 2^S = 2^(s_i + c_i) the residues a workgroup holds (S = 13, 32 KB; the
// debug option QKD_PRIVACY_NTT_LOG2 lowers it to bring the many-pass paths
// down to a few hundred points). At S = 13 a length up to 2^13 is one pass,
// up to 2^20 two, up to 2^27 three. The forward transform is decimation in
// frequency (natural order in, digit-reversed out), the inverse its mirror,
// decimation in time, so no pass ever permutes: the pointwise product with
// the key string's transform happens in the digit-reversed order both share.
// The block pass of a key block fuses forward pass, product and inverse pass
// on the same 2^s_n points in LDS.
//
// Twiddles come from a table in scratch, written once per call: the powers
// w^e of the root of order T as a product of two entries of 2 sqrt(T) stored
// ones (qkdn::table_split_log2; 96 KB at T = 2^27, which stays in cache). A
// table costs two loads and one product per factor where exponentiation per
// workgroup would cost up to 27 squarings, and a full table of T entries
// would double the memory the transform moves. The key string's transform is
// computed once per call, with T^-1 folded in and in Montgomery form; the
// blocks of a call then run one after another through the same T residues.
//
// qkd_privacy_amplify_kept_batch hashes only the kept frames of a block of B
// frames, as if they stood compacted at its front with zeros behind them: one
// scan per call turns the frame flags into a list of the kept frames of each
// block (kept_scan_kernel), and the input stage reads position p of the
// compacted block from frame list[p / N] (ntt_gather_x_kernel, the division by
// a reciprocal from the host); every pass after the input stage is the long
// form's, skipped through its keep byte for a block that keeps nothing.
//
// Plain loads, LDS and vector stores, launches on the caller's stream only:
// no atomics, no allocation, no host copy, no synchronisation.
#include <algorithm>

#include "qkd_internal.h"
// (after the HIP runtime header, whose function attributes they use)
#include "qkd_args.h"
#include "qkd_ntt.h"
#include "qkd_privacy.h"

static_assert(qkdn::kLongMaxBits == QKD_PRIVACY_LONG_MAX_BITS, "the header's limit is the kernels'");

namespace qkd {
namespace {

using qkdn::add;
using qkdn::kP;
using qkdn::kR1;
using qkdn::mont_mul;
using qkdn::sub;

#ifndef QKD_NTT_BLOCK
#define QKD_NTT_BLOCK 512
#endif
constexpr uint32_t kNttBlock = QKD_NTT_BLOCK;   // lanes of a workgroup (a multiple of 64)
constexpr uint32_t kNttMaxLog2 = 13;         // S: residues of a workgroup in LDS (log2)
constexpr uint32_t kNttMinLog2 = 3;          // the debug option's lowest S
constexpr uint32_t kNttMaxCols = 6;          // at most 2^6 columns (256 contiguous bytes a row)
constexpr uint32_t kNttMaxPasses = 32;
constexpr uint32_t kKeptScanGrid = 1024;     // workgroups of the kept-frames scan at most (each strides over blocks)

// The twiddle table (scratch): w^e = hi[e >> q] * lo[e & (2^q - 1)], Montgomery form.
struct NttTable {
    const uint32_t* lo;
    const uint32_t* hi;
    uint32_t q, k;           // k: log2 T
};

__device__ __forceinline__ uint32_t twiddle(const NttTable& t, uint32_t e) {
    return mont_mul(t.hi[e >> t.q], t.lo[e & ((1u << t.q) - 1u)]);
}

// lo[i] = w^i, i < 2^q; hi[i] = w^(i 2^q), i < 2^(k - q); w_form: the root of order 2^k
__global__ __launch_bounds__(kNttBlock) void ntt_table_kernel(uint32_t* lo, uint32_t* hi, uint32_t q, uint32_t k,
                                                             uint32_t w_form) {
    const uint32_t i = blockIdx.x * kNttBlock + threadIdx.x;
    if (i < (1u << q)) lo[i] = qkdn::mont_pow(w_form, i);
    if (i < (1u << (k - q))) hi[i] = qkdn::mont_pow(w_form, i << q);
}

// d[i] = bit i of the key string, i < T (zero past the string's last word), four to a lane
__global__ __launch_bounds__(kNttBlock) void ntt_unpack_key_kernel(uint32_t* d, uint32_t T, uint64_t seed,
                                                                  const uint64_t* words, uint32_t key_words) {
    const uint32_t g = blockIdx.x * kNttBlock + threadIdx.x;
    if (g >= T / 4u) return;
    const uint32_t i = 4u * g;
    const uint32_t v = (uint32_t)(qkdv::privacy_key_word(seed, words, key_words, i >> 6) >> (i & 63u));
    reinterpret_cast<uint4*>(d)[g] = make_uint4(v & 1u, (v >> 1) & 1u, (v >> 2) & 1u, (v >> 3) & 1u);
}

// d[(T - p) mod T] = x[p] & 1, zero where p >= n_in: x reversed cyclically, four to a lane
__global__ __launch_bounds__(kNttBlock) void ntt_unpack_x_kernel(uint32_t* d, uint32_t T, const uint8_t* x,
                                                                uint32_t n_in, const uint8_t* keep) {
    if (keep && !*keep) return;
    const uint32_t g = blockIdx.x * kNttBlock + threadIdx.x;
    if (g >= T / 4u) return;
    uint32_t v[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t p = (T - (4u * g + j)) & (T - 1u);
        v[j] = p < n_in ? (uint32_t)(x[p] & 1) : 0u;
    }
    reinterpret_cast<uint4*>(d)[g] = make_uint4(v[0], v[1], v[2], v[3]);
}

// The scan of qkd_privacy_amplify_kept_batch, one workgroup per block (a
// workgroup takes the blocks blockIdx.x, blockIdx.x + gridDim.x, ...):
// list[b B + rank] = the index in block b of its kept frame of that rank, in
// ascending order (an exclusive prefix sum of keep != 0: a ballot and popcounts
// inside a wave, the waves' counts through LDS, a running carry over the chunks
// of kNttBlock frames), qkdn::kKeptNone for the ranks from the count up to B;
// kept[b] (may be NULL) = the count, nonempty[b] = whether it is nonzero.
__global__ __launch_bounds__(kNttBlock) void kept_scan_kernel(const uint8_t* keep, uint32_t n_blocks, uint32_t B,
                                                             uint32_t* list, uint32_t* kept, uint8_t* nonempty) {
    constexpr uint32_t kWaves = kNttBlock / 64u;
    __shared__ uint32_t wave_count[kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (size_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {       // (64 bits: b + gridDim.x may pass 2^32)
        const size_t row = b * B;
        uint32_t carry = 0;                                        // kept frames of the chunks before (uniform)
        for (uint32_t f0 = 0; f0 < B; f0 += kNttBlock) {
            const uint32_t f = f0 + threadIdx.x;                   // (f0 < B <= 2^27: no wrap)
            const bool on = f < B && keep[row + f] != 0;
            const uint64_t m = __ballot(on);
            if (lane == 0) wave_count[wave] = (uint32_t)__popcll(m);
            __syncthreads();
            uint32_t before = 0, total = 0;
            for (uint32_t w = 0; w < kWaves; ++w) {
                const uint32_t c = wave_count[w];
                before += w < wave ? c : 0u;
                total += c;
            }
            if (on) list[row + carry + before + (uint32_t)__popcll(m & (((uint64_t)1 << lane) - 1u))] = f;
            carry += total;
            __syncthreads();                                       // (wave_count is rewritten by the next chunk)
        }
        for (uint32_t r = carry + threadIdx.x; r < B; r += kNttBlock) list[row + r] = qkdn::kKeptNone;
        if (threadIdx.x == 0) {
            if (kept) kept[b] = carry;
            nonempty[b] = carry ? 1 : 0;
        }
    }
}

// The input stage of qkd_privacy_amplify_kept_batch, ntt_unpack_x_kernel's
// counterpart: d[(T - p) mod T] = bit p of the block's kept frames set end to
// end, zero behind them, four residues to a lane. frames and list: the
// block's; n = frame_bits, recip = qkdn::kept_reciprocal(n). Position p lies in
// slot p / n, which holds frame list[slot] when that is a frame; a slot at or
// past B (p >= B n) is past the block. Skipped, as every later pass, for a
// block that keeps no frame.
__global__ __launch_bounds__(kNttBlock) void ntt_gather_x_kernel(uint32_t* d, uint32_t T, const uint8_t* frames,
                                                                uint32_t n, uint32_t recip, uint32_t B,
                                                                const uint32_t* list, const uint8_t* nonempty) {
    if (!*nonempty) return;
    const uint32_t g = blockIdx.x * kNttBlock + threadIdx.x;
    if (g >= T / 4u) return;
    uint32_t slot[4], off[4], v[4];
    qkdn::kept_lane_positions(T, g, n, recip, slot, off);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t f = slot[j] < B ? list[slot[j]] : qkdn::kKeptNone;
        v[j] = f < B ? (uint32_t)(frames[f * n + off[j]] & 1) : 0u;                    // (f n + off < B n <= 2^27)
    }
    reinterpret_cast<uint4*>(d)[g] = make_uint4(v[0], v[1], v[2], v[3]);
}

// The workgroup's stage twiddles: tw[j] = w_(2^s)^j, j < 2^(s - 1). The inverse
// stages read the same table: w^-j = -w^(2^(s - 1) - j) for j > 0.
__device__ __forceinline__ void fill_stage_twiddles(uint32_t* tw, const NttTable& tab, uint32_t s) {
    for (uint32_t j = threadIdx.x; j < (1u << (s - 1u)); j += kNttBlock) tw[j] = twiddle(tab, j << (tab.k - s));
}

// Entry idx of the stage twiddles, or of their inverses
template <bool INV>
__device__ __forceinline__ uint32_t stage_twiddle(const uint32_t* tw, uint32_t half, uint32_t idx) {
    if (!INV) return tw[idx];
    return idx ? kP - tw[half - idx] : kR1;
}

// The stage t = s - 1 alone (points half the transform apart); starts with a barrier
template <bool INV>
__device__ __forceinline__ void lds_single_stage(uint32_t* buf, const uint32_t* tw, uint32_t s, uint32_t c) {
    const uint32_t half = 1u << (s - 1u), n_fly = half << c;
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < n_fly; e += kNttBlock) {       // (e: point j0 = e >> c < half, column e & cm)
        const uint32_t i0 = e, i1 = e + n_fly;
        const uint32_t w = stage_twiddle<INV>(tw, half, e >> c);
        if (INV) {
            const uint32_t a = buf[i0], b = mont_mul(buf[i1], w);
            buf[i0] = add(a, b);
            buf[i1] = sub(a, b);
        } else {
            const uint32_t a = buf[i0], b = buf[i1];
            buf[i0] = add(a, b);
            buf[i1] = mont_mul(sub(a, b), w);
        }
    }
}

// 2^c transforms of 2^s points side by side in LDS, point j of column col at
// buf[(j << c) | col]. Forward: decimation in frequency, frequency
// bit-reversed(j) left at point j. Inverse: the mirror, without the factor 2^-s.
// Starts and ends with a barrier. Stage t pairs the points 2^t apart; two
// stages t and t - 1 go between two barriers, a lane holding the four points
// j0 + {0, q, h, h + q} (h = 2^t, q = h / 2) that they connect, which halves
// the LDS traffic and the barriers (measured: 3.68 against 4.23 ms per block of
// 10^8 bits; 512 lanes a workgroup against 4.01 ms with 256 and 3.85 with 1024,
// profiles/privacy_long_block_ab.txt). With an odd s the stage t = s - 1 is
// left over: the first of the forward transform, the last of the inverse.
template <bool INV>
__device__ __forceinline__ void lds_transform(uint32_t* buf, const uint32_t* tw, uint32_t s, uint32_t c) {
    const uint32_t half = 1u << (s - 1u), n_quad = (half >> 1) << c, cm = (1u << c) - 1u;
    if (!INV && (s & 1u)) lds_single_stage<false>(buf, tw, s, c);
    for (uint32_t st = 0; st < s / 2u; ++st) {
        const uint32_t t = INV ? 2u * st + 1u : (s & ~1u) - 1u - 2u * st;          // the upper stage of the two
        const uint32_t h = 1u << t, q = h >> 1;
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < n_quad; e += kNttBlock) {
            const uint32_t col = e & cm, pr = e >> c;
            const uint32_t jl = pr & (q - 1u), j0 = ((pr >> (t - 1u)) << (t + 1u)) | jl;
            const uint32_t i0 = (j0 << c) | col, i1 = i0 + (q << c), i2 = i0 + (h << c), i3 = i2 + (q << c);
            const uint32_t idx = jl << (s - 1u - t);
            const uint32_t w_lo = stage_twiddle<INV>(tw, half, idx), w_hi = stage_twiddle<INV>(tw, half, idx + (half >> 1));
            const uint32_t w_q = stage_twiddle<INV>(tw, half, 2u * idx);            // stage t - 1, both pairs
            const uint32_t x0 = buf[i0], x1 = buf[i1], x2 = buf[i2], x3 = buf[i3];
            if (INV) {
                const uint32_t b1 = mont_mul(x1, w_q), b3 = mont_mul(x3, w_q);
                const uint32_t a0 = add(x0, b1), a1 = sub(x0, b1);
                const uint32_t a2 = mont_mul(add(x2, b3), w_lo), a3 = mont_mul(sub(x2, b3), w_hi);
                buf[i0] = add(a0, a2);
                buf[i1] = add(a1, a3);
                buf[i2] = sub(a0, a2);
                buf[i3] = sub(a1, a3);
            } else {
                const uint32_t a0 = add(x0, x2), a2 = mont_mul(sub(x0, x2), w_lo);
                const uint32_t a1 = add(x1, x3), a3 = mont_mul(sub(x1, x3), w_hi);
                buf[i0] = add(a0, a1);
                buf[i1] = mont_mul(sub(a0, a1), w_q);
                buf[i2] = add(a2, a3);
                buf[i3] = mont_mul(sub(a2, a3), w_q);
            }
        }
    }
    if (INV && (s & 1u)) lds_single_stage<true>(buf, tw, s, c);
    __syncthreads();
}

struct NttPass {
    uint32_t a, s, c;        // log2 of the stride, of the points, of the columns per workgroup
};

// One strided pass over d, in place: workgroup = (sub-problem of 2^(a + s)
// residues, group of 2^c columns). Forward: transform, then the factor
// w_(2^(a + s))^(column * frequency) = w_T^(column * frequency << (k - a - s));
// inverse: the inverse factor, then the inverse transform.
template <bool INV>
__global__ __launch_bounds__(kNttBlock) void ntt_strided_kernel(uint32_t* d, NttTable tab, NttPass ps,
                                                               const uint8_t* keep) {
    __shared__ uint32_t buf[1u << kNttMaxLog2];
    __shared__ uint32_t tw[1u << (kNttMaxLog2 - kNttMaxCols)];      // s <= S - min(S / 2, kNttMaxCols) <= 7
    if (keep && !*keep) return;
    const uint32_t a = ps.a, s = ps.s, c = ps.c, T = 1u << tab.k;
    const uint32_t groups = a - c;                                        // log2 of the column groups
    const uint32_t col0 = (blockIdx.x & ((1u << groups) - 1u)) << c;
    const uint32_t base = ((blockIdx.x >> groups) << (a + s)) + col0;
    const uint32_t n = 1u << (s + c), cm = (1u << c) - 1u, up = tab.k - a - s;
    fill_stage_twiddles(tw, tab, s);
    for (uint32_t e = threadIdx.x; e < n; e += kNttBlock) {
        const uint32_t j = e >> c, col = e & cm;
        uint32_t v = d[base + (j << a) + col];
        if (INV) {
            const uint32_t ex = ((col0 + col) * (__brev(j) >> (32u - s))) << up;
            if (ex) v = mont_mul(v, twiddle(tab, T - ex));
        }
        buf[e] = v;
    }
    lds_transform<INV>(buf, tw, s, c);
    for (uint32_t e = threadIdx.x; e < n; e += kNttBlock) {
        const uint32_t j = e >> c, col = e & cm;
        uint32_t v = buf[e];
        if (!INV) {
            const uint32_t ex = ((col0 + col) * (__brev(j) >> (32u - s))) << up;
            if (ex) v = mont_mul(v, twiddle(tab, ex));
        }
        d[base + (j << a) + col] = v;
    }
}

// The block pass over 2^s contiguous residues a workgroup, in place.
//   KEY   (the key string, once per call): forward, then * scale, which holds
//         T^-1 R^2, so that what is stored is (transform / T) in Montgomery form
//   !KEY  (a key block): forward, * the key string's stored transform, inverse
template <bool KEY>
__global__ __launch_bounds__(kNttBlock) void ntt_block_kernel(uint32_t* d, const uint32_t* h, NttTable tab, uint32_t s,
                                                             uint32_t scale, const uint8_t* keep) {
    __shared__ uint32_t buf[1u << kNttMaxLog2];
    __shared__ uint32_t tw[1u << (kNttMaxLog2 - 1u)];
    if (keep && !*keep) return;
    const uint32_t n = 1u << s, base = blockIdx.x << s;
    fill_stage_twiddles(tw, tab, s);
    for (uint32_t e = threadIdx.x; e < n; e += kNttBlock) buf[e] = d[base + e];
    lds_transform<false>(buf, tw, s, 0);
    if (KEY) {
        for (uint32_t e = threadIdx.x; e < n; e += kNttBlock) d[base + e] = mont_mul(buf[e], scale);
    } else {
        // (a lane multiplies the points it stored or will read itself only after lds_transform's barrier)
        for (uint32_t e = threadIdx.x; e < n; e += kNttBlock) buf[e] = mont_mul(buf[e], h[base + e]);
        lds_transform<true>(buf, tw, s, 0);
        for (uint32_t e = threadIdx.x; e < n; e += kNttBlock) d[base + e] = buf[e];
    }
}

// out[w] = the parities of the canonical residues d[64 w .. 64 w + 63], the
// bits at and above out_bits zero; all zero for a block that is not kept
__global__ __launch_bounds__(kNttBlock) void ntt_pack_kernel(const uint32_t* d, uint32_t out_bits, uint32_t wo,
                                                            uint64_t* out, const uint8_t* keep) {
    const uint32_t i = blockIdx.x * kNttBlock + threadIdx.x;
    if (i >= 64u * wo) return;                                   // (whole waves: 64 lanes a word)
    const bool kept = !keep || *keep;
    const uint64_t m = __ballot(kept && i < out_bits && (d[i] & 1u));
    if ((threadIdx.x & 63u) == 0) out[i >> 6] = m;
}

// The passes of a length 2^k with 2^S residues a workgroup: the strided ones
// first to last; returns their number and the block pass's s in *s_block
uint32_t plan_passes(uint32_t k, uint32_t S, NttPass* strided, uint32_t* s_block) {
    const uint32_t sb = std::min(k, S), rest = k - sb;
    *s_block = sb;
    if (!rest) return 0;
    const uint32_t s_max = S - std::min(S / 2u, kNttMaxCols);
    const uint32_t n = (rest + s_max - 1u) / s_max;
    uint32_t a = k;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = rest / n + (i < rest % n ? 1u : 0u);
        a -= s;
        strided[i] = NttPass{a, s, S - s};       // (a >= sb == S >= the columns' log2)
    }
    return n;
}

// What a call's launches share: where the arrays lie in the scratch, the
// passes of the transform and the launch shapes. For sizes the argument check
// accepted; S from the debug option.
struct LongCall {
    uint32_t n_in, out_bits, k, T, wo, key_words;
    uint32_t* x;             // the block's T residues
    uint32_t* h;             // the key string's transform
    uint32_t *lo, *hi;       // the twiddle table (tab reads it)
    uint32_t* end;           // one past the table: where an entry's own tables may start
    NttTable tab;
    NttPass strided[kNttMaxPasses];
    uint32_t n_strided, s_block;
    dim3 lanes, grid4, grid_strided, grid_block;
    hipStream_t st;
};

LongCall plan_call(void* scratch, uint32_t n_in, uint32_t out_bits, hipStream_t st) {
    uint32_t S = kNttMaxLog2;
    if (const DbgOpt cap = debug_option(nullptr, "QKD_PRIVACY_NTT_LOG2"))
        S = (uint32_t)std::min<long>(std::max<long>(cap.as_long(), kNttMinLog2), kNttMaxLog2);
    LongCall c;
    c.n_in = n_in;
    c.out_bits = out_bits;
    c.k = qkdn::transform_log2(n_in, out_bits);
    c.T = 1u << c.k;
    const uint32_t q = qkdn::table_split_log2(c.k);
    c.x = reinterpret_cast<uint32_t*>(((uintptr_t)scratch + 15u) & ~(uintptr_t)15u);
    c.h = c.x + c.T;
    c.lo = c.h + c.T;
    c.hi = c.lo + (1u << q);
    c.end = c.hi + (1u << (c.k - q));
    c.tab = NttTable{c.lo, c.hi, q, c.k};
    c.n_strided = plan_passes(c.k, S, c.strided, &c.s_block);
    c.lanes = dim3(kNttBlock);
    c.grid4 = dim3((c.T / 4u + kNttBlock - 1u) / kNttBlock);
    c.grid_strided = dim3(c.T >> std::min(c.k, S));
    c.grid_block = dim3(c.T >> c.s_block);
    c.key_words = (uint32_t)qkdn::long_key_words(n_in, out_bits);
    c.wo = (uint32_t)qkdv::privacy_out_words(out_bits);
    c.st = st;
    return c;
}

// once per call: the table and the key string's transform
qkd_status launch_key_string(const LongCall& c, uint64_t hash_seed, const uint64_t* hash_words) {
    const uint32_t w_form = qkdn::to_mont(qkdn::root_of_order_log2(c.k));
    const uint32_t scale = qkdn::mont_mul(qkdn::to_mont(qkdn::inverse_of_length_log2(c.k)), qkdn::kR2);
    hipLaunchKernelGGL(ntt_table_kernel, dim3(((1u << c.tab.q) + kNttBlock - 1u) / kNttBlock), c.lanes, 0, c.st,
                       c.lo, c.hi, c.tab.q, c.k, w_form);
    hipLaunchKernelGGL(ntt_unpack_key_kernel, c.grid4, c.lanes, 0, c.st, c.h, c.T, hash_seed, hash_words, c.key_words);
    for (uint32_t i = 0; i < c.n_strided; ++i)
        hipLaunchKernelGGL(ntt_strided_kernel<false>, c.grid_strided, c.lanes, 0, c.st, c.h, c.tab, c.strided[i],
                           (const uint8_t*)nullptr);
    hipLaunchKernelGGL(ntt_block_kernel<true>, c.grid_block, c.lanes, 0, c.st, c.h, (const uint32_t*)nullptr, c.tab,
                       c.s_block, scale, (const uint8_t*)nullptr);
    QKD_HIP(hipGetLastError());
    return QKD_OK;
}

// One block, after its input stage has filled c.x: forward passes, the product
// with the key string's transform inside the block pass, inverse passes, and
// the packed output. kb: the block's keep byte (NULL: kept).
qkd_status launch_block_passes(const LongCall& c, const uint8_t* kb, uint64_t* out) {
    for (uint32_t i = 0; i < c.n_strided; ++i)
        hipLaunchKernelGGL(ntt_strided_kernel<false>, c.grid_strided, c.lanes, 0, c.st, c.x, c.tab, c.strided[i], kb);
    hipLaunchKernelGGL(ntt_block_kernel<false>, c.grid_block, c.lanes, 0, c.st, c.x, (const uint32_t*)c.h, c.tab,
                       c.s_block, 0u, kb);
    for (uint32_t i = c.n_strided; i-- > 0;)
        hipLaunchKernelGGL(ntt_strided_kernel<true>, c.grid_strided, c.lanes, 0, c.st, c.x, c.tab, c.strided[i], kb);
    hipLaunchKernelGGL(ntt_pack_kernel, dim3((64u * c.wo + kNttBlock - 1u) / kNttBlock), c.lanes, 0, c.st,
                       (const uint32_t*)c.x, c.out_bits, c.wo, out, kb);
    QKD_HIP(hipGetLastError());
    return QKD_OK;
}

// The device of a call, checked as every entry checks it
qkd_status check_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return set_error(QKD_ERR_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev)
        return set_error(QKD_ERR_INVALID_ARG, "device %d out of range (%d devices)", device, ndev);
    return QKD_OK;
}

}  // namespace
}  // namespace qkd

using namespace qkd;

extern "C" {

size_t qkd_privacy_long_scratch_bytes(uint32_t n_in, uint32_t out_bits) {
    return qkdn::long_scratch_bytes(n_in, out_bits);
}

qkd_status qkd_privacy_amplify_long_batch(int device, const uint8_t* keys, size_t n_blocks, uint32_t n_in,
                                          uint32_t out_bits, uint64_t hash_seed, const uint64_t* hash_words,
                                          const uint8_t* keep, uint64_t* out_words, void* scratch,
                                          size_t scratch_bytes, void* stream) {
    clear_error();
    if (const char* bad = qkda::privacy_amplify_long_args_error(keys, n_blocks, n_in, out_bits, out_words, scratch,
                                                                scratch_bytes))
        return set_error(QKD_ERR_INVALID_ARG, "%s", bad);
    if (const qkd_status s = check_device(device)) return s;
    DeviceGuard g(device);
    const LongCall c = plan_call(scratch, n_in, out_bits, (hipStream_t)stream);
    if (const qkd_status s = launch_key_string(c, hash_seed, hash_words)) return s;
    for (size_t b = 0; b < n_blocks; ++b) {
        const uint8_t* kb = keep ? keep + b : nullptr;
        hipLaunchKernelGGL(ntt_unpack_x_kernel, c.grid4, c.lanes, 0, c.st, c.x, c.T, keys + b * (size_t)n_in, n_in, kb);
        if (const qkd_status s = launch_block_passes(c, kb, out_words + b * (size_t)c.wo)) return s;
    }
    return QKD_OK;
}

size_t qkd_privacy_kept_scratch_bytes(uint32_t frame_bits, uint32_t frames_per_block, uint32_t out_bits,
                                      size_t n_blocks) {
    return qkdn::kept_scratch_bytes(frame_bits, frames_per_block, out_bits, n_blocks);
}

qkd_status qkd_privacy_amplify_kept_batch(int device, const uint8_t* frames, size_t n_blocks, uint32_t frame_bits,
                                          uint32_t frames_per_block, uint32_t out_bits, uint64_t hash_seed,
                                          const uint64_t* hash_words, const uint8_t* keep, uint64_t* out_words,
                                          uint32_t* kept, void* scratch, size_t scratch_bytes, void* stream) {
    clear_error();
    if (const char* bad = qkda::privacy_amplify_kept_args_error(frames, n_blocks, frame_bits, frames_per_block,
                                                                out_bits, keep, out_words, scratch, scratch_bytes))
        return set_error(QKD_ERR_INVALID_ARG, "%s", bad);
    if (const qkd_status s = check_device(device)) return s;
    DeviceGuard g(device);
    const uint32_t n_in = frame_bits * frames_per_block;                 // (checked: at most 2^27)
    const LongCall c = plan_call(scratch, n_in, out_bits, (hipStream_t)stream);
    // this entry's tables, behind the long form's: the frame list on a 16-byte boundary, then a byte per block
    uint32_t* list = reinterpret_cast<uint32_t*>(((uintptr_t)c.end + 15u) & ~(uintptr_t)15u);
    uint8_t* nonempty = reinterpret_cast<uint8_t*>(list + n_blocks * frames_per_block);
    hipLaunchKernelGGL(kept_scan_kernel, dim3((uint32_t)std::min<size_t>(n_blocks, kKeptScanGrid)), c.lanes, 0, c.st,
                       keep, (uint32_t)n_blocks, frames_per_block, list, kept, nonempty);
    if (const qkd_status s = launch_key_string(c, hash_seed, hash_words)) return s;
    const uint32_t recip = qkdn::kept_reciprocal(frame_bits);
    for (size_t b = 0; b < n_blocks; ++b) {
        hipLaunchKernelGGL(ntt_gather_x_kernel, c.grid4, c.lanes, 0, c.st, c.x, c.T, frames + b * (size_t)n_in,
                           frame_bits, recip, frames_per_block, (const uint32_t*)(list + b * (size_t)frames_per_block),
                           (const uint8_t*)(nonempty + b));
        if (const qkd_status s = launch_block_passes(c, nonempty + b, out_words + b * (size_t)c.wo)) return s;
    }
    return QKD_OK;
}

}  // extern "C"
