// frame_syn.hip — keys path, before the split decoder: per frame the target
// syndrome s_A = H * alice (calculate_syndrome_irregular, reference
// src/array_and_matrix_operations.cpp:476-486, on Alice's key,
// src/qkd_ldpc_algorithm.cpp:413-414) and the sign of each check's
// first-iteration product, and the keys rewritten in the split decoder's
// internal bit order. Three forms (gather, given target, bit-sliced over 16
// frames), chosen by launch_frame_syn. Built with the split decoder's
// scheduler strategy (Makefile), as when these kernels stood in decode_split.hip.
#include <hip/hip_runtime.h>

#include "qkd_decode.h"

namespace qkd {

// ---- keys path: the kernels around decode_split_kernel ---------------------
// frame_syn_kernel: per frame the target syndrome s_A = H * alice
// (calculate_syndrome_irregular, array_and_matrix_operations.cpp:476-486, on
// Alice's key, qkd_ldpc_algorithm.cpp:413-414) and the sign of each check's
// first-iteration product, q_j = s_j ^ (H * bob)_j ^ (deg_j & sign(log_p))
// (first_check_phase), one bit per check in whole 64-check groups. kSynFrames
// frames per workgroup share each load of a check's row.
#ifndef QKD_SYN_FRAMES
#define QKD_SYN_FRAMES 4
#endif
constexpr int kSynFrames = QKD_SYN_FRAMES;
constexpr int kSynBlock = 256;
constexpr int kSynRow = 8;
//
// It also rewrites the frames' two keys in place in the split decoder's
// internal bit order (DeviceCode::perm: internal bit q holds original bit
// perm[q]), from the copies it staged: the decoder then reads Bob's bits and
// compares Alice's word by word with no gathers of its own.
__global__ __launch_bounds__(kSynBlock) void frame_syn_kernel(DeviceCode c, uint64_t* alice_w, uint64_t* bob_w,
                                                              uint32_t words, uint32_t n_frames, uint32_t lsign,
                                                              uint32_t* synw, uint32_t* counter, uint32_t* win,
                                                              uint32_t win_words) {
    // [kSynFrames][2 * words] pairs (Alice's 32-bit word, Bob's 32-bit word):
    // one 8-byte LDS read gives both keys' bit
    extern __shared__ uint2 kw[];
    // the decoder's frame queue and replay count (launch.hip launch_prepared:
    // this kernel runs first on the stream, in place of a memset)
    if (blockIdx.x == 0 && threadIdx.x < 2) counter[threadIdx.x] = 0;
    for (uint32_t i = blockIdx.x * kSynBlock + threadIdx.x; i < win_words; i += gridDim.x * kSynBlock) win[i] = 0;
    const uint32_t w32 = 2 * words;
    const uint32_t f0 = blockIdx.x * kSynFrames;
    const uint32_t nf = min((uint32_t)kSynFrames, n_frames - f0);
    for (uint32_t q = threadIdx.x; q < nf * words; q += kSynBlock) {
        const uint32_t fr = q / words;
        const uint32_t w = q - fr * words;
        const uint64_t av = alice_w[(size_t)(f0 + fr) * words + w];
        const uint64_t bv = bob_w[(size_t)(f0 + fr) * words + w];
        kw[fr * w32 + 2 * w] = make_uint2((uint32_t)av, (uint32_t)bv);
        kw[fr * w32 + 2 * w + 1] = make_uint2((uint32_t)(av >> 32), (uint32_t)(bv >> 32));
    }
    __syncthreads();
    const int m_words = decode_m_words(c.m);
    const int lane = threadIdx.x & 63;
    for (int j0 = (int)(threadIdx.x & ~63u); j0 < c.m; j0 += kSynBlock) {
        const int j = j0 + lane;
        uint32_t pa[kSynFrames], pb[kSynFrames];
#pragma unroll
        for (int fr = 0; fr < kSynFrames; ++fr) pa[fr] = pb[fr] = 0;
        uint32_t deg = 0;
        auto take = [&](int bit) {
            if (bit < 0) return;
            deg++;
            const uint32_t wi = (uint32_t)bit >> 5, sh = (uint32_t)bit & 31u;
#pragma unroll
            for (int fr = 0; fr < kSynFrames; ++fr) {
                const uint2 v = kw[fr * w32 + wi];
                pa[fr] ^= v.x >> sh;
                pb[fr] ^= v.y >> sh;
            }
        };
        if (j < c.m) {
            // the row's first kSynRow entries loaded together (their latencies
            // overlap), the rest one by one
            int bits[kSynRow];
#pragma unroll
            for (int k = 0; k < kSynRow; ++k) bits[k] = k < c.max_dc ? c.chk_bits[k * c.m_pad + j] : -1;
#pragma unroll
            for (int k = 0; k < kSynRow; ++k) take(bits[k]);
            for (int k = kSynRow; k < c.max_dc; ++k) take(c.chk_bits[k * c.m_pad + j]);
        }
#pragma unroll
        for (int fr = 0; fr < kSynFrames; ++fr) {
            const uint64_t sm = __ballot(pa[fr] & 1u);
            const uint64_t qm = __ballot((pa[fr] ^ pb[fr] ^ (lsign & deg)) & 1u);
            if (lane == 0 && (uint32_t)fr < nf) {
                uint32_t* o = synw + (size_t)(f0 + fr) * 2 * m_words;
                o[j0 >> 5] = (uint32_t)sm;
                o[(j0 >> 5) + 1] = (uint32_t)(sm >> 32);
                o[m_words + (j0 >> 5)] = (uint32_t)qm;
                o[m_words + (j0 >> 5) + 1] = (uint32_t)(qm >> 32);
            }
        }
    }
    // the keys in the internal order: word w of a frame gathers bits
    // perm[64 w + lane] (one perm load serves the workgroup's frames). A wave
    // takes kSynPermBatch consecutive words at a time, issues their perm loads
    // first, and lane u keeps word u's ballots, so each key's words leave as
    // one coalesced store per frame.
    constexpr uint32_t kSynPermBatch = 8;
    constexpr uint32_t NWS = kSynBlock / 64;
    for (uint32_t w0 = (threadIdx.x >> 6) * kSynPermBatch; w0 < words; w0 += NWS * kSynPermBatch) {
        uint32_t ob[kSynPermBatch];
#pragma unroll
        for (uint32_t u = 0; u < kSynPermBatch; ++u) {
            const uint32_t q = (w0 + u) * 64 + (uint32_t)lane;
            ob[u] = q < (uint32_t)c.n ? (uint32_t)c.perm[q] : 0xffffffffu;
        }
#pragma unroll
        for (int fr = 0; fr < kSynFrames; ++fr) {
            uint64_t mya = 0, myb = 0;
#pragma unroll
            for (uint32_t u = 0; u < kSynPermBatch; ++u) {
                const bool in = ob[u] != 0xffffffffu;
                const uint32_t o = in ? ob[u] : 0u;
                const uint2 v = kw[fr * w32 + (o >> 5)];
                const uint64_t am = __ballot(in && ((v.x >> (o & 31u)) & 1u));
                const uint64_t bm = __ballot(in && ((v.y >> (o & 31u)) & 1u));
                if ((uint32_t)lane == u) {
                    mya = am;
                    myb = bm;
                }
            }
            const uint32_t w = w0 + (uint32_t)lane;
            if ((uint32_t)lane < kSynPermBatch && w < words && (uint32_t)fr < nf) {
                alice_w[(size_t)(f0 + fr) * words + w] = mya;
                bob_w[(size_t)(f0 + fr) * words + w] = myb;
            }
        }
    }
}

// frame_syn_kernel with the target syndrome given by the caller
// (qkd_reconcile_batch: syn_b[F x M] bytes, nonzero = 1; rows of any
// alignment): only Bob's words are staged ([kSynFrames][2 * words] 32-bit
// words), only (H * bob)_j is computed, and only bob_w is rewritten in the
// internal order. The queue and window resets, q_j and the layout of synw are
// frame_syn_kernel's.
__global__ __launch_bounds__(kSynBlock) void frame_syn_given_kernel(DeviceCode c, uint64_t* bob_w,
                                                                    const uint8_t* syn_b, uint32_t words,
                                                                    uint32_t n_frames, uint32_t lsign,
                                                                    uint32_t* synw, uint32_t* counter,
                                                                    uint32_t* win, uint32_t win_words) {
    extern __shared__ uint32_t kb[];
    if (blockIdx.x == 0 && threadIdx.x < 2) counter[threadIdx.x] = 0;
    for (uint32_t i = blockIdx.x * kSynBlock + threadIdx.x; i < win_words; i += gridDim.x * kSynBlock) win[i] = 0;
    const uint32_t w32 = 2 * words;
    const uint32_t f0 = blockIdx.x * kSynFrames;
    const uint32_t nf = min((uint32_t)kSynFrames, n_frames - f0);
    for (uint32_t q = threadIdx.x; q < (uint32_t)kSynFrames * words; q += kSynBlock) {
        const uint32_t fr = q / words;
        const uint32_t w = q - fr * words;
        const uint64_t bv = fr < nf ? bob_w[(size_t)(f0 + fr) * words + w] : 0ull;
        kb[fr * w32 + 2 * w] = (uint32_t)bv;
        kb[fr * w32 + 2 * w + 1] = (uint32_t)(bv >> 32);
    }
    __syncthreads();
    const int m_words = decode_m_words(c.m);
    const int lane = threadIdx.x & 63;
    for (int j0 = (int)(threadIdx.x & ~63u); j0 < c.m; j0 += kSynBlock) {
        const int j = j0 + lane;
        uint32_t pb[kSynFrames], sj[kSynFrames];
#pragma unroll
        for (int fr = 0; fr < kSynFrames; ++fr) pb[fr] = sj[fr] = 0;
        uint32_t deg = 0;
        if (j < c.m) {
#pragma unroll
            for (int fr = 0; fr < kSynFrames; ++fr)
                sj[fr] = ((uint32_t)fr < nf && syn_b[(size_t)(f0 + fr) * (uint32_t)c.m + j] != 0) ? 1u : 0u;
            for (int k = 0; k < c.max_dc; ++k) {
                const int bit = c.chk_bits[k * c.m_pad + j];
                if (bit < 0) continue;
                deg++;
                const uint32_t wi = (uint32_t)bit >> 5, sh = (uint32_t)bit & 31u;
#pragma unroll
                for (int fr = 0; fr < kSynFrames; ++fr) pb[fr] ^= kb[fr * w32 + wi] >> sh;
            }
        }
#pragma unroll
        for (int fr = 0; fr < kSynFrames; ++fr) {
            const uint64_t sm = __ballot(sj[fr]);
            const uint64_t qm = __ballot((sj[fr] ^ pb[fr] ^ (lsign & deg)) & 1u);
            if (lane == 0 && (uint32_t)fr < nf) {
                uint32_t* o = synw + (size_t)(f0 + fr) * 2 * m_words;
                o[j0 >> 5] = (uint32_t)sm;
                o[(j0 >> 5) + 1] = (uint32_t)(sm >> 32);
                o[m_words + (j0 >> 5)] = (uint32_t)qm;
                o[m_words + (j0 >> 5) + 1] = (uint32_t)(qm >> 32);
            }
        }
    }
    // Bob's key in the internal order: word w's lane l takes original bit
    // perm[64 w + l]; one ballot per frame
    for (uint32_t w = threadIdx.x >> 6; w < words; w += kSynBlock / 64) {
        const uint32_t q = w * 64 + (uint32_t)lane;
        const bool in = q < (uint32_t)c.n;
        const uint32_t o = in ? (uint32_t)c.perm[q] : 0u;
#pragma unroll
        for (int fr = 0; fr < kSynFrames; ++fr) {
            const uint64_t bm = __ballot(in && ((kb[fr * w32 + (o >> 5)] >> (o & 31u)) & 1u));
            if (lane == 0 && (uint32_t)fr < nf) bob_w[(size_t)(f0 + fr) * words + w] = bm;
        }
    }
}

// frame_syn_kernel's work bit-sliced over frames: a workgroup takes 16
// frames and first transposes their keys into 32-bit slices T[i] (bit f =
// Alice's bit i of frame f, bit 16 + f = Bob's; one ballot gives two bit
// positions: lanes 0-31 hold word w of the 16 frames' two keys, lanes 32-63
// word w + 1). A check's parities for all 16 frames and both keys are then
// one XOR of its row's slices, and each internal-order key word one slice read
// per lane followed by a ballot per frame and key. Per frame this reads LDS
// ~15x less than frame_syn_kernel (an 8-byte read per row entry and frame).
// LDS: words * 64 slices of 4 bytes (N <= 40960 in 160 KB).
constexpr int kSlicedFrames = 16;
constexpr int kSlicedBlock = 1024;
constexpr int kSlicedPre = 8;        // key-word pairs a wave loads ahead
// A bit transpose within each 32-lane half of the wave: afterwards lane 32 h +
// c holds in bit r what lane 32 h + r held in bit c. Five butterfly stages
// (s = 16 ... 1): lane l takes its partner l ^ s's value through ds_swizzle,
// rotates it by s toward the bit block it trades (one v_alignbit_b32) and
// keeps its own other block (one v_bfi_b32) -- 2 VALU and a swizzle per stage
// where a ballot per bit and a lane select per bit took ~15 VALU per bit.
template <int S, uint32_t MASK>
__device__ __forceinline__ uint32_t transpose_stage(uint32_t x, uint32_t lane) {
    const uint32_t y = (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x1F | (S << 10));   // lane ^ S
    const bool hi = (lane & (uint32_t)S) != 0;
    const uint32_t ys = __builtin_amdgcn_alignbit(y, y, hi ? (uint32_t)S : 32u - (uint32_t)S);
    const uint32_t k = hi ? ~MASK : MASK;
    return (x & k) | (ys & ~k);
}
__device__ __forceinline__ uint32_t wave_transpose32(uint32_t x, uint32_t lane) {
    x = transpose_stage<16, 0x0000FFFFu>(x, lane);
    x = transpose_stage<8, 0x00FF00FFu>(x, lane);
    x = transpose_stage<4, 0x0F0F0F0Fu>(x, lane);
    x = transpose_stage<2, 0x33333333u>(x, lane);
    return transpose_stage<1, 0x55555555u>(x, lane);
}
// BYTES (qkd_qkd_ldpc_batch's byte keys, N % 8 == 0, rows 8-byte aligned): the
// slices come straight from the caller's 0/1 bytes, and alice_w / bob_w are
// only written (step 3), so no packing kernel runs before this one: per
// thread and pass 8 positions of every frame and key, one 8-byte load each;
// (v & 0x01010101) << f gathers 8 frames' bits of 4 positions into the 4
// bytes of one word, and v_perm_b32 assembles each position's slice from the
// four words (Alice frames 0-7 / 8-15, Bob frames 0-7 / 8-15).
// GIVEN (qkd_reconcile_batch): the target syndrome comes from the caller's
// bytes syn_b[F x M] (nonzero = 1) instead of from Alice's key. Only Bob's key
// is loaded, sliced and rewritten (the Alice halves of the slices stay 0;
// alice_w / alice_b are neither read nor written), and in step 2 the lane of
// check j reads its 16 frames' bytes (consecutive lanes, consecutive bytes; no
// alignment of the rows assumed) in place of the low half of P.
template <bool BYTES, bool GIVEN = false>
__global__ __launch_bounds__(kSlicedBlock) void frame_syn_sliced_kernel(DeviceCode c, uint64_t* alice_w,
                                                                        uint64_t* bob_w, uint32_t words,
                                                                        uint32_t n_frames, uint32_t lsign,
                                                                        uint32_t* synw, uint32_t* counter,
                                                                        uint32_t* win, uint32_t win_words,
                                                                        const uint8_t* alice_b,
                                                                        const uint8_t* bob_b,
                                                                        const uint8_t* syn_b) {
    extern __shared__ uint32_t T[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // (uniform to the compiler)
    constexpr uint32_t NW = kSlicedBlock / 64;
    if (blockIdx.x == 0 && tid < 2) counter[tid] = 0;     // (the decoder's queue, as frame_syn_kernel)
    for (uint32_t i = blockIdx.x * kSlicedBlock + tid; i < win_words; i += gridDim.x * kSlicedBlock) win[i] = 0;
    const uint32_t f0 = blockIdx.x * kSlicedFrames;
    const uint32_t nf = min((uint32_t)kSlicedFrames, n_frames - f0);
    const uint32_t fr = lane & 15u;
    const bool bob_lane = (lane & 16u) != 0;
    const uint32_t half = lane >> 5;                      // which word of the pair
    const uint32_t pairs = (words + 1) / 2;
    // 1. slices: wave takes word pairs p = wave, wave + NW, ..., loading up to
    //    kSlicedPre of them ahead; lane b keeps the ballot of bit b: the
    //    slices of positions 64 (2p) + b (low half) and 64 (2p + 1) + b (high)
    auto load_pair = [&](uint32_t p) -> uint64_t {
        const uint32_t w = 2 * p + half;
        if (p >= pairs || w >= words || fr >= nf) return 0;
        if constexpr (GIVEN)
            if (!bob_lane) return 0;
        return (bob_lane ? bob_w : alice_w)[(size_t)(f0 + fr) * words + w];
    };
    auto slice_pair = [&](uint32_t p, uint64_t v) {
        // the lanes of half h hold word 2p + h of the 16 frames' keys (lane
        // 16 key + frame): transposed, lane 32 h + c holds the slice of that
        // word's bit c (low 32 bits) or bit 32 + c (high)
        const uint32_t tlo = wave_transpose32((uint32_t)v, lane);
        const uint32_t thi = wave_transpose32((uint32_t)(v >> 32), lane);
        const uint32_t w = 2 * p + half, b = lane & 31u;
        if (w < words) {
            T[(size_t)w * 64 + b] = tlo;
            T[(size_t)w * 64 + 32 + b] = thi;
        }
    };
    if constexpr (BYTES) {
        const uint32_t n = (uint32_t)c.n;
        for (uint32_t p = tid; p * 8 < n; p += kSlicedBlock) {
            uint2 va[kSlicedFrames], vb[kSlicedFrames];
#pragma unroll
            for (uint32_t f = 0; f < (uint32_t)kSlicedFrames; ++f) {
                const size_t off = (size_t)(f0 + f) * n + 8 * p;
                if constexpr (GIVEN) va[f] = make_uint2(0, 0);
                else va[f] = f < nf ? *reinterpret_cast<const uint2*>(alice_b + off) : make_uint2(0, 0);
                vb[f] = f < nf ? *reinterpret_cast<const uint2*>(bob_b + off) : make_uint2(0, 0);
            }
            // x[key][frame half][position half]: byte k bit f' = that key's bit
            // at position 4 * (position half) + k of frame 8 * (frame half) + f'
            uint32_t x[2][2][2] = {};
#pragma unroll
            for (uint32_t f = 0; f < (uint32_t)kSlicedFrames; ++f) {
                const uint32_t h = f >> 3, sh = f & 7u;
                x[0][h][0] |= (va[f].x & 0x01010101u) << sh;
                x[0][h][1] |= (va[f].y & 0x01010101u) << sh;
                x[1][h][0] |= (vb[f].x & 0x01010101u) << sh;
                x[1][h][1] |= (vb[f].y & 0x01010101u) << sh;
            }
            uint32_t sl[8];
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) {
                const uint32_t ph = k >> 2, b = k & 3u;
                // bytes 0-1: Alice frames 0-7 / 8-15; 2-3: Bob's (selector 12: 0x00)
                const uint32_t lo = __builtin_amdgcn_perm(x[0][1][ph], x[0][0][ph], b | ((b + 4) << 8) | 0x0c0c0000u);
                const uint32_t hi = __builtin_amdgcn_perm(x[1][1][ph], x[1][0][ph], 0x0c0cu | (b << 16) | ((b + 4) << 24));
                sl[k] = lo | hi;
            }
            // (positions past N are never read: rows and perm hold bits < N)
            *reinterpret_cast<uint4*>(T + 8 * p) = make_uint4(sl[0], sl[1], sl[2], sl[3]);
            *reinterpret_cast<uint4*>(T + 8 * p + 4) = make_uint4(sl[4], sl[5], sl[6], sl[7]);
        }
    } else {
        for (uint32_t p0 = wave; p0 < pairs; p0 += NW * kSlicedPre) {
            uint64_t v[kSlicedPre];
#pragma unroll
            for (int k = 0; k < kSlicedPre; ++k) v[k] = load_pair(p0 + (uint32_t)k * NW);
#pragma unroll
            for (int k = 0; k < kSlicedPre; ++k)
                if (p0 + (uint32_t)k * NW < pairs) slice_pair(p0 + (uint32_t)k * NW, v[k]);
        }
    }
    __syncthreads();
    // 2. syndromes: lane = check; 64 checks per wave and pass, then per frame
    //    two ballots (target s_j, first-product sign q_j) that lane f keeps
    const int m_words = decode_m_words(c.m);
    const int rs = c.chk_rs;
    for (uint32_t j0 = wave * 64; j0 < (uint32_t)c.m; j0 += kSlicedBlock) {
        const uint32_t j = j0 + lane;
        uint32_t P = 0, deg = 0;
        if (j < (uint32_t)c.m) {
            const uint16_t* row = c.chk_rows16 + (size_t)j * rs;
            for (int h = 0; h < rs; h += 8) {
                const uint4 r = *reinterpret_cast<const uint4*>(row + h);
                const uint32_t e[8] = {r.x & 0xffffu, r.x >> 16, r.y & 0xffffu, r.y >> 16,
                                       r.z & 0xffffu, r.z >> 16, r.w & 0xffffu, r.w >> 16};
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (e[k] != 0xffffu) {
                        P ^= T[e[k]];
                        deg++;
                    }
            }
            if constexpr (GIVEN) {
                // the caller's target bits of this check, frame f in bit f
                uint8_t sb[kSlicedFrames];
#pragma unroll
                for (uint32_t f = 0; f < (uint32_t)kSlicedFrames; ++f)
                    sb[f] = f < nf ? syn_b[(size_t)(f0 + f) * (uint32_t)c.m + j] : (uint8_t)0;
                uint32_t tb = 0;
#pragma unroll
                for (uint32_t f = 0; f < (uint32_t)kSlicedFrames; ++f) tb |= (sb[f] != 0 ? 1u : 0u) << f;
                P = (P & 0xffff0000u) | tb;
            }
        }
        const uint32_t Q = P ^ (P >> 16) ^ ((lsign & deg) ? 0xffffu : 0u);   // low 16: q bits
        // transposed, lane f < 16 holds frame f's target bits of the 64 checks
        // (its own value the low word, lane 32 + f's the high) and lane 16 + f
        // its q bits; both go out as one 8-byte store (m_words and j0 / 32 even)
        const uint32_t tr = wave_transpose32((P & 0xffffu) | (Q << 16), lane);
        const uint32_t up = (uint32_t)__shfl_xor((int)tr, 32);
        const uint32_t g = lane & 15u;
        if (lane < 32 && g < nf) {
            uint32_t* o = synw + (size_t)(f0 + g) * 2 * m_words + (lane < 16 ? 0 : m_words) + (j0 >> 5);
            *reinterpret_cast<uint2*>(o) = make_uint2(tr, up);
        }
    }
    // 3. the keys in the internal order (DeviceCode::perm), in place: word w's
    //    lane l reads the slice of original bit perm[64 w + l] (the perm entry
    //    of the wave's next word loaded a word ahead, through a clamped index:
    //    no branch around the load); transposed, lane f < 16 holds Alice's word
    //    of frame f (high half from lane 32 + f), lane 16 + f Bob's
    const uint32_t cn = (uint32_t)c.n;
    auto perm_at = [&](uint32_t w) -> uint32_t {
        const uint32_t q = w * 64 + lane;
        return c.perm[q < cn ? q : 0u];
    };
    uint32_t pq = perm_at(wave < (uint32_t)words ? wave : 0u);
    for (uint32_t w = wave; w < words; w += NW) {
        const uint32_t wn = w + NW;
        const uint32_t pn = perm_at(wn < (uint32_t)words ? wn : w);
        const uint32_t S = w * 64 + lane < cn ? T[pq] : 0u;
        const uint32_t tr = wave_transpose32(S, lane);
        const uint32_t up = (uint32_t)__shfl_xor((int)tr, 32);
        const uint32_t g = lane & 15u;
        if (lane < 32 && g < nf && !(GIVEN && lane < 16))
            (lane < 16 ? alice_w : bob_w)[(size_t)(f0 + g) * words + w] = ((uint64_t)up << 32) | tr;
        pq = pn;
    }
}

hipError_t launch_frame_syn(const DecodeArgs& a, hipStream_t stream, bool gather, bool pack_first) {
    const uint32_t lsign = (uint32_t)qkdm::hi32(a.log_p) >> 31;
    // the bit-sliced form when its slices fit LDS and the compact rows exist
    // (gather, the QKD_SYN_SLICED option 0: frame_syn_kernel; tests compare the two)
    const size_t slds = (size_t)a.words * 64 * sizeof(uint32_t);
    const bool sliced = a.code.chk_rows16 && slds <= kLdsBytesMax && !gather;
    // the target syndrome given by the caller (qkd_reconcile_batch: a.syn set,
    // no Alice key): the GIVEN kernels, Bob's key alone
    const bool given = a.syn != nullptr;
    // byte keys (qkd_qkd_ldpc_batch, qkd_reconcile_batch): packed by the sliced
    // kernel itself when their rows allow 8-byte loads (pack_first, the
    // QKD_SYN_BYTES option 0: pack_kernel first; tests compare the two), else
    // by pack_kernel
    const bool bytes = a.bob_b && sliced && a.code.n % 8 == 0 &&
                       ((reinterpret_cast<uintptr_t>(a.alice_b) | reinterpret_cast<uintptr_t>(a.bob_b)) & 7u) == 0 &&
                       !pack_first;
    if (a.bob_b && !bytes) {
        const hipError_t e = launch_pack_keys(a, stream);
        if (e != hipSuccess) return e;
    }
    if (sliced) {
        const void* fn = given ? (bytes ? (const void*)frame_syn_sliced_kernel<true, true>
                                        : (const void*)frame_syn_sliced_kernel<false, true>)
                               : (bytes ? (const void*)frame_syn_sliced_kernel<true>
                                        : (const void*)frame_syn_sliced_kernel<false>);
        // (the attribute on every launch, for the current device, as decode_grid
        // does for the decoder: no process-wide flag to race on or to skip for
        // a second device)
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytesMax);
        if (e != hipSuccess) return e;
        const dim3 grid((a.n_frames + kSlicedFrames - 1) / kSlicedFrames);
        if (given && bytes)
            hipLaunchKernelGGL((frame_syn_sliced_kernel<true, true>), grid, dim3(kSlicedBlock), slds, stream, a.code,
                               nullptr, const_cast<uint64_t*>(a.bob_w), a.words, a.n_frames, lsign,
                               const_cast<uint32_t*>(a.synw), a.counter, a.win, 2 * a.win_count, nullptr, a.bob_b,
                               a.syn);
        else if (given)
            hipLaunchKernelGGL((frame_syn_sliced_kernel<false, true>), grid, dim3(kSlicedBlock), slds, stream, a.code,
                               nullptr, const_cast<uint64_t*>(a.bob_w), a.words, a.n_frames, lsign,
                               const_cast<uint32_t*>(a.synw), a.counter, a.win, 2 * a.win_count, nullptr, nullptr,
                               a.syn);
        else if (bytes)
            hipLaunchKernelGGL(frame_syn_sliced_kernel<true>, grid, dim3(kSlicedBlock), slds, stream, a.code,
                               const_cast<uint64_t*>(a.alice_w), const_cast<uint64_t*>(a.bob_w), a.words,
                               a.n_frames, lsign, const_cast<uint32_t*>(a.synw), a.counter, a.win,
                               2 * a.win_count, a.alice_b, a.bob_b, nullptr);
        else
            hipLaunchKernelGGL(frame_syn_sliced_kernel<false>, grid, dim3(kSlicedBlock), slds, stream, a.code,
                               const_cast<uint64_t*>(a.alice_w), const_cast<uint64_t*>(a.bob_w), a.words,
                               a.n_frames, lsign, const_cast<uint32_t*>(a.synw), a.counter, a.win,
                               2 * a.win_count, nullptr, nullptr, nullptr);
        return hipGetLastError();
    }
    const dim3 ggrid((a.n_frames + kSynFrames - 1) / kSynFrames);
    if (given) {
        const size_t glds = (size_t)kSynFrames * 2 * a.words * sizeof(uint32_t);
        hipLaunchKernelGGL(frame_syn_given_kernel, ggrid, dim3(kSynBlock), glds, stream, a.code,
                           const_cast<uint64_t*>(a.bob_w), a.syn, a.words, a.n_frames, lsign,
                           const_cast<uint32_t*>(a.synw), a.counter, a.win, 2 * a.win_count);
        return hipGetLastError();
    }
    const size_t lds = (size_t)kSynFrames * 2 * a.words * sizeof(uint64_t);
    hipLaunchKernelGGL(frame_syn_kernel, ggrid, dim3(kSynBlock), lds,
                       stream, a.code, const_cast<uint64_t*>(a.alice_w), const_cast<uint64_t*>(a.bob_w), a.words,
                       a.n_frames, lsign, const_cast<uint32_t*>(a.synw), a.counter, a.win, 2 * a.win_count);
    return hipGetLastError();
}

}  // namespace qkd
