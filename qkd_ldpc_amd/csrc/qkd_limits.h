// qkd_limits.h — sizes and limits shared by the kernels and the host-side code
// layout (qkd_layout.h). No HIP header: also compiled by the native tests.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QKD_LHD __host__ __device__
#else
#define QKD_LHD
#endif

namespace qkd {

// Threads per decode workgroup: one workgroup decodes one frame at a time.
#ifndef QKD_DECODE_BLOCK
#define QKD_DECODE_BLOCK 1024
#endif
constexpr int kDecodeBlock = QKD_DECODE_BLOCK;
// Second-iteration tanh table (decode.hip): entries per degree pattern are
// 2^(1 + max_dv) sign codes x max_dv rows; the table is used when
// max_dv <= kTab2MaxDv and n_pat * entries <= kTab2MaxEntries.
constexpr int kTab2MaxDv = 3;   // <= the bit phase's unrolled rows (decode.hip kDvUnroll)
constexpr int kTab2MaxEntries = 2048;
// per-bit arrays of the split kernels (bit_code, bit_pat): rounds of padding
// past the last round, >= the largest bit-phase load batch minus one
constexpr int kBitPadRounds = 4;
QKD_LHD inline int tab2_stride(int max_dv) { return (1 << (1 + max_dv)) * max_dv; }

// Largest check degree: one check's edges fit one wavefront (qkd_plan.h).
constexpr int kMaxCheckDegree = 64;
// The per-frame bit totals live in LDS as binary64: N <= this.
constexpr int kMaxBitsLds = 20480;
// The split-store kernels (decode_split.hip): Bob's bits of a thread's
// bit-phase rounds in one 64-bit register, 64 rounds of kDecodeBlock bits
constexpr int kMaxBitsSplit = 64 * kDecodeBlock;
// longer codes (the frame-interleaved decoder and its exact hand-off kernel,
// decode_split_kernel<..., LONG>): the split view's arrays exist up to this
constexpr int kMaxBitsSplitLong = 128 * kDecodeBlock;
// (the split decoder's encoded segment words hold (j >> 5) * 4 in 13 bits:
// qkd_decode.h encode_seg)
constexpr int32_t kMaxChecksSplit = 65536;
// Parallel key generation: 64 lanes per frame, jump levels log2(64); frames
// with more flipped positions than this take the serial kernel.
// keygen_fast_kernel: kKeygenLanes lanes per frame (kKeygenLevels = log2 of
// it jump levels), kKeygenFrames frames per workgroup of kKeygenBlock threads
#ifndef QKD_KEYGEN_LEVELS
#define QKD_KEYGEN_LEVELS 6
#endif
constexpr int kKeygenLevels = QKD_KEYGEN_LEVELS;
constexpr int kKeygenLanes = 1 << kKeygenLevels;
constexpr int kKeygenBlock = kKeygenLanes < 64 ? 64 : kKeygenLanes;   // threads per workgroup
constexpr int kKeygenFrames = kKeygenBlock / kKeygenLanes;
constexpr uint32_t kKeygenFastMaxErrors = 4096;
// keygen_split_kernel: lanes per frame in each of its two waves (Alice's bits,
// shuffle draws), so 64 / kKgSplitLanes frames per 128-thread workgroup
#ifndef QKD_KG_SPLIT_LANES
#define QKD_KG_SPLIT_LANES 64
#endif
constexpr uint32_t kKgSplitLanes = QKD_KG_SPLIT_LANES;
// wave pairs (one Alice wave, one shuffle wave) per workgroup
#ifndef QKD_KG_PAIRS
#define QKD_KG_PAIRS 1
#endif
constexpr uint32_t kKgPairs = QKD_KG_PAIRS;
constexpr uint32_t kKgBlock = 128 * kKgPairs;
constexpr uint32_t kKgSplitFrames = kKgPairs * (64 / kKgSplitLanes);
static_assert(kKgSplitLanes >= 1 && 64 % kKgSplitLanes == 0, "lanes per frame divide a wave");

}  // namespace qkd
