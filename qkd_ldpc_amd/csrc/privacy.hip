// privacy.hip — privacy amplification (qkd_privacy_amplify_batch): the Hankel
// hash of qkd_privacy.h over a batch of byte keys, in two forms with the same
// output bits:
//   direct  one workgroup per (frame, tile of outputs); a lane owns one 32-bit
//           output word and XORs in the funnel-shifted window of the key
//           string for every set input bit. The verification kernel widened.
//   table   one workgroup per (group of 32 frames, tile of outputs); bit-sliced
//           over the frames, four-Russians tables over groups of 8 positions
//           in LDS; a lane owns output bits and does one lookup per 8
//           positions x 32 frames.
// Both walk the positions in chunks and stage only the chunk's stretch of the
// key string in LDS (the whole string of a long block is up to 256 KB). No
// atomics, no workspace: plain loads, LDS and vector stores.
#include <algorithm>

#include "qkd_internal.h"
// (after the HIP runtime header, whose function attributes they use)
#include "qkd_args.h"
#include "qkd_privacy.h"

static_assert(qkdv::kPrivacyMaxBits == QKD_PRIVACY_MAX_BITS, "the header's limit is the kernels'");

namespace qkd {
namespace {

struct PrivacyArgs {
    const uint8_t* keys;       // [F x n_in] bytes
    const uint8_t* keep;       // [F] or nullptr
    const uint64_t* words;     // the caller's key string or nullptr (seeded)
    uint64_t seed;
    uint64_t* out;             // [F x wo]
    uint32_t n_frames, n_in, out_bits;
    uint32_t key_words;        // qkdv::privacy_key_words(n_in, out_bits)
    uint32_t wo;               // qkdv::privacy_out_words(out_bits)
    uint32_t n_tiles;          // output tiles per frame (direct) or frame group (table)
};

// ---- direct form ------------------------------------------------------------
// Up to kDirBlock lanes, lane t owning 32-bit output word tile * blockDim.x + t.
// Per chunk of kDirChunk positions the input bits are packed by ballots into
// kDirChunk / 32 words (uniform over the workgroup) and the key string's
// 32-bit words (chunk start / 32 + first output word) .. + kDirChunk / 32 +
// blockDim.x are staged; for 32 positions from q a lane's windows all lie in
// its two staged words q / 32 + t and q / 32 + t + 1.
constexpr uint32_t kDirBlock = 256;
constexpr uint32_t kDirChunk = 1024;
constexpr uint32_t kDirKey = kDirChunk / 32 + kDirBlock + 1;

__global__ __launch_bounds__(kDirBlock) void privacy_direct_kernel(PrivacyArgs a) {
    __shared__ uint32_t kr[kDirKey];
    __shared__ uint32_t xb[kDirChunk / 32];
    const uint32_t t = threadIdx.x, nt = blockDim.x;        // nt: a multiple of 64, <= kDirBlock
    const uint32_t ow = 2u * a.wo;                           // 32-bit output words per frame
    uint32_t* out32 = reinterpret_cast<uint32_t*>(a.out);
    const uint64_t total = (uint64_t)a.n_frames * a.n_tiles;
    for (uint64_t item = blockIdx.x; item < total; item += gridDim.x) {
        const uint64_t f = item / a.n_tiles;
        const uint32_t o0 = (uint32_t)(item % a.n_tiles) * nt, o = o0 + t;
        uint32_t acc = 0;
        if (!a.keep || a.keep[f]) {
            const uint8_t* x = a.keys + f * a.n_in;
            for (uint32_t p0 = 0; p0 < a.n_in; p0 += kDirChunk) {
                __syncthreads();                             // the last chunk's readers are done
                const uint32_t kbase = (p0 >> 5) + o0;
                for (uint32_t j = t; j < kDirChunk / 32 + nt + 1; j += nt)
                    kr[j] = qkdv::privacy_key_word32(a.seed, a.words, a.key_words, kbase + j);
                for (uint32_t q = t; q < kDirChunk; q += nt) {      // (q - t uniform: whole waves ballot)
                    const uint32_t p = p0 + q;
                    const uint64_t m = __ballot(p < a.n_in && (x[p] & 1));
                    if ((t & 63u) == 0) {
                        xb[q >> 5] = (uint32_t)m;
                        xb[(q >> 5) + 1] = (uint32_t)(m >> 32);
                    }
                }
                __syncthreads();
                const uint32_t n_q = (min(kDirChunk, a.n_in - p0) + 31u) >> 5;
                for (uint32_t g = 0; g < n_q; ++g) {
                    uint32_t bits = __builtin_amdgcn_readfirstlane(xb[g]);
                    if (!bits) continue;
                    const uint32_t lo = kr[g + t], hi = kr[g + t + 1];
                    while (bits) {
                        const uint32_t j = (uint32_t)__builtin_ctz(bits);
                        bits &= bits - 1u;
                        acc ^= qkdv::verify_funnel(hi, lo, j);
                    }
                }
            }
        }
        if (o < ow) out32[f * ow + o] = acc & qkdv::privacy_word_mask32(a.out_bits, o);
    }
}

// ---- table form -------------------------------------------------------------
// kTabBlock lanes; a workgroup's tile is kTabTile = kTabBlock * kTabOpl output
// bits, lane t owning bits tile start + t + kTabBlock * k, k < kTabOpl, each
// with a 32-bit accumulator whose bit f belongs to frame f of the group.
// Per chunk of kTabChunk positions:
//   1. the kTabBlock / kTabChunk lanes of a position read its byte in 32 /
//      that many frames each (coalesced over the lanes of a frame) and store
//      their bytes of the position's slice word sl[position];
//   2. half tables: for each group of 8 positions the 16 XOR combinations of
//      its low and of its high four slices;
//   3. the 256-entry table of each group as one XOR of two half entries, and
//      the chunk's stretch of the key string;
//   4. per 32 positions a lane takes the 32 key bits r[p + i ..] of each of its
//      outputs (one funnel shift of two staged words) and per byte of them one
//      lookup and one XOR.
// At the end the accumulators go through LDS to be packed per frame.
// kTabOpl is a template parameter (1, 2 or 4): a larger tile spreads the table
// build over more lookups, a smaller one gives more workgroups. The block is
// the largest there is, so that the most lanes share one build (measured, per
// config-2 batch: 0.21 ms with 1024 lanes against 0.24 with 256, best tile each).
#ifndef QKD_PRIVACY_BLOCK
#define QKD_PRIVACY_BLOCK 1024
#endif
constexpr uint32_t kTabBlock = QKD_PRIVACY_BLOCK;
constexpr uint32_t kTabMaxOpl = 4;
constexpr uint32_t kTabChunk = 256;
constexpr uint32_t kTabGroups = kTabChunk / 8;
constexpr uint32_t kTabParts = kTabBlock / kTabChunk;      // lanes per position in step 1
constexpr uint32_t kTabPartFrames = 32 / kTabParts;        // frames each of them reads
static_assert(kTabBlock % kTabChunk == 0 && kTabBlock <= 1024 && kTabPartFrames % 8 == 0 && kTabPartFrames * kTabParts == 32,
              "step 1: a position's lanes split the 32 frames in whole bytes of the slice word");
static_assert(kTabBlock * kTabMaxOpl * 33 / 32 <= kTabGroups * 256, "the packing buffer reuses the tables");

template <uint32_t kTabOpl>
__global__ __launch_bounds__(kTabBlock) void privacy_table_kernel(PrivacyArgs a) {
    constexpr uint32_t kTabTile = kTabBlock * kTabOpl;
    // staged key words: a lane reads up to word (kTabChunk - 32 + kTabTile - 1) / 32 + 1
    constexpr uint32_t kTabKey = (kTabChunk - 32 + kTabTile - 1) / 32 + 2;
    static_assert(kTabKey <= kTabBlock, "one key word per lane in step 3");
    __shared__ uint32_t tab[kTabGroups * 256];
    __shared__ uint32_t half[kTabGroups * 32];
    __shared__ uint32_t sl[kTabChunk];
    __shared__ uint32_t kr[kTabKey];
    const uint32_t t = threadIdx.x;
    const uint32_t ow = 2u * a.wo;
    uint32_t* out32 = reinterpret_cast<uint32_t*>(a.out);
    const uint64_t total = (((uint64_t)a.n_frames + 31u) >> 5) * a.n_tiles;
    for (uint64_t item = blockIdx.x; item < total; item += gridDim.x) {
        const uint32_t fg = (uint32_t)(item / a.n_tiles);
        const uint32_t i0 = (uint32_t)(item % a.n_tiles) * kTabTile;    // first output bit of the tile
        const uint32_t n_fr = min(32u, a.n_frames - fg * 32u);
        const uint32_t n_k = min(kTabOpl, (a.out_bits - i0 + kTabBlock - 1) / kTabBlock);
        const uint8_t* x = a.keys + (uint64_t)fg * 32u * a.n_in;
        uint32_t acc[kTabOpl];
#pragma unroll
        for (uint32_t k = 0; k < kTabOpl; ++k) acc[k] = 0;

        for (uint32_t p0 = 0; p0 < a.n_in; p0 += kTabChunk) {
            // 1. slices: lane t reads frames part * kTabPartFrames .. of position t % kTabChunk
            {
                const uint32_t pos = t % kTabChunk, part = t / kTabChunk;
                const uint32_t f0 = part * kTabPartFrames;
                const uint32_t n_f = n_fr > f0 ? min(kTabPartFrames, n_fr - f0) : 0u;
                uint32_t s = 0;
                if (p0 + pos < a.n_in) {
                    const uint8_t* xp = x + (uint64_t)f0 * a.n_in + p0 + pos;
                    if (n_f == kTabPartFrames) {
#pragma unroll
                        for (uint32_t f = 0; f < kTabPartFrames; ++f) s |= (uint32_t)(xp[(uint64_t)f * a.n_in] & 1) << f;
                    } else {
                        for (uint32_t f = 0; f < n_f; ++f) s |= (uint32_t)(xp[(uint64_t)f * a.n_in] & 1) << f;
                    }
                }
                uint8_t* dst = reinterpret_cast<uint8_t*>(sl + pos) + f0 / 8;
#pragma unroll
                for (uint32_t b = 0; b < kTabPartFrames / 8; ++b) dst[b] = (uint8_t)(s >> (8 * b));
            }
            __syncthreads();
            // 2. half tables: entry e = group * 32 + half * 16 + combination
            for (uint32_t e = t; e < kTabGroups * 32; e += kTabBlock) {
                const uint32_t* q = sl + (e >> 4) * 4;
                half[e] = ((e & 1u) ? q[0] : 0u) ^ ((e & 2u) ? q[1] : 0u) ^ ((e & 4u) ? q[2] : 0u) ^ ((e & 8u) ? q[3] : 0u);
            }
            __syncthreads();          // (every lane is past the last chunk's lookups here)
            // 3. tables and key stretch
            // (left rolled: unrolled it measured 0.26 against 0.21 ms per config-2 batch)
            for (uint32_t g = t >> 8; g < kTabGroups; g += kTabBlock / 256)
                tab[g * 256 + (t & 255u)] = half[g * 32 + (t & 15u)] ^ half[g * 32 + 16 + ((t >> 4) & 15u)];
            const uint32_t kbase = (p0 + i0) >> 5;      // p0 and i0 are multiples of 32
            if (t < kTabKey) kr[t] = qkdv::privacy_key_word32(a.seed, a.words, a.key_words, kbase + t);
            __syncthreads();
            // 4. lookups
            const uint32_t n_q = (min(kTabChunk, a.n_in - p0) + 31u) >> 5;
            for (uint32_t qw = 0; qw < n_q; ++qw) {
                const uint32_t* tb = tab + qw * 4 * 256;
#pragma unroll
                for (uint32_t k = 0; k < kTabOpl; ++k) {
                    if (k < n_k) {
                        const uint32_t w = qw + (t >> 5) + k * (kTabBlock / 32);
                        const uint32_t v = qkdv::verify_funnel(kr[w + 1], kr[w], t & 31u);
                        acc[k] ^= tb[v & 255u] ^ tb[256 + ((v >> 8) & 255u)] ^ tb[512 + ((v >> 16) & 255u)] ^
                                  tb[768 + (v >> 24)];
                    }
                }
            }
        }

        // pack: output bit i of frame f is bit f of accumulator i; buffer index
        // i + i / 32 keeps a wave's reads (32 words apart) on different banks
        __syncthreads();
        uint32_t* buf = tab;
#pragma unroll
        for (uint32_t k = 0; k < kTabOpl; ++k) {
            const uint32_t i = t + k * kTabBlock;
            buf[i + (i >> 5)] = acc[k];
        }
        __syncthreads();
        for (uint32_t e = t; e < 32u * (kTabTile / 32); e += kTabBlock) {
            const uint32_t j = e % (kTabTile / 32), f = e / (kTabTile / 32);    // tile word, frame of the group
            const uint32_t o = (i0 >> 5) + j;
            if (f >= n_fr || o >= ow) continue;
            const uint64_t fr = (uint64_t)fg * 32u + f;
            uint32_t v = 0;
            if (!a.keep || a.keep[fr]) {
                const uint32_t* b = buf + j * 33u;
#pragma unroll 8
                for (uint32_t bit = 0; bit < 32; ++bit) v |= ((b[bit] >> f) & 1u) << bit;
            }
            out32[fr * ow + o] = v & qkdv::privacy_word_mask32(a.out_bits, o);
        }
        __syncthreads();              // the buffer is the next item's tables
    }
}

constexpr bool kPrivacyDefaultTable = true;
constexpr uint64_t kPrivacyMaxGrid = 1u << 20;
constexpr uint64_t kTabMinItems = 256;      // one workgroup per compute unit

}  // namespace
}  // namespace qkd

using namespace qkd;

extern "C" {

qkd_status qkd_privacy_amplify_batch(int device, const uint8_t* keys, size_t n_frames, uint32_t n_in,
                                     uint32_t out_bits, uint64_t hash_seed, const uint64_t* hash_words,
                                     const uint8_t* keep, uint64_t* out_words, void* stream) {
    clear_error();
    if (const char* bad = qkda::privacy_amplify_args_error(keys, n_frames, n_in, out_bits, out_words))
        return set_error(QKD_ERR_INVALID_ARG, "%s", bad);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return set_error(QKD_ERR_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev)
        return set_error(QKD_ERR_INVALID_ARG, "device %d out of range (%d devices)", device, ndev);
    // "table1" / "table2" / "table4" fix the table form's outputs per lane (A/B runs)
    const DbgOpt form = debug_option(nullptr, "QKD_PRIVACY_KERNEL");
    uint32_t opl = form.is("table1") ? 1u : form.is("table2") ? 2u : form.is("table4") ? 4u : 0u;
    const bool table = opl || form.is("table") || (kPrivacyDefaultTable && !form.is("direct"));
    DeviceGuard g(device);
    PrivacyArgs a{};
    a.keys = keys;
    a.keep = keep;
    a.words = hash_words;
    a.seed = hash_seed;
    a.out = out_words;
    a.n_frames = (uint32_t)n_frames;
    a.n_in = n_in;
    a.out_bits = out_bits;
    a.key_words = (uint32_t)qkdv::privacy_key_words(n_in, out_bits);
    a.wo = (uint32_t)qkdv::privacy_out_words(out_bits);
    if (table) {
        const uint64_t groups = ((uint64_t)a.n_frames + 31u) >> 5;
        // the largest tile that still leaves kTabMinItems workgroups, else the smallest
        if (!opl)
            for (opl = kTabMaxOpl; opl > 1u; opl >>= 1)
                if (groups * ((out_bits + kTabBlock * opl - 1) / (kTabBlock * opl)) >= kTabMinItems) break;
        a.n_tiles = (out_bits + kTabBlock * opl - 1) / (kTabBlock * opl);
        const dim3 grid((uint32_t)std::min(groups * a.n_tiles, kPrivacyMaxGrid));
        if (opl == 4u)
            hipLaunchKernelGGL(privacy_table_kernel<4>, grid, dim3(kTabBlock), 0, (hipStream_t)stream, a);
        else if (opl == 2u)
            hipLaunchKernelGGL(privacy_table_kernel<2>, grid, dim3(kTabBlock), 0, (hipStream_t)stream, a);
        else
            hipLaunchKernelGGL(privacy_table_kernel<1>, grid, dim3(kTabBlock), 0, (hipStream_t)stream, a);
    } else {
        // lanes: the frame's 32-bit output words in whole waves, at most kDirBlock
        const uint32_t lanes = std::min(kDirBlock, (2u * a.wo + 63u) / 64u * 64u);
        a.n_tiles = (2u * a.wo + lanes - 1) / lanes;
        const uint64_t total = (uint64_t)a.n_frames * a.n_tiles;
        hipLaunchKernelGGL(privacy_direct_kernel, dim3((uint32_t)std::min(total, kPrivacyMaxGrid)), dim3(lanes), 0,
                           (hipStream_t)stream, a);
    }
    QKD_HIP(hipGetLastError());
    return QKD_OK;
}

}  // extern "C"
