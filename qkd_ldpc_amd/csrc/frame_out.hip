// frame_out.hip — what follows a decoder on a frame's decisions: bits_out from
// the split decoder's packed words (zout_unpack*), Bob's corrected-bit counts
// (count_flips) and the key verification tags (qkd_verify.h), with their
// launchers and the two tag entries of the ABI. The reference has the key
// compare alone (arrays_equal, src/qkd_ldpc_algorithm.cpp:433).
// Built with the split decoder's scheduler strategy (Makefile), as when these
// kernels stood in decode_split.hip.
#include <hip/hip_runtime.h>

#include "qkd_args.h"
#include "qkd_decode.h"
#include "qkd_host.h"

namespace qkd {

// bits_out[f][bit] from the decoder's packed decisions in the internal bit
// order (DeviceCode::inv)
__global__ void zout_unpack_kernel(const uint64_t* zout, const int32_t* inv, uint32_t n, uint32_t words,
                                   uint32_t n_frames, uint8_t* out) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (size_t)n_frames * n) return;
    const size_t f = gid / n;
    const uint32_t q = (uint32_t)inv[gid - f * n];
    out[gid] = (uint8_t)((zout[f * words + (q >> 6)] >> (q & 63)) & 1u);
}

// The sum of v over the workgroup's threads, at thread 0 (red: one word per wave).
constexpr int kCountBlock = 256;
__device__ __forceinline__ uint32_t count_block_sum(uint32_t v, uint32_t* red) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kCountBlock / 64; ++w) t += red[w];
    return t;
}

// zout_unpack_kernel for qkd_reconcile_batch with a corrected[] output: a
// workgroup per frame stages the frame's decision words in LDS, writes
// bits_out through inv and counts the positions where the decision differs
// from Bob's byte key (original order): corrected[f] = popcount(bits_out ^
// bob), no atomics. quad (the host's choice: N % 4 == 0, bob and out 4-byte
// aligned): four positions per thread and pass, one 4-byte load and store.
__global__ __launch_bounds__(kCountBlock) void zout_unpack_count_kernel(const uint64_t* zout, const int32_t* inv,
                                                                        uint32_t n, uint32_t words,
                                                                        const uint8_t* bob, uint8_t* out,
                                                                        uint32_t* corrected, uint32_t quad) {
    extern __shared__ uint64_t zf[];
    __shared__ uint32_t red[kCountBlock / 64];
    const size_t f = blockIdx.x;
    for (uint32_t w = threadIdx.x; w < words; w += kCountBlock) zf[w] = zout[f * words + w];
    __syncthreads();
    auto bit_at = [&](int32_t q) -> uint32_t { return (uint32_t)(zf[(uint32_t)q >> 6] >> ((uint32_t)q & 63u)) & 1u; };
    uint32_t cnt = 0;
    if (quad) {
        for (uint32_t i = threadIdx.x * 4; i < n; i += kCountBlock * 4) {
            const int4 q = *reinterpret_cast<const int4*>(inv + i);
            const uint32_t d = bit_at(q.x) | (bit_at(q.y) << 8) | (bit_at(q.z) << 16) | (bit_at(q.w) << 24);
            const uint32_t b = *reinterpret_cast<const uint32_t*>(bob + f * n + i) & 0x01010101u;
            *reinterpret_cast<uint32_t*>(out + f * n + i) = d;
            cnt += (uint32_t)__popc(d ^ b);
        }
    } else {
        for (uint32_t i = threadIdx.x; i < n; i += kCountBlock) {
            const uint32_t d = bit_at(inv[i]);
            out[f * n + i] = (uint8_t)d;
            cnt += d ^ (uint32_t)(bob[f * n + i] & 1u);
        }
    }
    const uint32_t total = count_block_sum(cnt, red);
    if (threadIdx.x == 0) corrected[f] = total;
}

// The classic kernel writes bits_out itself: corrected[f] = popcount(bits_out
// ^ bob) of a frame per workgroup (qkd_reconcile_batch, corrected != NULL).
__global__ __launch_bounds__(kCountBlock) void count_flips_kernel(const uint8_t* bits, const uint8_t* bob, uint32_t n,
                                                                  uint32_t* corrected) {
    __shared__ uint32_t red[kCountBlock / 64];
    const size_t f = blockIdx.x;
    uint32_t cnt = 0;
    for (uint32_t i = threadIdx.x; i < n; i += kCountBlock) cnt += (uint32_t)((bits[f * n + i] ^ bob[f * n + i]) & 1u);
    const uint32_t total = count_block_sum(cnt, red);
    if (threadIdx.x == 0) corrected[f] = total;
}

// ---- key verification tags (qkd_verify.h) -----------------------------------
// The frame's key string in LDS: R[0 .. key_words) from the caller's words or
// from the seed, and a zero word after them (qkdv::verify_xor_run reads one
// 32-bit word past its windows at every position).
__device__ __forceinline__ void verify_stage_key(uint64_t* R, const VerifyArgs& v) {
    for (uint32_t k = threadIdx.x; k <= v.key_words; k += kCountBlock)
        R[k] = k == v.key_words ? 0ull : (v.words ? v.words[k] : qkdv::verify_key_word(v.seed, k));
}

// The XOR of v over the workgroup's threads, at thread 0 (red: one word per wave).
__device__ __forceinline__ uint64_t verify_block_xor(uint64_t v, uint64_t* red) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        lo ^= (uint32_t)__shfl_xor((int)lo, s);
        hi ^= (uint32_t)__shfl_xor((int)hi, s);
    }
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = ((uint64_t)hi << 32) | lo;
    __syncthreads();
    uint64_t t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kCountBlock / 64; ++w) t ^= red[w];
    return t;
}

// Thread 0's epilogue: the masked tag out and, against Alice's, the verdict.
__device__ __forceinline__ void verify_finish(const VerifyArgs& v, size_t f, uint64_t total) {
    const uint64_t tag = total & v.mask;
    if (v.tags_out) v.tags_out[f] = tag;
    if (v.alice_tags) v.verified[f] = (v.sp_ok[f] != 0 && ((tag ^ v.alice_tags[f]) & v.mask) == 0) ? 1 : 0;
}

// The tags of byte keys (qkd_verify_tags_batch; qkd_reconcile_verify_batch
// after the classic kernel, which wrote bits_out itself): a workgroup per
// frame, the key string staged in LDS once, acc ^= W(p) & -(bit) over the
// frame's positions, a block XOR, one ordinary store. No atomics. wide (the
// host's choice: N % 8 == 0, bits 8-byte aligned): eight positions per thread
// and pass from one 8-byte load; else a byte per thread and pass.
__global__ __launch_bounds__(kCountBlock) void verify_tags_kernel(const uint8_t* bits, uint32_t n, uint32_t wide,
                                                                  VerifyArgs v) {
    extern __shared__ uint64_t vR[];
    __shared__ uint64_t red[kCountBlock / 64];
    const size_t f = blockIdx.x;
    verify_stage_key(vR, v);
    __syncthreads();
    const uint32_t* r32 = reinterpret_cast<const uint32_t*>(vR);
    uint64_t acc = 0;
    if (wide) {
        for (uint32_t i = threadIdx.x * 8; i < n; i += kCountBlock * 8)
            acc ^= qkdv::verify_xor_run<8>(r32, i, *reinterpret_cast<const uint64_t*>(bits + f * n + i));
    } else {
        for (uint32_t i = threadIdx.x; i < n; i += kCountBlock) acc ^= qkdv::verify_xor_run<1>(r32, i, bits[f * n + i]);
    }
    const uint64_t total = verify_block_xor(acc, red);
    if (threadIdx.x == 0) verify_finish(v, f, total);
}

// zout_unpack_count_kernel that also takes the frame's verification tag
// (qkd_reconcile_verify_batch on the split path): the decision d at original
// position i, already in hand for bits_out, adds W(i) & -(d) to the thread's
// XOR; the key string sits in LDS after the decision words. corrected may be
// nullptr: Bob's bytes are then not read at all (and quad asks nothing of
// them).
__global__ __launch_bounds__(kCountBlock) void zout_unpack_verify_kernel(const uint64_t* zout, const int32_t* inv,
                                                                         uint32_t n, uint32_t words,
                                                                         const uint8_t* bob, uint8_t* out,
                                                                         uint32_t* corrected, uint32_t quad,
                                                                         VerifyArgs v) {
    extern __shared__ uint64_t zf[];          // [words] decisions, [key_words + 1] key string
    __shared__ uint32_t red[kCountBlock / 64];
    __shared__ uint64_t xred[kCountBlock / 64];
    uint64_t* R = zf + words;
    const uint32_t* r32 = reinterpret_cast<const uint32_t*>(R);
    const size_t f = blockIdx.x;
    for (uint32_t w = threadIdx.x; w < words; w += kCountBlock) zf[w] = zout[f * words + w];
    verify_stage_key(R, v);
    __syncthreads();
    auto bit_at = [&](int32_t q) -> uint32_t { return (uint32_t)(zf[(uint32_t)q >> 6] >> ((uint32_t)q & 63u)) & 1u; };
    uint32_t cnt = 0;
    uint64_t acc = 0;
    if (quad) {
        for (uint32_t i = threadIdx.x * 4; i < n; i += kCountBlock * 4) {
            const int4 q = *reinterpret_cast<const int4*>(inv + i);
            const uint32_t d = bit_at(q.x) | (bit_at(q.y) << 8) | (bit_at(q.z) << 16) | (bit_at(q.w) << 24);
            *reinterpret_cast<uint32_t*>(out + f * n + i) = d;
            if (corrected) cnt += (uint32_t)__popc(d ^ (*reinterpret_cast<const uint32_t*>(bob + f * n + i) & 0x01010101u));
            acc ^= qkdv::verify_xor_run<4>(r32, i, d);
        }
    } else {
        for (uint32_t i = threadIdx.x; i < n; i += kCountBlock) {
            const uint32_t d = bit_at(inv[i]);
            out[f * n + i] = (uint8_t)d;
            if (corrected) cnt += d ^ (uint32_t)(bob[f * n + i] & 1u);
            acc ^= qkdv::verify_xor_run<1>(r32, i, d);
        }
    }
    if (corrected) {          // (uniform over the launch)
        const uint32_t total = count_block_sum(cnt, red);
        if (threadIdx.x == 0) corrected[f] = total;
    }
    const uint64_t tag = verify_block_xor(acc, xred);
    if (threadIdx.x == 0) verify_finish(v, f, tag);
}

hipError_t launch_key_match(const DecodeArgs& a, hipStream_t stream, uint32_t* corrected, const VerifyArgs* v) {
    // (decode_split_kernel compares the keys itself: keys_match needs no launch)
    if (a.bits_out && v) {
        // qkd_reconcile_verify_batch: the unpack that also takes the tags (and
        // counts the flips when asked to; Bob's bytes are read only then)
        const uint32_t n = (uint32_t)a.code.n;
        const bool quad = n % 4 == 0 && (((corrected ? reinterpret_cast<uintptr_t>(a.bob_b) : 0) |
                                          reinterpret_cast<uintptr_t>(a.bits_out)) & 3u) == 0;
        hipLaunchKernelGGL(zout_unpack_verify_kernel, dim3(a.n_frames), dim3(kCountBlock),
                           ((size_t)a.words + v->key_words + 1) * 8, stream, a.zout, a.code.inv, n, a.words, a.bob_b,
                           a.bits_out, corrected, quad ? 1u : 0u, *v);
    } else if (a.bits_out && corrected) {
        // qkd_reconcile_batch: the unpack that also counts the flips against Bob's bytes
        const uint32_t n = (uint32_t)a.code.n;
        const bool quad = n % 4 == 0 && ((reinterpret_cast<uintptr_t>(a.bob_b) |
                                          reinterpret_cast<uintptr_t>(a.bits_out)) & 3u) == 0;
        hipLaunchKernelGGL(zout_unpack_count_kernel, dim3(a.n_frames), dim3(kCountBlock), (size_t)a.words * 8, stream,
                           a.zout, a.code.inv, n, a.words, a.bob_b, a.bits_out, corrected, quad ? 1u : 0u);
    } else if (a.bits_out) {
        const size_t total = (size_t)a.n_frames * a.code.n;
        hipLaunchKernelGGL(zout_unpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a.zout,
                           a.code.inv, (uint32_t)a.code.n, a.words, a.n_frames, a.bits_out);
    }
    return hipGetLastError();
}

hipError_t launch_count_flips(const uint8_t* bits, const uint8_t* bob, uint32_t n, uint32_t n_frames,
                              uint32_t* corrected, hipStream_t stream) {
    hipLaunchKernelGGL(count_flips_kernel, dim3(n_frames), dim3(kCountBlock), 0, stream, bits, bob, n, corrected);
    return hipGetLastError();
}

hipError_t launch_verify_tags(const uint8_t* bits, uint32_t n, uint32_t n_frames, const VerifyArgs& v,
                              hipStream_t stream) {
    const bool wide = n % 8 == 0 && (reinterpret_cast<uintptr_t>(bits) & 7u) == 0;
    hipLaunchKernelGGL(verify_tags_kernel, dim3(n_frames), dim3(kCountBlock), ((size_t)v.key_words + 1) * 8, stream,
                       bits, n, wide ? 1u : 0u, v);
    return hipGetLastError();
}

VerifyArgs verify_args(const qkd_code* c, uint64_t hash_seed, const uint64_t* hash_words, uint32_t tag_bits,
                       const uint64_t* alice_tags, uint64_t* tags_out, uint8_t* verified, const uint8_t* sp_ok) {
    VerifyArgs v{};
    v.seed = hash_seed;
    v.words = hash_words;
    v.key_words = (uint32_t)qkdv::verify_key_words(c->n);
    v.mask = qkdv::verify_tag_mask(tag_bits);
    v.alice_tags = alice_tags;
    v.tags_out = tags_out;
    v.verified = verified;
    v.sp_ok = sp_ok;
    return v;
}

}  // namespace qkd

using namespace qkd;

extern "C" {

qkd_status qkd_verify_tags_batch(const qkd_code* c, const uint8_t* bits, size_t n_frames, uint64_t hash_seed,
                                 const uint64_t* hash_words, uint32_t tag_bits, uint64_t* tags, void* stream) {
    clear_error();
    if (const char* bad = qkda::verify_tags_args_error(c, bits, n_frames, tag_bits, tags))
        return set_error(QKD_ERR_INVALID_ARG, "%s", bad);
    DeviceGuard g(c->device);
    const VerifyArgs v = verify_args(c, hash_seed, hash_words, tag_bits, nullptr, tags, nullptr, nullptr);
    QKD_HIP(launch_verify_tags(bits, (uint32_t)c->n, (uint32_t)n_frames, v, (hipStream_t)stream));
    return QKD_OK;
}

qkd_status qkd_adapt_verify_tags_batch(const qkd_adapt* ad, const uint8_t* payload, size_t n_frames,
                                       uint64_t hash_seed, const uint64_t* hash_words, uint32_t tag_bits,
                                       uint64_t* tags, void* stream) {
    clear_error();
    if (const char* bad = qkda::adapt_verify_tags_args_error(ad, payload, n_frames, tag_bits, tags))
        return set_error(QKD_ERR_INVALID_ARG, "%s", bad);
    DeviceGuard g(ad->device);
    // the byte-key tag kernel over the payload: positions are payload indices
    VerifyArgs v{};
    v.seed = hash_seed;
    v.words = hash_words;
    v.key_words = (uint32_t)qkdv::verify_key_words(ad->n_payload);
    v.mask = qkdv::verify_tag_mask(tag_bits);
    v.tags_out = tags;
    QKD_HIP(launch_verify_tags(payload, (uint32_t)ad->n_payload, (uint32_t)n_frames, v, (hipStream_t)stream));
    return QKD_OK;
}

}  // extern "C"
