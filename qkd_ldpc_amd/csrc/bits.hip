// bits.hip — syndromes and bit packing of byte keys, in the original bit order.
//
// syndrome_kernel: calculate_syndrome_irregular (reference
// src/array_and_matrix_operations.cpp:476-486), a thread per check and frame.
// pack_kernel / unpack_kernel: 0/1 bytes <-> the packed uint64 key words the
// decoders and the key generators (keygen.hip) work on.
#include <hip/hip_runtime.h>

#include "qkd_decode.h"
#include "qkd_host.h"

namespace qkd {

// ---- syndrome ---------------------------------------------------------------
__global__ void syndrome_kernel(DeviceCode c, const uint8_t* bits, uint32_t n_frames, uint8_t* syn) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (size_t)n_frames * c.m) return;
    const size_t f = gid / c.m;
    const int j = (int)(gid - f * c.m);
    const int deg = c.chk_deg[j];
    int s = 0;
    for (int k = 0; k < deg; ++k) s ^= bits[f * c.n + c.chk_bits[k * c.m_pad + j]] & 1;
    syn[gid] = (uint8_t)s;
}

// ---- bit packing ------------------------------------------------------------
// One lane per 8 key bytes -> one packed byte (little-endian words, so the
// byte array is the uint64 word array); bits past n are 0. 8-byte loads when
// every frame row is 8-byte aligned (n % 8 == 0), byte loads otherwise.
__global__ void pack_kernel(const uint8_t* bytes0, const uint8_t* bytes1, uint32_t n, uint32_t words,
                            uint32_t n_frames, uint64_t* out0, uint64_t* out1, uint32_t wide) {
    // wide (the host's choice: n % 32 == 0 and both arrays 16-byte aligned): 32
    // key bytes -> 4 packed bytes per thread (two 16-byte loads); else one
    // packed byte per thread
    const uint8_t* bytes = blockIdx.y ? bytes1 : bytes0;
    uint64_t* out = blockIdx.y ? out1 : out0;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per_frame = (size_t)words * 8;
    if (wide) {
        const size_t per4 = per_frame / 4;            // 4-byte output groups per frame
        if (gid >= (size_t)n_frames * per4) return;
        const size_t f = gid / per4;
        const uint32_t b = (uint32_t)(gid - f * per4);   // output bytes 4b .. 4b+3
        uint32_t m = 0;
        if ((size_t)b * 32 < n) {
            const uint4* src = reinterpret_cast<const uint4*>(bytes + f * n + (size_t)b * 32);
            const uint4 v0 = src[0], v1 = src[1];
            const uint32_t w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t t = w[k] & 0x01010101u;            // byte q's LSB at bit 8q
                m |= ((t * 0x01020408u) >> 24 & 0xfu) << (4 * k); // byte q -> bit 24 + q
            }
        }
        reinterpret_cast<uint32_t*>(out)[gid] = m;
        return;
    }
    if (gid >= (size_t)n_frames * per_frame) return;
    const size_t f = gid / per_frame;
    const uint32_t b = (uint32_t)(gid - f * per_frame);
    const uint8_t* src = bytes + f * n;
    uint32_t m = 0;
    for (uint32_t k = 0; k < 8; ++k) {
        const uint32_t i = b * 8 + k;
        if (i < n) m |= (uint32_t)(src[i] & 1u) << k;
    }
    reinterpret_cast<uint8_t*>(out)[gid] = (uint8_t)m;
}

hipError_t launch_pack_keys(const DecodeArgs& a, hipStream_t stream) {
    const uint32_t n = (uint32_t)a.code.n;
    const size_t nw = (size_t)a.n_frames * a.words;
    // Alice's and Bob's keys in one launch (grid.y selects the key; the wide
    // form needs both arrays 16-byte aligned)
    const bool wide = (n % 32) == 0 &&
                      ((reinterpret_cast<uintptr_t>(a.alice_b) | reinterpret_cast<uintptr_t>(a.bob_b)) & 15u) == 0;
    const size_t threads = wide ? nw * 2 : nw * 8;
    if (!a.alice_b) {
        // Bob's key alone (qkd_reconcile_batch): one grid row, alice_w untouched
        hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((threads + 255) / 256), 1), dim3(256), 0, stream,
                           a.bob_b, a.bob_b, n, a.words, a.n_frames, const_cast<uint64_t*>(a.bob_w),
                           const_cast<uint64_t*>(a.bob_w), wide ? 1u : 0u);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((threads + 255) / 256), 2), dim3(256), 0, stream,
                       a.alice_b, a.bob_b, n, a.words, a.n_frames, const_cast<uint64_t*>(a.alice_w),
                       const_cast<uint64_t*>(a.bob_w), wide ? 1u : 0u);
    return hipGetLastError();
}

__global__ void unpack_kernel(const uint64_t* words_in, uint32_t n, uint32_t words, uint32_t n_frames,
                              uint8_t* out) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (size_t)n_frames * n) return;
    const size_t f = gid / n;
    const uint32_t i = (uint32_t)(gid - f * n);
    out[gid] = (uint8_t)((words_in[f * words + (i >> 6)] >> (i & 63)) & 1u);
}

}  // namespace qkd

using namespace qkd;

extern "C" {

qkd_status qkd_syndrome_batch(const qkd_code* c, const uint8_t* bits, size_t n_frames, uint8_t* syn,
                              void* stream) {
    clear_error();
    if (!c || !bits || !syn) return set_error(QKD_ERR_INVALID_ARG, "null argument");
    qkd_status s = check_frames(n_frames);
    if (s != QKD_OK) return s;
    DeviceGuard g(c->device);
    const size_t total = n_frames * (size_t)c->m;
    hipLaunchKernelGGL(syndrome_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       c->view(), bits, (uint32_t)n_frames, syn);
    QKD_HIP(hipGetLastError());
    return QKD_OK;
}

}  // extern "C"
