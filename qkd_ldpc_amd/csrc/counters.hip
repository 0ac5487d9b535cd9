// counters.hip — the batch reduction of a run's per-frame outputs into one
// qkd_counters record (reference src/simulation.cpp:252-312: exact integer
// sums, extrema), and the merge of several ranks' records.
#include <hip/hip_runtime.h>

#include "qkd_host.h"

namespace qkd {

// ---- batch reduction (simulation.cpp:252-312) ----------------------------------
__global__ void counters_kernel(const uint32_t* iters, const uint8_t* sp, const uint8_t* ko,
                                uint32_t n_frames, qkd_counters* out) {
    __shared__ unsigned long long s_sum[5];
    __shared__ uint32_t s_min, s_max;
    if (threadIdx.x < 5) s_sum[threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_min = 0xffffffffu; s_max = 0; }
    __syncthreads();
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n_frames) {
        atomicAdd(&s_sum[0], 1ull);
        if (sp[f]) {
            const unsigned long long it = iters[f];
            atomicAdd(&s_sum[1], 1ull);
            if (!ko || ko[f]) atomicAdd(&s_sum[2], 1ull);
            atomicAdd(&s_sum[3], it);
            atomicAdd(&s_sum[4], it * it);
            atomicMin(&s_min, (uint32_t)it);
            atomicMax(&s_max, (uint32_t)it);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd((unsigned long long*)&out->frames, s_sum[0]);
        atomicAdd((unsigned long long*)&out->sp_ok, s_sum[1]);
        atomicAdd((unsigned long long*)&out->ldpc_ok, s_sum[2]);
        atomicAdd((unsigned long long*)&out->sum_iters, s_sum[3]);
        atomicAdd((unsigned long long*)&out->sum_iters_sq, s_sum[4]);
        atomicMin(&out->min_iters, s_min);
        atomicMax(&out->max_iters, s_max);
    }
}

// One workgroup over every frame (batches up to kCountersOneBlock frames): the
// reduction and the record's initialisation in one launch.
constexpr uint32_t kCountersOneBlock = 1u << 16;
__global__ __launch_bounds__(1024) void counters_one_kernel(const uint32_t* iters, const uint8_t* sp,
                                                            const uint8_t* ko, uint32_t n_frames,
                                                            qkd_counters* out) {
    __shared__ unsigned long long s_sum[5];
    __shared__ uint32_t s_min, s_max;
    if (threadIdx.x < 5) s_sum[threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_min = 0xffffffffu; s_max = 0; }
    __syncthreads();
    unsigned long long c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    uint32_t mn = 0xffffffffu, mx = 0;
    // (every load unconditional and kCntBatch frames' loads issued together:
    // a load behind the sp[f] branch made each frame two dependent round trips)
    constexpr uint32_t kCntBatch = 4;
    for (uint32_t f0 = threadIdx.x; f0 < n_frames; f0 += kCntBatch * blockDim.x) {
        uint32_t itv[kCntBatch];
        uint8_t spv[kCntBatch], kov[kCntBatch];
#pragma unroll
        for (uint32_t u = 0; u < kCntBatch; ++u) {
            const uint32_t f = f0 + u * blockDim.x;
            const bool in = f < n_frames;
            itv[u] = in ? iters[f] : 0u;
            spv[u] = in ? sp[f] : (uint8_t)0;
            kov[u] = (in && ko) ? ko[f] : (uint8_t)1;
        }
#pragma unroll
        for (uint32_t u = 0; u < kCntBatch; ++u) {
            if (spv[u]) {
                const unsigned long long it = itv[u];
                c1++;
                if (kov[u]) c2++;
                c3 += it;
                c4 += it * it;
                mn = min(mn, (uint32_t)it);
                mx = max(mx, (uint32_t)it);
            }
        }
    }
    // wave reductions first: one LDS atomic per wave and quantity
    for (int o = 32; o > 0; o >>= 1) {
        c1 += __shfl_xor(c1, o);
        c2 += __shfl_xor(c2, o);
        c3 += __shfl_xor(c3, o);
        c4 += __shfl_xor(c4, o);
        mn = min(mn, (uint32_t)__shfl_xor((int)mn, o));
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_sum[1], c1);
        atomicAdd(&s_sum[2], c2);
        atomicAdd(&s_sum[3], c3);
        atomicAdd(&s_sum[4], c4);
        atomicMin(&s_min, mn);
        atomicMax(&s_max, mx);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out->frames = n_frames;
        out->sp_ok = s_sum[1];
        out->ldpc_ok = s_sum[2];
        out->sum_iters = s_sum[3];
        out->sum_iters_sq = s_sum[4];
        out->min_iters = s_min;
        out->max_iters = s_max;
    }
}

__global__ void counters_init_kernel(qkd_counters* c) {
    c->frames = c->sp_ok = c->ldpc_ok = c->sum_iters = c->sum_iters_sq = 0;
    c->min_iters = 0xffffffffu;
    c->max_iters = 0;
}

// counters <- the reduction of F frames' outputs (one launch up to kCountersOneBlock)
hipError_t launch_counters(const uint32_t* iters, const uint8_t* sp, const uint8_t* ko, size_t n_frames,
                           qkd_counters* c, hipStream_t stream) {
    if (n_frames <= kCountersOneBlock) {
        hipLaunchKernelGGL(counters_one_kernel, dim3(1), dim3(1024), 0, stream, iters, sp, ko, (uint32_t)n_frames, c);
    } else {
        hipLaunchKernelGGL(counters_init_kernel, dim3(1), dim3(1), 0, stream, c);
        hipLaunchKernelGGL(counters_kernel, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, stream, iters, sp,
                           ko, (uint32_t)n_frames, c);
    }
    return hipGetLastError();
}

// The records of n ranks (one all-gather, qkd_ldpc_amd/dist.py) combined as the
// reference's one-process reduction would see all their frames
// (simulation.cpp:252-312): sums add, extrema take min / max. One wave; every
// record is read before `out` is written, so `out` may alias any of them.
__global__ __launch_bounds__(64) void counters_merge_kernel(const qkd_counters* recs, uint32_t n,
                                                            qkd_counters* out) {
    unsigned long long s[5] = {0, 0, 0, 0, 0};
    uint32_t mn = 0xffffffffu, mx = 0;
    for (uint32_t r = threadIdx.x; r < n; r += 64) {
        const qkd_counters c = recs[r];
        s[0] += c.frames;
        s[1] += c.sp_ok;
        s[2] += c.ldpc_ok;
        s[3] += c.sum_iters;
        s[4] += c.sum_iters_sq;
        mn = min(mn, c.min_iters);
        mx = max(mx, c.max_iters);
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] += __shfl_xor(s[k], o);
        mn = min(mn, (uint32_t)__shfl_xor((int)mn, o));
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out->frames = s[0];
        out->sp_ok = s[1];
        out->ldpc_ok = s[2];
        out->sum_iters = s[3];
        out->sum_iters_sq = s[4];
        out->min_iters = mn;
        out->max_iters = mx;
    }
}

}  // namespace qkd

using namespace qkd;

extern "C" {

qkd_status qkd_counters_batch(const uint32_t* iterations, const uint8_t* syndromes_match,
                              const uint8_t* keys_match, size_t n_frames, qkd_counters* counters,
                              int device, void* stream) {
    clear_error();
    if (!iterations || !syndromes_match || !counters) return set_error(QKD_ERR_INVALID_ARG, "null argument");
    qkd_status s = check_frames(n_frames);
    if (s != QKD_OK) return s;
    DeviceGuard g(device);
    QKD_HIP(launch_counters(iterations, syndromes_match, keys_match, n_frames, counters, (hipStream_t)stream));
    return QKD_OK;
}

qkd_status qkd_counters_merge(const qkd_counters* records, size_t n_records, qkd_counters* out, int device,
                              void* stream) {
    clear_error();
    if (!records || !out) return set_error(QKD_ERR_INVALID_ARG, "null argument");
    if (n_records == 0 || n_records > 0xffffffffu) return set_error(QKD_ERR_INVALID_ARG, "bad record count");
    DeviceGuard g(device);
    hipLaunchKernelGGL(counters_merge_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, records,
                       (uint32_t)n_records, out);
    QKD_HIP(hipGetLastError());
    return QKD_OK;
}

}  // extern "C"
