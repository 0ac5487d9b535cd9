// debug.hip — the qkd_debug_* entries: the device math of qkd_math.h and
// qkd_spec.h evaluated point by point (math_kernel; the bit-exactness tests
// against the reference's glibc tanh / atanh, qkd_ldpc_algorithm.cpp:224,
// :239-249), the exhaustive phi-bound sweep, and the read-outs of a
// workspace's diagnostic state (replays, check-lane form, decoder timing,
// phase clocks).
#include <hip/hip_runtime.h>

#include "qkd_decode.h"
#include "qkd_host.h"

using namespace qkd;

extern "C" {

__global__ void math_kernel(int which, const double* x, double* y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    switch (which) {
        case 0: y[i] = qkdm::tanh_flat(x[i]); break;
        case 1: y[i] = qkdm::atanh_flat(x[i]); break;
        case 2: y[i] = (double)RuleMath<kRuleSp32>::tanh_half((float)x[i]); break;   // signed psi(|x|)
        case 4:
        case 5: {
            // phi bounds over [x[2k], x[2k+1]] -> y[2k] = lo, y[2k+1] = hi
            // (4: qkds::phi_bounds, 5: qkds::phi_bounds_out); one thread per pair
            // phi_bounds gives psi = phi / ln 2 (returned scaled back to phi in
            // binary64); phi_bounds_out takes psi-unit sums (x = S / ln 2)
            if (i & 1) break;
            float lo, hi;
            if (which == 4) {
                qkds::phi_bounds((float)x[i], (float)x[i + 1], lo, hi);
                y[i] = (double)lo * 0.6931471805599453;
                y[i + 1] = (double)hi * 0.6931471805599453;
            } else {
                qkds::phi_bounds_out((float)x[i], (float)x[i + 1], lo, hi);
                y[i] = lo;
                y[i + 1] = hi;
            }
            break;
        }
        case 8:
        case 9: {
            // quadruples (a, b, s_lo, s_hi) -> (in lo, in hi, out lo, out hi),
            // raw binary32 results: 8 the packed qkds::phi_pair, 9 the scalar
            // phi_bounds (psi units) and phi_bounds_out; one thread per quadruple
            if (i & 3) break;
            qkds::f2 in, out;
            if (which == 8) {
                qkds::phi_pair((float)x[i], (float)x[i + 1], (float)x[i + 2], (float)x[i + 3], in, out);
            } else {
                in = qkds::phi_bounds((float)x[i], (float)x[i + 1]);
                out = qkds::phi_bounds_out((float)x[i + 2], (float)x[i + 3]);
            }
            y[i] = in.x;
            y[i + 1] = in.y;
            y[i + 2] = out.x;
            y[i + 3] = out.y;
            break;
        }
        case 10:
        case 11: {
            // pairs of exact b2c (x[2k], x[2k+1]) -> the raw psi slots (low
            // word: lo with the sign of b2c in bit 31, high word: hi; NaN in
            // both: sign not certain): 10 the packed qkds::psi_of_exact2, 11
            // the scalar psi_of_exact twice; one thread per pair
            if (i & 1) break;
            qkds::f2 r0, r1;
            if (which == 10) {
                qkds::psi_of_exact2(x[i], x[i + 1], r0, r1);
            } else {
                r0 = qkds::psi_of_exact(x[i]);
                r1 = qkds::psi_of_exact(x[i + 1]);
            }
            y[i] = __builtin_bit_cast(double, r0);
            y[i + 1] = __builtin_bit_cast(double, r1);
            break;
        }
        case 12:
        case 13: {
            // pairs (x, S) -> (|tanh_half(x)|, two_atanh(S)) of the binary32 rule:
            // 12 the packed RuleMath<kRuleSp32>::pair, 13 the scalar forms
            if (i & 1) break;
            qkds::f2 r;
            if (which == 12) {
                r = RuleMath<kRuleSp32>::pair((float)x[i], (float)x[i + 1]);
            } else {
                r = qkds::f2{__builtin_fabsf(RuleMath<kRuleSp32>::tanh_half((float)x[i])),
                             RuleMath<kRuleSp32>::two_atanh((float)x[i + 1])};
            }
            y[i] = r.x;
            y[i + 1] = r.y;
            break;
        }
        case 14:
        case 15:
        case 16:
        case 17: {
            // quadruples (a lo, a hi, b lo, b hi) -> the bounds of both
            // intervals: 14 the packed phi_bounds2, 15 two scalar phi_bounds
            // (the interleaved decoder's input form); 16 the packed
            // phi_bounds_out2, 17 two scalar phi_bounds_out (its output form)
            if (i & 3) break;
            const qkds::f2 u{(float)x[i], (float)x[i + 1]}, v{(float)x[i + 2], (float)x[i + 3]};
            qkds::f2 ru, rv;
            if (which == 14) qkds::phi_bounds2(u, v, ru, rv);
            else if (which == 16) qkds::phi_bounds_out2(u, v, ru, rv);
            else if (which == 15) { ru = qkds::phi_bounds(u.x, u.y); rv = qkds::phi_bounds(v.x, v.y); }
            else { ru = qkds::phi_bounds_out(u.x, u.y); rv = qkds::phi_bounds_out(v.x, v.y); }
            y[i] = ru.x;
            y[i + 1] = ru.y;
            y[i + 2] = rv.x;
            y[i + 3] = rv.y;
            break;
        }
        case 6: y[i] = (double)__builtin_amdgcn_exp2f((float)x[i]); break;   // hardware v_exp_f32
        case 7: y[i] = (double)__builtin_amdgcn_logf((float)x[i]); break;    // hardware v_log_f32
        default: y[i] = (double)RuleMath<kRuleSp32>::two_atanh((float)x[i]); break;  // phi(S ln 2)
    }
}

qkd_status qkd_debug_math(int which, const double* x, double* y, size_t n, void* stream) {
    clear_error();
    if (!x || !y || which < 0 || which > 17) return set_error(QKD_ERR_INVALID_ARG, "bad argument");
    if (which >= 14 && (n & 3)) return set_error(QKD_ERR_INVALID_ARG, "packed phi bounds take quadruples");
    if ((which == 10 || which == 11) && (n & 1)) return set_error(QKD_ERR_INVALID_ARG, "psi pairs take n even");
    if ((which == 12 || which == 13) && (n & 1)) return set_error(QKD_ERR_INVALID_ARG, "rule pairs take n even");
    if ((which == 4 || which == 5) && (n & 1)) return set_error(QKD_ERR_INVALID_ARG, "phi bounds take pairs (n even)");
    if ((which == 8 || which == 9) && (n & 3))
        return set_error(QKD_ERR_INVALID_ARG, "paired phi bounds take quadruples (n % 4 == 0)");
    if (n == 0) return QKD_OK;
    hipLaunchKernelGGL(math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, which,
                       x, y, n);
    QKD_HIP(hipGetLastError());
    return QKD_OK;
}

// Exhaustive phi-bound sweep (qkd_debug_phi_sweep): one binary32 point per
// (thread, step), binary64 phi and |phi'| from OCML's exp / expm1 / log1p
// (about 1 ulp of binary64, 2^-32 of the 2^-20 allowance).
__device__ __forceinline__ void sweep_max(float v, uint32_t bits, uint32_t* mx, uint32_t* at) {
    const uint32_t b = __builtin_bit_cast(uint32_t, v);
    if (b > atomicMax(mx, b)) atomicExch(at, bits);
}

__global__ void phi_sweep_kernel(int which, uint32_t first, uint32_t last, unsigned long long* cnt,
                                 uint32_t* mx) {
    const uint32_t stride = gridDim.x * blockDim.x;
    unsigned long long pts = 0, bad_hi = 0, bad_lo = 0, bad_sl = 0;
    float e_max = 0.0f, s_max = 0.0f;
    uint32_t e_at = 0, s_at = 0;
    constexpr double R = 0x1.0p-20;
    for (uint64_t k = (uint64_t)first + blockIdx.x * blockDim.x + threadIdx.x; k <= last; k += stride) {
        const uint32_t bits = (uint32_t)k;
        const float a = __builtin_bit_cast(float, bits);
        double S, v, lo, hi, sl;       // S in nep units; v, lo, hi in the form's output units
        if (which == 4) {
            const float a1 = __builtin_amdgcn_fmed3f(a, 0.0f, qkds::kPhiHuge);
            const qkds::PhiVal e = qkds::phi_core<true, false>(a1, qkds::exp_neg(a1), __builtin_amdgcn_logf(a1));
            const qkds::f2 b = qkds::phi_bounds(a, a);
            S = a1;
            v = e.v * 0.6931471805599453;         // psi -> phi
            lo = b.x * 0.6931471805599453;
            hi = b.y * 0.6931471805599453;
            sl = e.slope;
        } else {
            const float at = __builtin_fminf(a, qkds::kPsiHuge);
            const qkds::PhiVal e = qkds::phi_core<false, true>(at * qkds::kLn2, __builtin_amdgcn_exp2f(-at),
                                                               __builtin_amdgcn_logf(at));
            const qkds::f2 b = qkds::phi_bounds_out(a, a);
            S = (double)at * 0.6931471805599453;
            v = e.v;
            lo = b.x;
            hi = b.y;
            sl = e.slope;
        }
        const double u = exp(-S), w = -expm1(-S);                    // e^-S, 1 - e^-S
        const double phi = log1p(2.0 * u / w);                       // -ln tanh(S / 2)
        const double dphi = 2.0 * u / (w * (1.0 + u));               // 1 / sinh(S)
        ++pts;
        bad_hi += hi < phi;
        bad_lo += lo > phi;
        bad_sl += sl * (1.0 + R) < dphi;
        // evaluation-error statistics over normal arguments (a subnormal a gives
        // rcp overflow and an infinite upper bound: sound, counted above)
        if (phi > 1e-30 && bits >= 0x00800000u && v < 3.0e38) {
            const float err = (float)(fabs(v / phi - 1.0) / R);
            if (err > e_max) { e_max = err; e_at = bits; }
        }
        const float sr = (float)(dphi / sl);
        if (sr > s_max && bits >= 0x00800000u) { s_max = sr; s_at = bits; }
    }
    atomicAdd(&cnt[0], pts);
    if (bad_hi) atomicAdd(&cnt[1], bad_hi);
    if (bad_lo) atomicAdd(&cnt[2], bad_lo);
    if (bad_sl) atomicAdd(&cnt[3], bad_sl);
    sweep_max(e_max, e_at, &mx[0], &mx[2]);
    sweep_max(s_max, s_at, &mx[1], &mx[3]);
}

qkd_status qkd_debug_phi_sweep(int which, uint32_t first_bits, uint32_t last_bits, uint64_t* result) {
    clear_error();
    if ((which != 4 && which != 5) || !result || first_bits > last_bits || last_bits >= 0x7f800000u)
        return set_error(QKD_ERR_INVALID_ARG, "bad argument");
    DevBuf<unsigned long long> d_cnt;
    DevBuf<uint32_t> d_mx;
    QKD_HIP(d_cnt.alloc(4));
    if (d_mx.alloc(4) != hipSuccess) return set_error(QKD_ERR_OUT_OF_MEMORY, "phi sweep: cannot allocate");
    hipError_t e = hipMemset(d_cnt, 0, 4 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(d_mx, 0, 4 * sizeof(uint32_t));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(phi_sweep_kernel, dim3(4096), dim3(256), 0, nullptr, which, first_bits, last_bits, d_cnt.get(),
                           d_mx.get());
        e = hipGetLastError();
    }
    unsigned long long cnt[4] = {0, 0, 0, 0};
    uint32_t mx[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(mx, d_mx, sizeof mx, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return set_error(QKD_ERR_DEVICE, "phi sweep: %s", hipGetErrorString(e));
    for (int k = 0; k < 4; ++k) result[k] = cnt[k];
    for (int k = 0; k < 4; ++k) result[4 + k] = mx[k];
    return QKD_OK;
}

qkd_status qkd_debug_spec_replays(qkd_workspace* ws, uint64_t* replays, int reset) {
    if (!ws || !replays) return set_error(QKD_ERR_INVALID_ARG, "null argument");
    *replays = 0;
    if (!ws->counter) return QKD_OK;
    DeviceGuard g(ws->device);
    QKD_HIP(hipDeviceSynchronize());
    char* p = reinterpret_cast<char*>(ws->counter.get()) + 120;
    QKD_HIP(hipMemcpy(replays, p, 8, hipMemcpyDeviceToHost));
    if (reset) QKD_HIP(hipMemset(p, 0, 8));
    return QKD_OK;
}

qkd_status qkd_debug_check_lanes(qkd_workspace* ws, int32_t* form, int32_t* lane_tasks, int32_t* edge_tasks) {
    if (!ws) return set_error(QKD_ERR_INVALID_ARG, "null workspace");
    if (form) *form = ws->last_cl_form;
    if (lane_tasks) *lane_tasks = ws->last_cl_tasks;
    if (edge_tasks) *edge_tasks = ws->last_cl_rem_tasks;
    return QKD_OK;
}

qkd_status qkd_debug_decoder_timing(qkd_workspace* ws, int start, double* ms_total, uint64_t* launches) {
    if (!ws) return set_error(QKD_ERR_INVALID_ARG, "null workspace");
    DeviceGuard g(ws->device);
    std::lock_guard<std::mutex> lk(ws->mu);
    if (!start) QKD_HIP(decoder_events_fold(ws));
    if (ms_total) *ms_total = start ? 0.0 : ws->dec_ms_folded;
    if (launches) *launches = start ? 0 : ws->dec_pairs_folded;
    ws->dec_ev_used = 0;
    ws->dec_ms_folded = 0.0;
    ws->dec_pairs_folded = 0;
    ws->time_decoder = start != 0;
    return QKD_OK;
}

qkd_status qkd_debug_phase_cycles(qkd_workspace* ws, uint64_t* cycles7) {
    if (!ws || !cycles7) return set_error(QKD_ERR_INVALID_ARG, "null argument");
    if (!ws->counter) return set_error(QKD_ERR_INVALID_ARG, "workspace has not decoded yet");
    DeviceGuard g(ws->device);
    QKD_HIP(hipDeviceSynchronize());
    QKD_HIP(hipMemcpy(cycles7, reinterpret_cast<char*>(ws->counter.get()) + 64, 56, hipMemcpyDeviceToHost));
    return QKD_OK;
}

}  // extern "C"
