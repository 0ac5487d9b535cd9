// adapt.hip — rate adaptation of one mother code by puncturing and shortening
// (Elkouss et al.): the plan object (qkd_adapt), the kernels that place a
// payload in a frame and take it out again, and the class bytes the decoder of
// qkd_reconcile_adaptive_batch reads instead of per-bit LLRs, and the round
// kernels of qkd_reconcile_blind_batch (revealed punctured bits, per frame).
//
// A frame of N bits holds n_payload = N - p - s key bits (payload bit k at the
// k-th position, ascending, that is neither punctured nor shortened), p
// punctured bits (Alice's private random bits, never sent: Bob's LLR is 0) and
// s shortened bits (0 on both sides: Bob's LLR is +known).
#include <algorithm>
#include <new>
#include <vector>

#include "qkd_decode.h"
#include "qkd_internal.h"

namespace qkd {

constexpr int kAdaptBlock = 256;

// cls[f * n + i] from the map src (in whichever bit order the decoder reads)
__global__ __launch_bounds__(kAdaptBlock) void adapt_class_kernel(const int32_t* __restrict__ src,
                                                                  const uint8_t* __restrict__ payload, uint32_t n,
                                                                  uint32_t n_payload, uint8_t* __restrict__ cls) {
    const uint32_t i = blockIdx.x * kAdaptBlock + threadIdx.x;
    const size_t f = blockIdx.y;
    if (i >= n) return;
    const int32_t k = src[i];
    uint8_t v;
    if (k >= 0) v = payload[f * n_payload + (uint32_t)k] & 1u;
    else v = k == kSrcPunctured ? 2u : 3u;
    cls[f * n + i] = v;
}

// qkd_reconcile_blind_batch: the same for frame f = list[blockIdx.y] of the
// round's open frames, with the punctured bits Alice has revealed so far as
// known bits: rank[i] = j is position i's index in the plan's punctured list
// (-1 elsewhere), and the position is class 4 | value when j < min(nrev[f], p).
// revealed[f * p + j] is read for those j only: Bob has no later byte yet.
__global__ __launch_bounds__(kAdaptBlock) void blind_class_kernel(const int32_t* __restrict__ src,
                                                                  const int32_t* __restrict__ rank,
                                                                  const uint8_t* __restrict__ payload,
                                                                  const uint8_t* __restrict__ revealed,
                                                                  const uint32_t* __restrict__ nrev,
                                                                  const uint32_t* __restrict__ list,
                                                                  const uint32_t* __restrict__ count, uint32_t y0,
                                                                  uint32_t n, uint32_t n_payload, uint32_t p,
                                                                  uint8_t* __restrict__ cls) {
    const uint32_t k = y0 + blockIdx.y;
    if (k >= *count) return;
    const uint32_t i = blockIdx.x * kAdaptBlock + threadIdx.x;
    if (i >= n) return;
    const size_t f = list[k];
    const int32_t s = src[i];
    uint8_t v;
    if (s >= 0) {
        v = payload[f * n_payload + (uint32_t)s] & 1u;
    } else if (s == kSrcPunctured) {
        const uint32_t nr = nrev[f] < p ? nrev[f] : p;
        const uint32_t j = (uint32_t)rank[i];
        v = j < nr ? (uint8_t)(4u | (revealed[f * p + j] & 1u)) : (uint8_t)2u;
    } else {
        v = 3u;
    }
    cls[f * n + i] = v;
}

// One round's bookkeeping of qkd_reconcile_blind_batch (BlindRound), one
// workgroup. Round 0 opens every frame that is not skipped (n_revealed past p
// counts as p, rounds = 0). A later round first settles the frames the round
// before decoded: a frame that matched (with Alice's tags given,
// qkd_reconcile_blind_verify_batch: one that is verified) is closed, so is one
// that failed with nothing left to reveal; any other gets step more bits, up to
// p. Then the open frames go to list in ascending order (rounds[f] counts the
// rounds that decode f) and *count says how many.
constexpr int kBlindBlock = 1024;
__global__ __launch_bounds__(kBlindBlock) void blind_round_kernel(BlindRound r) {
    __shared__ uint32_t wave_n[kBlindBlock / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t total = 0;
    for (uint32_t f0 = 0; f0 < r.n_frames; f0 += kBlindBlock) {       // (uniform trip count)
        const uint32_t f = f0 + tid;
        bool open = false;
        if (f < r.n_frames) {
            if (r.round == 0) {
                open = !(r.skip && r.skip[f] != 0);
                if (open) {
                    if (r.n_revealed[f] > r.p) r.n_revealed[f] = r.p;
                    if (r.rounds) r.rounds[f] = 0;
                }
            } else if (r.open[f]) {
                const uint32_t nr = r.n_revealed[f];
                // (closed: verified when Alice's tags were given, else matched)
                const uint8_t closed = r.verified ? r.verified[f] : r.sp_ok[f];
                open = closed == 0 && nr < r.p;
                if (open) r.n_revealed[f] = r.step >= r.p - nr ? r.p : nr + r.step;
            }
            r.open[f] = open ? 1 : 0;
        }
        const uint64_t b = __ballot(open);
        if (lane == 0) wave_n[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < kBlindBlock / 64; ++w) {
            const uint32_t c = wave_n[w];
            before += w < wave ? c : 0u;
            all += c;
        }
        if (open) {
            r.list[total + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = f;
            if (r.rounds) r.rounds[f] += 1;
        }
        total += all;
        __syncthreads();
    }
    if (tid == 0) *r.count = total;
}

// frames[f * n + i] from the embedding map (qkd_adapt::d_emb)
__global__ __launch_bounds__(kAdaptBlock) void adapt_embed_kernel(const int32_t* __restrict__ emb,
                                                                  const uint8_t* __restrict__ payload,
                                                                  const uint8_t* __restrict__ fill, uint32_t n,
                                                                  uint32_t n_payload, uint32_t p,
                                                                  uint8_t* __restrict__ frames) {
    const uint32_t i = blockIdx.x * kAdaptBlock + threadIdx.x;
    const size_t f = blockIdx.y;
    if (i >= n) return;
    const int32_t k = emb[i];
    uint8_t v = 0;                                      // a shortened bit
    if (k >= 0) v = payload[f * n_payload + (uint32_t)k] & 1u;
    else if (k <= -2) v = fill[f * p + (uint32_t)(-2 - k)] & 1u;
    frames[f * n + i] = v;
}

// payload[f * n_payload + src[i]] = frames[f * n + i] & 1 for the payload bits
__global__ __launch_bounds__(kAdaptBlock) void adapt_extract_kernel(const int32_t* __restrict__ src,
                                                                    const uint8_t* __restrict__ frames, uint32_t n,
                                                                    uint32_t n_payload, uint8_t* __restrict__ payload) {
    const uint32_t i = blockIdx.x * kAdaptBlock + threadIdx.x;
    const size_t f = blockIdx.y;
    if (i >= n) return;
    const int32_t k = src[i];
    if (k >= 0) payload[f * n_payload + (uint32_t)k] = frames[f * n + i] & 1u;
}

// (grid y: at most 65535 frames per launch)
constexpr size_t kAdaptFramesPerLaunch = 65535;

hipError_t launch_adapt_classes(const int32_t* src, const uint8_t* payload, uint32_t n, uint32_t n_payload,
                                uint32_t n_frames, uint8_t* cls, hipStream_t stream) {
    for (size_t f0 = 0; f0 < n_frames; f0 += kAdaptFramesPerLaunch) {
        const size_t nf = std::min(kAdaptFramesPerLaunch, (size_t)n_frames - f0);
        hipLaunchKernelGGL(adapt_class_kernel, dim3((n + kAdaptBlock - 1) / kAdaptBlock, (unsigned)nf),
                           dim3(kAdaptBlock), 0, stream, src, payload + f0 * n_payload, n, n_payload, cls + f0 * n);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_blind_classes(const int32_t* src, const int32_t* rank, const uint8_t* payload, const BlindArgs& b,
                                uint32_t n, uint32_t n_payload, uint32_t n_frames, uint8_t* cls, hipStream_t stream) {
    for (size_t f0 = 0; f0 < n_frames; f0 += kAdaptFramesPerLaunch) {
        const size_t nf = std::min(kAdaptFramesPerLaunch, (size_t)n_frames - f0);
        hipLaunchKernelGGL(blind_class_kernel, dim3((n + kAdaptBlock - 1) / kAdaptBlock, (unsigned)nf),
                           dim3(kAdaptBlock), 0, stream, src, rank, payload, b.revealed, b.n_revealed, b.list, b.count,
                           (uint32_t)f0, n, n_payload, b.p, cls);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_blind_round(const BlindRound& r, hipStream_t stream) {
    hipLaunchKernelGGL(blind_round_kernel, dim3(1), dim3(kBlindBlock), 0, stream, r);
    return hipGetLastError();
}

// The seeded key string of the verification hash, word k per thread
// (qkd_verify.h: counter form, so no word depends on another).
__global__ __launch_bounds__(kAdaptBlock) void verify_expand_kernel(uint64_t seed, uint32_t words,
                                                                    uint64_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * kAdaptBlock + threadIdx.x;
    if (k < words) out[k] = qkdv::verify_key_word(seed, k);
}

hipError_t launch_verify_expand(uint64_t seed, uint32_t words, uint64_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(verify_expand_kernel, dim3((words + kAdaptBlock - 1) / kAdaptBlock), dim3(kAdaptBlock), 0,
                       stream, seed, words, out);
    return hipGetLastError();
}

static qkd_status adapt_build(qkd_adapt* a, const qkd_code* c, const int32_t* punctured, int32_t p,
                              const int32_t* shortened, int32_t s) {
    const int32_t n = c->n;
    if (p < 0 || s < 0 || (p > 0 && !punctured) || (s > 0 && !shortened))
        return set_error(QKD_ERR_INVALID_ARG, "qkd_adapt_create: bad position lists");
    if ((int64_t)p + s >= n) return set_error(QKD_ERR_INVALID_ARG, "qkd_adapt_create: no payload bit left (p + s >= N)");
    // emb as in qkd_adapt; every position starts as payload
    std::vector<int32_t> emb(n, 0);
    for (int32_t r = 0; r < p + s; ++r) {
        const int32_t pos = r < p ? punctured[r] : shortened[r - p];
        if (pos < 0 || pos >= n)
            return set_error(QKD_ERR_INVALID_ARG, "qkd_adapt_create: position %d out of range [0,%d)", pos, n);
        if (emb[pos] != 0) return set_error(QKD_ERR_INVALID_ARG, "qkd_adapt_create: position %d given twice", pos);
        emb[pos] = r < p ? -2 - r : -1;
    }
    std::vector<int32_t> src(n), src_int(n), rank(n, -1), rank_int(n);
    for (int32_t r = 0; r < p; ++r) rank[punctured[r]] = r;
    int32_t k = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (emb[i] == 0) emb[i] = k++;
        src[i] = emb[i] >= 0 ? emb[i] : (emb[i] == -1 ? kSrcShortened : kSrcPunctured);
    }
    a->code = c;
    a->device = c->device;
    a->n = n;
    a->n_payload = n - p - s;
    a->p = p;
    a->s = s;
    // (a code too long for the split kernels has no internal order: the status
    // the device-to-host copy of its null perm used to give)
    const std::vector<int32_t>& perm = c->perm;
    if (perm.size() != (size_t)n)
        return set_error(QKD_ERR_DEVICE, "qkd_adapt_create: the code has no internal bit order (N=%d)", n);
    for (int32_t q = 0; q < n; ++q) {
        src_int[q] = src[perm[q]];
        rank_int[q] = rank[perm[q]];
    }
    DeviceGuard g(c->device);
    QKD_HIP(a->d_rank_orig.upload(rank));
    QKD_HIP(a->d_rank_int.upload(rank_int));
    QKD_HIP(a->d_src_orig.upload(src));
    QKD_HIP(a->d_src_int.upload(src_int));
    QKD_HIP(a->d_emb.upload(emb));
    return QKD_OK;
}

static qkd_status adapt_frames_check(const qkd_adapt* a, const void* in, const void* out, size_t n_frames) {
    if (!a || !in || !out) return set_error(QKD_ERR_INVALID_ARG, "null argument");
    if (n_frames == 0) return set_error(QKD_ERR_INVALID_ARG, "n_frames must be > 0");
    if (n_frames > 0xffffffffull) return set_error(QKD_ERR_INVALID_ARG, "n_frames too large");
    return QKD_OK;
}

}  // namespace qkd

using namespace qkd;

extern "C" {

qkd_adapt* qkd_adapt_create(const qkd_code* code, const int32_t* punctured, int32_t p, const int32_t* shortened,
                            int32_t s, qkd_status* status) {
    clear_error();
    qkd_status st = QKD_OK;
    qkd_adapt* a = nullptr;
    if (!code) {
        st = set_error(QKD_ERR_INVALID_ARG, "null code");
    } else if (!(a = new (std::nothrow) qkd_adapt())) {
        st = set_error(QKD_ERR_OUT_OF_MEMORY, "out of host memory");
    } else {
        a->device = code->device;
        st = adapt_build(a, code, punctured, p, shortened, s);
        if (st != QKD_OK) {
            delete a;
            a = nullptr;
        }
    }
    if (status) *status = st;
    return a;
}

void qkd_adapt_destroy(qkd_adapt* a) { delete a; }

qkd_status qkd_adapt_get_info(const qkd_adapt* a, qkd_adapt_info* info) {
    if (!a || !info) return set_error(QKD_ERR_INVALID_ARG, "null argument");
    info->n_bits = a->n;
    info->n_payload = a->n_payload;
    info->n_punctured = a->p;
    info->n_shortened = a->s;
    return QKD_OK;
}

qkd_status qkd_adapt_embed_batch(const qkd_adapt* a, const uint8_t* payload, size_t n_frames, const uint8_t* fill,
                                 uint8_t* frames, void* stream) {
    clear_error();
    qkd_status s = adapt_frames_check(a, payload, frames, n_frames);
    if (s != QKD_OK) return s;
    if ((a->p > 0) != (fill != nullptr))
        return set_error(QKD_ERR_INVALID_ARG, "fill is required exactly when the plan punctures");
    DeviceGuard g(a->device);
    const uint32_t n = (uint32_t)a->n;
    for (size_t f0 = 0; f0 < n_frames; f0 += kAdaptFramesPerLaunch) {
        const size_t nf = std::min(kAdaptFramesPerLaunch, n_frames - f0);
        hipLaunchKernelGGL(adapt_embed_kernel, dim3((n + kAdaptBlock - 1) / kAdaptBlock, (unsigned)nf),
                           dim3(kAdaptBlock), 0, (hipStream_t)stream, a->d_emb, payload + f0 * (size_t)a->n_payload,
                           fill ? fill + f0 * (size_t)a->p : nullptr, n, (uint32_t)a->n_payload, (uint32_t)a->p,
                           frames + f0 * n);
        QKD_HIP(hipGetLastError());
    }
    return QKD_OK;
}

qkd_status qkd_adapt_extract_batch(const qkd_adapt* a, const uint8_t* frames, size_t n_frames, uint8_t* payload,
                                   void* stream) {
    clear_error();
    qkd_status s = adapt_frames_check(a, frames, payload, n_frames);
    if (s != QKD_OK) return s;
    DeviceGuard g(a->device);
    const uint32_t n = (uint32_t)a->n;
    for (size_t f0 = 0; f0 < n_frames; f0 += kAdaptFramesPerLaunch) {
        const size_t nf = std::min(kAdaptFramesPerLaunch, n_frames - f0);
        hipLaunchKernelGGL(adapt_extract_kernel, dim3((n + kAdaptBlock - 1) / kAdaptBlock, (unsigned)nf),
                           dim3(kAdaptBlock), 0, (hipStream_t)stream, a->d_src_orig, frames + f0 * n, n,
                           (uint32_t)a->n_payload, payload + f0 * (size_t)a->n_payload);
        QKD_HIP(hipGetLastError());
    }
    return QKD_OK;
}

}  // extern "C"
