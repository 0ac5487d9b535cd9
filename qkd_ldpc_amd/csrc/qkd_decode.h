// qkd_decode.h — device-side pieces shared by the decode kernels (decode.hip:
// the classic message store; decode_split.hip: the LDS/global split store):
// launch arguments, LDS helpers, wave-plan words, the per-edge check rule and
// the second-iteration table. Compiled with -ffp-contract=off (qkd_math.h).
#pragma once
#include <hip/hip_runtime.h>

#include "qkd_internal.h"
#include "qkd_math.h"
#include "qkd_plan.h"
#include "qkd_spec.h"
#include "qkd_verify.h"

namespace qkd {


// Speculative interval iterations per frame before the exact fallback
// (decode_split.hip; QKD_SPEC_CAP overrides).
constexpr int kSpecCapDefault = 8;
constexpr int kCkptUnsatDefault = 128;    // checkpointed speculation trigger (unsatisfied checks)
// across calls: a QBER whose speculative call replayed more than this fraction
// of its frames switches to the checkpointed speculation (decode_keys)
constexpr double kSpecCkptSwitch = 1.0 / 16.0;
// Replay fraction above which speculation stops: within a launch for the
// frames still to start (decode_split.hip), across calls for that QBER and up.
constexpr double kSpecReplayMax = 1.0 / 6.0;
// decode_keys samples the replay count of a QBER that twice stayed under
// kSpecCkptSwitch only once every this many calls
constexpr uint64_t kSpecStatEvery = 64;

template <int RULE> struct RuleMsg { using T = float; };
template <> struct RuleMsg<kRuleSp64> { using T = double; };

// Key verification (qkd_verify.h) of a launch's frames: the key string, the
// tag mask and where the tags go. verified[f] = sp_ok[f] && the masked tag
// equals alice_tags[f]'s; written exactly when alice_tags is given.
struct VerifyArgs {
    uint64_t seed;                // the seeded key string (words == nullptr)
    const uint64_t* words;        // the caller's key string (key_words of them, device) or nullptr
    uint32_t key_words;           // qkdv::verify_key_words(n)
    uint64_t mask;                // qkdv::verify_tag_mask(tag_bits)
    const uint64_t* alice_tags;   // [F] or nullptr
    uint64_t* tags_out;           // [F] or nullptr
    uint8_t* verified;            // [F], with alice_tags
    const uint8_t* sp_ok;         // [F] the decoder's syndromes_match, with alice_tags
};

struct DecodeArgs {
    DeviceCode code;
    uint32_t n_frames;
    uint32_t max_it;
    double thr;
    int clamp_on;
    float ms_scale;    // kRuleMinSum normalisation
    float ms_offset;   // kRuleMinSum offset (subtracted after the scale, floored at 0)
    int ms_sc;         // kRuleMinSumLds: self-corrected (QKD_MINSUM_SELF_CORRECT)
    // kModeLlr
    const double* llr;
    // the caller's target syndrome bytes (F x M, nonzero = 1): kModeLlr, and
    // kModeKeys when the target is given instead of computed from Alice's key
    // (qkd_reconcile_batch: alice_b and key_ok are nullptr, alice_w is neither
    // read nor written); nullptr on the other keys-path calls
    const uint8_t* syn;
    // kModeKeys
    const uint64_t* alice_w;
    const uint64_t* bob_w;
    // qkd_qkd_ldpc_batch: the caller's byte keys (F x N, 0/1), packed into
    // alice_w / bob_w by the frame-syndrome kernel itself (the split path's
    // byte form) or by pack_kernel first (launch_pack_keys); nullptr when the
    // keys are packed already (device keygen)
    const uint8_t* alice_b;
    const uint8_t* bob_b;
    uint32_t words;
    double log_p;
    // First-iteration message table (kModeKeys): with every channel LLR equal
    // to +-log_p, the first check phase is a function of signs and degrees
    // only (see first_check_phase); first_c2b[d] = its message magnitude for
    // a check of degree d. Used when first_table != 0.
    int first_table;
    double first_c2b[kFirstTableDeg + 1];
    // Second-iteration tanh table (kModeKeys, needs first_table): entries,
    // 0 when off (see second_table_fill).
    int tab2_entries;
    // speculative kernel, QKD path: entries of the folded first iteration's
    // table (kFoldTabPat per degree pattern, decode_split.hip fold_table_fill),
    // 0 when off
    int ftab_entries;
    // outputs
    uint8_t* bits_out;
    uint32_t* iters;
    uint8_t* sp_ok;
    uint8_t* key_ok;
    // scratch
    double* c2b;
    size_t c2b_stride;
    uint32_t* counter;
    // diagnostics: per-phase shader-clock cycles summed over workgroups
    // (thread 0's view between barriers), or nullptr
    unsigned long long* phase;
    // qkd_trace_decode (binary64 rule, one frame): per executed iteration, the
    // c2b store (max_dv x n_pad) then the bit totals (n_pad), or nullptr
    double* trace;
    size_t trace_stride;
    // large codes (decode_kernel<..., GT = true>): the bit totals of each
    // workgroup's frame in global scratch, totals_stride doubles apart
    double* totals;
    size_t totals_stride;
    // decode_split_kernel: the LDS budget its layout was sized for (SplitLds)
    uint32_t lds_budget;
    // decode_split_kernel, binary64 rule: DeviceCode::plan_slot with the slot
    // field encoded for this launch's layout (encode_slot)
    const uint2* plan_enc;
    // speculative kernel, buckets 4 and 6 (QKD_CHECK_LANES): bit 31 set = the
    // interval check phases run one check per lane (spec_check_phase_lanes)
    // over cl_tasks = bits 0-15 tasks of the check-lane plan, then the
    // edge-lane phase over the rem_tasks = bits 16-30 tasks of the remainder
    // plan; both follow the edge-lane plan in plan_enc (cl_plan_offsets). 0:
    // the edge-lane phases over the whole plan
    uint32_t cl_split;
    // decode_split_kernel, kModeKeys: per frame 2 * m_words syndrome words
    // from frame_syn_kernel (target s_A, then the first-product signs), and
    // the frame's last hard decision out as packed words (key_match_kernel
    // compares them with Alice's key and unpacks bits_out)
    const uint32_t* synw;
    uint64_t* zout;
    // decode_split_kernel, kModeKeys, binary64 rule: speculative interval
    // iterations (qkd_spec.h) before the exact ones; spec_cap = how many (0:
    // off), log_p and thr as binary32 bounds, spec_replays counts the frames
    // that fell back to the exact iterations
    uint32_t spec_cap;
    float lp_dn, lp_up, thr_dn, thr_up;
    float pinf;          // +inf (an operand the compiler cannot fold: decode_split.hip)
    unsigned long long* spec_replays;
    // frames replayed exactly in this launch (zeroed per launch): once they
    // pass a quarter of the frames started, later frames skip the speculation
    uint32_t* replay_count;
    // QKD_SPEC_POLICY=always (tests): the in-launch replay policy never turns
    // the speculation off
    uint32_t spec_always;
    // The in-launch replay policy over frame-index windows of 2^win_shift
    // frames (decode_split.hip spec_policy): 64-bit word w of win (2 *
    // win_count uint32) holds window w's completed frames (low half) and
    // replay events (high half), zeroed per launch by the frame-syndrome
    // kernel, or a memset. Frame f speculates iff window
    // f / W - win_lag replayed at most a sixth of its frames (windows below
    // win_lag: always) -- a function of the frames alone, not of the order in
    // which workgroups finish them.
    uint32_t* win;
    uint32_t win_count;
    uint32_t win_shift;
    uint32_t win_lag;
    // checkpointed speculation (SPEC 2, high QBER): once an exact iteration
    // leaves at most ckpt_unsat checks unsatisfied, the messages are saved to
    // ckpt (ckpt_stride elements per workgroup) and the iterations continue on
    // intervals; a frame they cannot certify resumes exactly from the save
    double* ckpt;
    uint32_t ckpt_stride;
    uint32_t ckpt_unsat;
    // the frame-interleaved decoder (decode_ilv.hip): its message lines
    // (ilv_stride doubles per workgroup) and the frames whose intervals could
    // not certify, for the split kernel (fb_list, fb_count entries)
    double* ilv_store;
    size_t ilv_stride;
    uint32_t* fb_list;
    uint32_t* fb_count;
    // decode_split_kernel and decode_kernel: decode only
    // frame_list[0 .. *frame_count) (the interleaved decoder's hand-offs; the
    // open frames of a round of qkd_reconcile_blind_batch), or every frame
    // when nullptr
    const uint32_t* frame_list;
    const uint32_t* frame_count;
    // kModeClass: the frames' class bytes (F x N, the launched view's bit
    // order), the shortened bits' LLR, and the payload outputs: src[i] = the
    // payload index of the view's bit i (< 0: punctured or shortened),
    // payload_out F x n_payload, flips[f] = popcount(payload_out ^ bob's
    // payload) or nullptr. bits_out (may be nullptr): the whole decision.
    const uint8_t* cls;
    double known;
    const int32_t* src;
    uint8_t* payload_out;
    uint32_t n_payload;
    uint32_t* flips;
    // kModeClass, key verification (qkd_reconcile_adaptive_verify_batch,
    // qkd_reconcile_blind_verify_batch; vkey == nullptr: none, and the kernel
    // instantiation without it, the VFY template parameter): the payload's
    // tag (qkd_verify.h, positions = payload indices) taken in the loop that
    // writes payload_out. vkey: the qkdv::verify_key_words(n_payload) words of
    // the key string on the device, exactly that many (the caller's, or the
    // workspace's expansion of the seed); vmask: qkdv::verify_tag_mask(tag_bits).
    // vtags[f] (or nullptr) = the masked tag; with valice, vok[f] = sp_ok[f] &&
    // the masked tag equals valice[f]'s.
    const uint64_t* vkey;
    uint64_t vmask;
    const uint64_t* valice;
    uint64_t* vtags;
    uint8_t* vok;
};

// kModeClass with DecodeArgs::vkey: the payload decision d at payload index k
// adds W(k) & -(d) to the thread's XOR (the per-position form of qkd_verify.h).
// At k & 63 == 0 the window is R[k >> 6] itself and the word after it may lie
// past the string's end: the low word is read twice instead.
__device__ __forceinline__ uint64_t class_verify_window(const uint64_t* __restrict__ R, uint32_t k, uint32_t d) {
    const uint32_t w = k >> 6, s = k & 63u;
    const uint64_t lo = R[w], hi = R[w + (s ? 1u : 0u)];
    return qkdv::verify_window(lo, hi, s) & (0ull - (uint64_t)d);
}

// The XOR of v over the lanes of a wave, in every lane.
__device__ __forceinline__ uint64_t wave_xor64(uint64_t v) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        lo ^= (uint32_t)__shfl_xor((int)lo, s);
        hi ^= (uint32_t)__shfl_xor((int)hi, s);
    }
    return ((uint64_t)hi << 32) | lo;
}

// Thread 0, after the barrier that follows the waves' stores of their XORs to
// red[0 .. kDecodeBlock / 64): the frame's tag out and, against Alice's, the
// verdict (DecodeArgs::vmask, vtags, valice, vok).
__device__ __forceinline__ void class_verify_finish(const uint64_t* red, uint64_t mask, uint64_t* vtags,
                                                    const uint64_t* valice, uint8_t* vok, uint32_t f, bool sp_ok) {
    uint64_t t = 0;
#pragma unroll
    for (int w = 0; w < kDecodeBlock / 64; ++w) t ^= red[w];
    t &= mask;
    if (vtags) vtags[f] = t;
    if (valice) vok[f] = (sp_ok && ((t ^ valice[f]) & mask) == 0) ? 1 : 0;
}

// kModeClass: the channel LLR of a class byte (selects on registers: no table)
__device__ __forceinline__ double class_llr(uint32_t cl, double log_p, double known) {
    const double a = (cl & 1u) ? -log_p : log_p;
    const double b = (cl & 1u) ? known : 0.0;
    const double v = (cl & 2u) ? b : a;
    // classes 4 and 5 (revealed bits): +known / -known
    const double r = (cl & 1u) ? -known : known;
    return (cl & 4u) ? r : v;
}

// Phase-clock accumulation (diagnostic; a wave-uniform test when off). Each
// mark adds straight to the global slot, so nothing is indexed dynamically in
// registers (an accumulator array would live in scratch).
struct PhaseClock {
    unsigned long long* out;
    long long t = 0;
    __device__ explicit PhaseClock(unsigned long long* o) : out(threadIdx.x == 0 ? o : nullptr) {
        if (out) t = clock64();
    }
    __device__ __forceinline__ void mark(int k) {
        if (out) {
            const long long n = clock64();
            atomicAdd(out + k, (unsigned long long)(n - t));
            t = n;
        }
    }
    __device__ void flush() {}
};

template <typename T>
__device__ __forceinline__ T clamp_msg(T v, T thr) {
    // threshold_matrix_irregular (array_and_matrix_operations.cpp:508-524):
    // compare-based, so NaN passes through.
    return v > thr ? thr : (v < -thr ? -thr : v);
}

// Block-wide any(); flags[2] live in LDS and alternate between calls. Every
// call must be separated from the next by at least one __syncthreads().
__device__ __forceinline__ bool block_any(bool p, uint32_t* flags, uint32_t& k) {
    uint32_t* f = flags + (k & 1u);
    const bool wave_hit = __any(p);
    if (wave_hit && (threadIdx.x & 63) == 0) atomicOr(f, 1u);
    __syncthreads();
    const bool r = *f != 0;
    if (threadIdx.x == 0) flags[(k + 1) & 1u] = 0;
    k++;
    return r;
}


constexpr int kBitChunk = 5;
#ifndef QKD_SPEC_EXACT_CHUNK
#define QKD_SPEC_EXACT_CHUNK 2
#endif
constexpr int kBitChunkSpec = QKD_SPEC_EXACT_CHUNK;     // the exact iterations inside the speculative kernel
// Plan-walking loops outside the check phase load this many tasks' plan words
// per trip (the plan carries kPlanPadTasks >= kPlanGroup * NW idle tasks).
constexpr int kPlanGroup = 4;

// ---- wave-plan words (qkd_plan.h) ------------------------------------------
__device__ __forceinline__ uint32_t pw_bit(uint2 p) { return p.x & qkdp::kPlanBitMask; }
// DeviceCode::plan_slot's first word: the edge's message slot
__device__ __forceinline__ uint32_t pw_slot(uint2 p) { return p.x; }
__device__ __forceinline__ uint32_t pw_row(uint2 p) { return p.x >> 24; }
__device__ __forceinline__ uint32_t pw_chk(uint2 p) { return p.y & qkdp::kPlanChkMask; }
__device__ __forceinline__ int pw_start(uint2 p) { return (int)((p.y >> 20) & 63u); }
__device__ __forceinline__ int pw_deg(uint2 p) { return (int)(p.y >> 26) + 1; }
// Parity of the lanes of this lane's check (its segment) in a wave ballot.
__device__ __forceinline__ int seg_parity(uint64_t ballot, uint2 w) {
    // the segment's bits start at lane pw_start: shift them down, keep deg
    // (<= 64) of them, count
    const uint64_t sh = ballot >> pw_start(w);
    const int deg = pw_deg(w);
    // (v_bfe_u32 takes its width from 5 bits: a width of 32 would read as 0)
    if (deg < 32) return __popc(__builtin_amdgcn_ubfe((uint32_t)sh, 0, (uint32_t)deg)) & 1;
    const uint64_t m = deg == 64 ? ~0ull : ((1ull << deg) - 1ull);
    return __popcll(sh & m) & 1;
}
// The same for segments known to be shorter than 32 lanes (check-degree
// buckets up to 16; v_bfe_u32's width field has 5 bits).
__device__ __forceinline__ int seg_parity32(uint64_t ballot, uint2 w) {
    const uint32_t sh = (uint32_t)(ballot >> pw_start(w));
    return __popc(__builtin_amdgcn_ubfe(sh, 0, (uint32_t)pw_deg(w))) & 1;
}

// One edge of the check phase (qkd_ldpc_algorithm.cpp:220-249):
//   b2c = FIRST ? LLR_i : clamp(total_i - c2b)                  (:188, :303-316)
//   t   = tanh(b2c / 2)                                         (:224)
//   P   = (s_j ? -1 : 1) * t_0 * t_1 * ...  (ascending bits)    (:231-235)
//   c2b = clamp(2 * atanh(P / t))                               (:239-249)
// `row` is this wave's LDS row of tanh values (64 + DC doubles, so reads past
// a segment's end stay inside it and are discarded).
// Where a check phase takes its incoming tanh values from.
enum CheckSrc : int {
    kSrcGeneral = 0,   // tanh(clamp(total_i - c2b) / 2)
    kSrcFirst = 1,     // first iteration: tanh(LLR_i / 2)
    kSrcTable = 2      // second QKD iteration: looked up (second_table_index)
};

template <int RULE> struct RuleMath;
template <> struct RuleMath<kRuleSp64> {
    static __device__ __forceinline__ double tanh_half(double x) { return qkdm::tanh_flat(x / 2.0); }
    static __device__ __forceinline__ double two_atanh(double p) { return 2.0 * qkdm::atanh_flat(p); }
};
// The binary32 variant evaluates the check rule in Gallager's form,
//   c2b = sigma * phi(sum_{k != self} phi(|b2c_k|)),  phi(x) = -ln tanh(x / 2),
// sigma = s_j xor the other signs: the sum-product rule without the tanh
// domain's binary32 trouble (tanh(b2c / 2) rounds to 1 from |b2c| ~ 18 on,
// and P / t is 0 / 0 when a b2c cancels to 0). "tanh_half" publishes
// sign(b2c) * psi(|b2c|), psi = phi / ln 2, with |b2c| limited to [1e-30,
// 80] so psi is finite and positive (the sign survives); "two_atanh" maps a
// psi-unit sum S to phi(S ln 2) (S limited to 115).
//
// This is a decoder, not a certificate: phi only needs to be accurate to a
// few 1e-6 relative (tests/test_variants.py holds it to 5e-6 against binary64
// numpy), which needs far fewer operations than the certified bounds'
// qkds::phi_core (2^-20 with an exact argument split):
//   x < 1/32:      w = x (1 - x/2 + x^2/6)   (truncation < x^3/24 < 1.3e-6 of w)
//   1/32 <= x:     w = 1 - u, u = e^-x = 2^-(x log2 e) (no argument split:
//                  x log2 e rounds to 2^-24 relative, ~4e-6 of psi at x = 80)
//   x < 2:         phi = ln((2 - w) / w)     (argument >= 1.31: v_log_f32's
//                  absolute error stays ~1e-7 of the value)
//   x >= 2:        phi = 2u (1 + s/3 + s^2/5), s = u^2 <= e^-4 (truncation < 9e-7)
// Measured (numpy model of the same steps): 3.7e-6 relative worst case, ~1e-6
// for x < 20.
namespace sp32m {
template <bool PSI>
__device__ __forceinline__ float phi(float x, float u) {
    float t = __builtin_fmaf(x, 1.0f / 6.0f, -0.5f);
    t = __builtin_fmaf(x, t, 1.0f);
    const float w = x < 0.03125f ? x * t : 1.0f - u;
    const float lg = __builtin_amdgcn_logf((2.0f - w) * __builtin_amdgcn_rcpf(w));
    const float vlo = PSI ? lg : qkds::kLn2 * lg;
    const float s = u * u;
    float h = __builtin_fmaf(s, 0.2f, 1.0f / 3.0f);
    h = __builtin_fmaf(s, h, 1.0f);
    const float vhi = (u * (PSI ? 2.0f * qkds::kInvLn2 : 2.0f)) * h;
    return x < 2.0f ? vlo : vhi;
}
}  // namespace sp32m
template <> struct RuleMath<kRuleSp32> {
    static __device__ __forceinline__ float tanh_half(float x) {
        const float a = __builtin_amdgcn_fmed3f(__builtin_fabsf(x), 1.0e-30f, qkds::kPhiHuge);
        const float p = sp32m::phi<true>(a, __builtin_amdgcn_exp2f(a * -qkds::kInvLn2));
        return x < 0.0f ? -p : p;
    }
    static __device__ __forceinline__ float two_atanh(float s) {
        const float at = __builtin_fminf(s, qkds::kPsiHuge);
        return sp32m::phi<false>(at * qkds::kLn2, __builtin_amdgcn_exp2f(-at));
    }
    // |tanh_half(x)| (half 0) and two_atanh(s) (half 1) in one packed
    // evaluation: every operation is the scalar forms', so each half is bit
    // for bit their result (tests/test_variants.py compares them)
    static __device__ __forceinline__ qkds::f2 pair(float x, float s) {
        typedef qkds::f2 f2;
        const float a = __builtin_amdgcn_fmed3f(__builtin_fabsf(x), 1.0e-30f, qkds::kPhiHuge);
        const float at = __builtin_fminf(s, qkds::kPsiHuge);
        const f2 e = f2{a, at} * f2{-qkds::kInvLn2, -1.0f};
        const f2 u = f2{__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)};
        const f2 xx = f2{a, at * qkds::kLn2};
        f2 t = __builtin_elementwise_fma(xx, f2(1.0f / 6.0f), f2(-0.5f));
        t = __builtin_elementwise_fma(xx, t, f2(1.0f));
        const f2 ws = xx * t;
        const f2 wd = f2(1.0f) - u;
        const f2 w = f2{xx.x < 0.03125f ? ws.x : wd.x, xx.y < 0.03125f ? ws.y : wd.y};
        const f2 arg = (f2(2.0f) - w) * f2{__builtin_amdgcn_rcpf(w.x), __builtin_amdgcn_rcpf(w.y)};
        const float lg1 = __builtin_amdgcn_logf(arg.y);
        const f2 vlo = f2{__builtin_amdgcn_logf(arg.x), qkds::kLn2 * lg1};
        const f2 sq = u * u;
        f2 h = __builtin_elementwise_fma(sq, f2(0.2f), f2(1.0f / 3.0f));
        h = __builtin_elementwise_fma(sq, h, f2(1.0f));
        const f2 vhi = (u * f2{2.0f * qkds::kInvLn2, 2.0f}) * h;
        return f2{xx.x < 2.0f ? vlo.x : vhi.x, xx.y < 2.0f ? vlo.y : vhi.y};
    }
};

// A check-phase message store. (Non-temporal stores, which skip L2, measured
// 2x slower: the bit phase re-reads these lines shortly after.)
template <typename T>
__device__ __forceinline__ void msg_store(T* p, T v) {
    *p = v;
}

// Makes this wave's LDS row writes visible to its own lanes (no s_barrier).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// First half of an edge: the value the lane publishes in its wave's LDS row.
//   sum-product: t = tanh(b2c / 2) (or the tabulated t), min-sum: b2c itself.
template <int SRC, bool CLAMP, int RULE, typename T>
__device__ __forceinline__ T edge_in(T x, T old, T thr) {
    if (SRC == kSrcGeneral) {
        x = x - old;
        if (CLAMP) x = clamp_msg(x, thr);
    }
    if constexpr (RULE == kRuleMinSum) return x;
    else return SRC == kSrcTable ? x : RuleMath<RULE>::tanh_half(x);
}

// Second half: the lane's message from the published row of its check
// (segment [start, start + deg) of `row`; the row has 64 + DC entries, so reads
// past a segment's end stay inside it and are discarded).
// ERA (QKD_FLAG_ERASURES, binary64 rule): the rule extended to published
// values that are zero. With z = the number of zero t_k of the check (either
// sign): z = 0 the reference rule; z = 1 the edge whose t is zero gets
// 2 atanh(P'), P' the product without it (same order), every other edge +0.0;
// z >= 2 every edge +0.0. A frame without a zero t computes what the reference
// rule computes, operation for operation.
template <bool CLAMP, int DC, int RULE, bool ERA = false, typename T>
__device__ __forceinline__ T edge_out(T tv, uint2 w, uint32_t sbit, int lane, T thr, const T* row,
                                      float ms_scale, float ms_offset = 0.0f) {
    const int start = pw_start(w);
    const int deg = pw_deg(w);
    T o[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) o[k] = row[start + k];
    T v;
    if constexpr (RULE == kRuleMinSum) {
        // c2b = scale * (s_j ^ signs of the other b2c) * min over the other |b2c|
        uint32_t neg = sbit ^ (tv < 0 ? 1u : 0u);
        T mn = __builtin_inff();
#pragma unroll
        for (int k = 0; k < DC; ++k) {
            if (k < deg) {
                neg ^= o[k] < 0 ? 1u : 0u;
                if (start + k != lane) mn = fminf(mn, fabsf(o[k]));
            }
        }
        v = (T)ms_scale * mn;
        if (ms_offset > 0.0f) v = fmaxf(v - (T)ms_offset, (T)0);
        v = neg ? -v : v;
    } else if constexpr (RULE == kRuleSp64) {
        // the reference's P = (s_j ? -1 : 1) * prod_k t_k, then 2 atanh(P / t_self) (:231-241)
        T P = sbit ? (T)-1 : (T)1;
        if constexpr (ERA) {
            int z = 0;
#pragma unroll
            for (int k = 0; k < DC; ++k) {
                if (k < deg) {
                    const bool zero = o[k] == (T)0;
                    z += zero ? 1 : 0;
                    P = zero ? P : P * o[k];
                }
            }
            v = RuleMath<RULE>::two_atanh(z == 0 ? P / tv : P);
            if (z >= 2 || (z == 1 && !(tv == (T)0))) v = (T)0;
        } else {
            P = P * o[0];                         // every check has degree >= 1
#pragma unroll
            for (int k = 1; k < DC; ++k) P = k < deg ? P * o[k] : P;
            v = RuleMath<RULE>::two_atanh(P / tv);
        }
    } else {
        // binary32 variant (Gallager form, RuleMath<kRuleSp32>): the extrinsic
        // psi sum over the other edges in ascending order and their sign parity
        T S = (T)0;
        uint32_t neg = sbit;
#pragma unroll
        for (int k = 0; k < DC; ++k) {
            if (k < deg && start + k != lane) {
                S = S + __builtin_fabsf(o[k]);
                neg ^= o[k] < (T)0 ? 1u : 0u;
            }
        }
        v = RuleMath<RULE>::two_atanh(S);
        v = neg ? -v : v;
    }
    if (CLAMP) v = clamp_msg(v, thr);
    return v;
}

// Second check phase of the QKD path. After the first iteration every message
// is +-C_d (first_check_phase), so bit i's total is
//   total_i = ((LLR_i + c_0) + c_1) + ...    c_k = sign_k * C_{d_k}   (:256-267)
// and its second-iteration incoming value for its k-th check is
//   t = tanh(clamp(total_i - c_k) / 2)                            (:303-316, :224)
// a function of (the degrees d_k of bit i's checks, bob_i, sign_0.., k). The
// table holds it for every degree pattern p, sign code and row k:
//   tab2[p * stride + code * max_dv + k],  code = bob_i | sign_k << (1 + k)
// computed with the same binary64 operations in the same order. The
// iteration-1 bit phase records each bit's base index (second_table_index).
template <bool CLAMP>
__device__ void second_table_fill(const DeviceCode& c, const double* ctab, double log_p, double thr,
                                  double* tab2, int entries) {
    const int dvm = c.max_dv;
    const int stride = tab2_stride(dvm);
    for (int e = threadIdx.x; e < entries; e += kDecodeBlock) {
        const int p = e / stride;
        const int r = e - p * stride;
        const int code = r / dvm;
        const int k = r - code * dvm;
        const uint8_t* degs = c.pat_deg + p * dvm;
        double total = (code & 1) ? -log_p : log_p;
        double ck = 0.0;
        int dv = 0;
        for (int m = 0; m < dvm; ++m) {
            if (degs[m] == 0) break;
            const double cm = ctab[degs[m]];
            const double v = ((code >> (1 + m)) & 1) ? -cm : cm;
            total = total + v;
            if (m == k) ck = v;
            dv = m + 1;
        }
        double y = 0.0;
        if (k < dv) {
            double b = total - ck;
            if (CLAMP) b = clamp_msg(b, thr);
            y = qkdm::tanh_flat(b / 2.0);
        }
        tab2[e] = y;
    }
    __syncthreads();
}

// ---- split message store (decode_split.hip) ----------------------------------
// (its LDS layout SplitLds and the slot words' constants: qkd_launch.h)
__host__ __device__ inline uint32_t encode_slot(uint32_t x, uint32_t S, uint32_t msg, uint32_t esz) {
    return x < S ? (kSlotLds | (msg + x * esz)) : (kSlotGlobalBase + (x - S) * esz);
}

// The encoded plan's second word (check-degree bucket DC), the lane's
// segment and its check's target bit pre-decoded for the check phases:
//   bits 0-4    j & 31: the target bit's position in its syndrome word (a
//               shift by the whole word uses these bits only)
//   bits 5-10   start: the segment's first lane
//   bits 11-18  wi: the row of the segment-weight table (SegWeights): DC <= 8:
//               deg * 8 + min(lane - start, DC - 1); DC = 16: (deg - 1) * DC +
//               min(lane - start, DC - 1); wider buckets: deg - 1
//   bits 19-31  (j >> 5) * 4: the byte offset of the check's syndrome word
// (needs M <= 65536: the split decoder's limit).
constexpr uint32_t kSegStartShift = 5, kSegWiShift = 11, kSegWordShift = 19;
__host__ __device__ inline uint32_t encode_seg(uint32_t j, uint32_t start, uint32_t deg, uint32_t lane, uint32_t dc) {
    const uint32_t p = lane - start;
    const uint32_t pc = p < dc - 1 ? p : dc - 1;
    const uint32_t wi = dc <= 8 ? deg * 8 + pc : dc <= 16 ? (deg - 1) * dc + pc : deg - 1;
    return (j & 31u) | (start << kSegStartShift) | (wi << kSegWiShift) | (((j >> 5) * 4u) << kSegWordShift);
}

// The check-lane plan (qkd_plan.h CheckLanePlan) encoded for a layout: per
// task dc + 1 rows of 64 words, one per lane: rows k < dc the encoded slot
// word (encode_slot) of the lane's check's k-th entry (past its degree the
// reserved word kSlotDead: the entry loads {+0, +0}, which the psi-input form
// reads as "psi = 0, sign +", and its store is dropped -- no compare with the
// degree on its account), row dc the check's word as the plan builder made it
// (qkdp::encode_chk: syndrome word offset, bit, degree).
// In DecodeArgs::plan_enc the remainder's edge-lane plan (rem_tasks +
// kPlanPadTasks tasks) follows the n_tasks + kPlanPadTasks tasks of the whole
// edge-lane plan, and the check-lane words follow the remainder.
static_assert(qkdp::kChkWordShift == kSegWordShift, "check words address syndrome words as segment words do");
__host__ __device__ inline size_t cl_rem_offset(int n_tasks) {      // in uint2 words
    return (size_t)(n_tasks + qkdp::kPlanPadTasks) * 64;
}
__host__ __device__ inline size_t cl_words_offset(int n_tasks, int rem_tasks) {
    return cl_rem_offset(n_tasks) + (size_t)(rem_tasks + qkdp::kPlanPadTasks) * 64;
}

using DecodeFn = void (*)(DecodeArgs);
// The kernel of a key (qkd_launch.h KernelKey), one lookup per translation
// unit: decode_split.hip (kKernelSplit), decode_ilv.hip (kKernelIlv); the
// classic kernels' (decode.hip classic_kernel) is declared in qkd_host.h.
// nullptr: no such instantiation.
DecodeFn split_kernel(const KernelKey& k);
DecodeFn ilv_kernel(const KernelKey& k);
// kModeKeys: the kernels around the split decoder. Before (frame_syn.hip):
// a.synw from the packed keys. After (frame_out.hip): key_ok / bits_out from a.zout.
// gather: the gather kernel instead of the bit-sliced one; pack_first: byte
// keys packed by pack_kernel first (the QKD_SYN_SLICED / QKD_SYN_BYTES options)
// a.syn set (qkd_reconcile_batch): the given-target kernels, Bob's key alone.
hipError_t launch_frame_syn(const DecodeArgs& a, hipStream_t stream, bool gather = false, bool pack_first = false);
// bits.hip: a.alice_b / a.bob_b -> a.alice_w / a.bob_w (original bit order);
// a.alice_b == nullptr: Bob's key alone
hipError_t launch_pack_keys(const DecodeArgs& a, hipStream_t stream);
// corrected (qkd_reconcile_batch, with a.bits_out and a.bob_b): the unpack
// also writes popcount(bits_out ^ bob) per frame
// v (qkd_reconcile_verify_batch): the unpack also takes the frame's
// verification tag (zout_unpack_verify_kernel; corrected may then be nullptr)
hipError_t launch_key_match(const DecodeArgs& a, hipStream_t stream, uint32_t* corrected = nullptr,
                            const VerifyArgs* v = nullptr);
// the same count after the classic kernel, which writes bits_out itself
hipError_t launch_count_flips(const uint8_t* bits, const uint8_t* bob, uint32_t n, uint32_t n_frames,
                              uint32_t* corrected, hipStream_t stream);
// the verification tags of byte keys bits[F x N] (qkd_verify_tags_batch, and
// qkd_reconcile_verify_batch after the classic kernel): one launch, no workspace
hipError_t launch_verify_tags(const uint8_t* bits, uint32_t n, uint32_t n_frames, const VerifyArgs& v,
                              hipStream_t stream);
// adapt.hip, kModeClass: what the decode launch needs of a qkd_adapt and its call
// (the plan's maps in both bit orders, Bob's payload, the workspace's class
// bytes), and the kernel that writes the class bytes of F frames from a map:
// cls[f * n + i] = src[i] >= 0 ? payload[f * n_payload + src[i]] & 1
//                              : src[i] == kSrcPunctured ? 2 : 3
// qkd_reconcile_blind_batch (blind != nullptr): the class bytes of the frames
// of the round's list only, a punctured position of rank j (rank_orig /
// rank_int: its index in the plan's punctured list, -1 elsewhere) being
// 4 | (revealed[f * p + j] & 1) when j < min(n_revealed[f], p), else 2.
struct BlindArgs {
    const int32_t* rank_orig;
    const int32_t* rank_int;
    const uint8_t* revealed;         // F x p (nullptr when p = 0)
    const uint32_t* n_revealed;      // F
    uint32_t p;
    const uint32_t* list;            // the round's open frames
    const uint32_t* count;           // how many of them
};
struct ClassArgs {
    const int32_t* src_orig;
    const int32_t* src_int;
    const uint8_t* bob_payload;
    uint8_t* cls;
    const BlindArgs* blind = nullptr;
};
constexpr int32_t kSrcPunctured = -1, kSrcShortened = -2;
hipError_t launch_adapt_classes(const int32_t* src, const uint8_t* payload, uint32_t n, uint32_t n_payload,
                                uint32_t n_frames, uint8_t* cls, hipStream_t stream);
// the same for the frames list[0 .. *count) only (grid sized for n_frames: a
// block past the count exits)
hipError_t launch_blind_classes(const int32_t* src, const int32_t* rank, const uint8_t* payload, const BlindArgs& b,
                                uint32_t n, uint32_t n_payload, uint32_t n_frames, uint8_t* cls, hipStream_t stream);
// One round's bookkeeping of qkd_reconcile_blind_batch (adapt.hip
// blind_round_kernel): closes and advances the frames of the round before,
// then compacts the open frames into list / *count in ascending order.
struct BlindRound {
    uint32_t round;                  // t
    uint32_t n_frames, p, step;
    const uint8_t* skip;             // F or nullptr
    const uint8_t* sp_ok;            // F: the decoder's syndromes_match
    uint32_t* n_revealed;            // F, in/out
    uint32_t* rounds;                // F or nullptr
    uint8_t* open;                   // F: workspace
    uint32_t* list;
    uint32_t* count;
    // qkd_reconcile_blind_verify_batch with alice_tags: the decoder's verified
    // (F); a frame is then closed by it instead of by sp_ok. nullptr otherwise.
    const uint8_t* verified = nullptr;
};
hipError_t launch_blind_round(const BlindRound& r, hipStream_t stream);
// out[0 .. words) = the seeded key string of the verification hash
// (qkdv::verify_key_word), once per verifying class-mode call
hipError_t launch_verify_expand(uint64_t seed, uint32_t words, uint64_t* out, hipStream_t stream);

}  // namespace qkd
