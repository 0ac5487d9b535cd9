// api.hip — the C ABI entries that decode (include/qkd_ldpc.h); no kernels.
//
// Each entry checks its arguments, opens a session on the workspace and hands a
// DecodeArgs to launch_decode (launch.hip). decode_keys is the keys path the
// reference runs per trial (QKD_LDPC_*, src/qkd_ldpc_algorithm.cpp:347-447:
// log_p at :400, the first-iteration tables, the speculation policy across
// calls); the reconcile / adaptive / blind families are Bob's side from a
// received syndrome; qkd_interactive_batch is QKD_LDPC_interactive_simulation
// (src/simulation.cpp:73-137) and qkd_trials_batch run_trial with its
// reduction (:161-189, :252-312).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>
#include <vector>

#include "qkd_args.h"
#include "qkd_decode.h"
#include "qkd_host.h"
#include "qkd_rng.h"

namespace qkd {

qkd_status check_frames(size_t n_frames) {
    if (n_frames == 0) return set_error(QKD_ERR_INVALID_ARG, "n_frames must be > 0");
    if (n_frames > 0xffffffffull) return set_error(QKD_ERR_INVALID_ARG, "n_frames too large");
    return QKD_OK;
}

// erasures_ok: the entry takes QKD_FLAG_ERASURES (qkd_decode_batch; binary64 variant only)
qkd_status check_decode_params(uint32_t max_it, double thr, uint32_t flags, bool erasures_ok) {
    if (max_it < 1) return set_error(QKD_ERR_INVALID_ARG, "max_iterations must be >= 1");
    if (flags & QKD_FLAG_ERASURES) {
        if (!erasures_ok) return set_error(QKD_ERR_INVALID_ARG, "QKD_FLAG_ERASURES is not taken by this entry");
        if ((flags & QKD_VARIANT_MASK) != QKD_VARIANT_SP_F64)
            return set_error(QKD_ERR_INVALID_ARG, "QKD_FLAG_ERASURES needs QKD_VARIANT_SP_F64");
        flags &= ~QKD_FLAG_ERASURES;
    }
    const uint32_t known = QKD_FLAG_THRESHOLD | QKD_VARIANT_MASK | (0xffu << QKD_MINSUM_SCALE_SHIFT) |
                           (0xffu << QKD_MINSUM_OFFSET_SHIFT) | QKD_MINSUM_SELF_CORRECT;
    if (flags & ~known) return set_error(QKD_ERR_INVALID_ARG, "unknown flags 0x%x", flags);
    if ((flags & QKD_VARIANT_MASK) == QKD_VARIANT_MASK)
        return set_error(QKD_ERR_INVALID_ARG, "unknown decoder variant 0x%x", flags & QKD_VARIANT_MASK);
    if ((flags >> QKD_MINSUM_SCALE_SHIFT) && (flags & QKD_VARIANT_MASK) != QKD_VARIANT_MINSUM)
        return set_error(QKD_ERR_INVALID_ARG, "min-sum scale or offset given without QKD_VARIANT_MINSUM");
    if ((flags & QKD_FLAG_THRESHOLD) && !(thr > 0.0))
        return set_error(QKD_ERR_INVALID_ARG, "message threshold must be > 0");
    return QKD_OK;
}

// binary32 bound of a binary64 value: the largest float <= x (up: smallest >= x)
static float f32_bound(double x, bool up) {
    float f = (float)x;
    if (up && (double)f < x) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    if (!up && (double)f > x) f = std::nextafter(f, -std::numeric_limits<float>::infinity());
    return f;
}

// The speculation policy's per-QBER record (qkd_workspace::spec_clean). The
// map is bounded: a workspace fed ever new QBERs (a continuous-q pipeline, a
// sweep) forgets the records once there are kSpecCleanMax of them, which only
// resamples those QBERs' replay fractions.
static constexpr size_t kSpecCleanMax = 64;
static SpecClean& spec_clean_of(qkd_workspace* ws, double q) {
    if (ws->spec_clean.size() >= kSpecCleanMax && !ws->spec_clean.count(q)) ws->spec_clean.clear();
    return ws->spec_clean[q];
}

// Shared by qkd_qkd_ldpc_batch, qkd_trials_batch and qkd_reconcile_batch: keys
// already packed in ws, or byte keys. syn (qkd_reconcile_batch): the target
// syndrome given by the caller, with bob_b alone (alice_b and key_ok nullptr);
// corrected: its flip counts; verify (qkd_reconcile_verify_batch): its tags.
qkd_status decode_keys(const qkd_code* c, qkd_workspace* ws, size_t n_frames, double q,
                       uint32_t max_it, double thr, uint32_t flags, uint8_t* bits_out,
                       uint32_t* iters, uint8_t* sp_ok, uint8_t* key_ok, hipStream_t stream,
                       const uint8_t* alice_b, const uint8_t* bob_b, const uint8_t* syn, uint32_t* corrected,
                       const VerifyArgs* verify) {
    DecodeArgs a{};
    a.alice_b = alice_b;
    a.bob_b = bob_b;
    a.syn = syn;
    a.pinf = std::numeric_limits<float>::infinity();
    a.n_frames = (uint32_t)n_frames;
    a.max_it = max_it;
    a.thr = thr;
    a.clamp_on = (flags & QKD_FLAG_THRESHOLD) ? 1 : 0;
    a.alice_w = ws->alice_w;
    a.bob_w = ws->bob_w;
    a.words = (uint32_t)((c->n + 63) / 64);
    a.log_p = std::log((1. - q) / q);          // host glibc log, qkd_ldpc_algorithm.cpp:400
    // first-iteration message magnitudes by check degree (first_check_phase)
    // (the binary32 rule folds on the device, decode_split_kernel; not at
    // log_p = 0, where Bob's 1 bits give -0.0, not negative)
    // (min-sum folds on the device too, decode_split_kernel)
    a.first_table = (c->max_dc <= kFirstTableDeg &&
                     (rule_of(flags) == kRuleSp64 ||
                      ((rule_of(flags) == kRuleSp32 || rule_of(flags) == kRuleMinSum) && a.log_p != 0.0)))
                        ? 1 : 0;
    if (a.first_table) {
        const double T = std::fabs(qkdm::tanh_flat(a.log_p / 2.0));
        double M = 1.0;
        a.first_c2b[0] = 0.0;
        for (int d = 1; d <= kFirstTableDeg; ++d) {
            M = M * T;
            double v = 2.0 * qkdm::atanh_flat(M / T);
            if (a.clamp_on) v = v > thr ? thr : (v < -thr ? -thr : v);
            a.first_c2b[d] = v;
        }
    }
    a.tab2_entries = (a.first_table && c->n_pat > 0 && rule_of(flags) == kRuleSp64)
                         ? c->n_pat * tab2_stride(c->max_dv) : 0;
    // speculative interval iterations (decode_split.hip, qkd_spec.h) ahead of
    // the exact ones, for the binary64 rule with clamped messages;
    // QKD_SPEC_CAP overrides how many (0: off)
    int cap = kSpecCapDefault;
    if (const DbgOpt e = debug_option(ws, "QKD_SPEC_CAP")) cap = std::max(0, e.as_int());
    a.spec_cap = (rule_of(flags) == kRuleSp64 && a.clamp_on && a.first_table) ? (uint32_t)cap : 0u;
    a.lp_dn = f32_bound(a.log_p, false);
    a.lp_up = f32_bound(a.log_p, true);
    a.thr_dn = f32_bound(thr, false);
    a.thr_up = f32_bound(thr, true);
    a.bits_out = bits_out;
    a.iters = iters;
    a.sp_ok = sp_ok;
    a.key_ok = key_ok;
    // across calls: the last speculative call's replay fraction, once its
    // count is back (never waits); above kSpecCkptSwitch the frames speculate
    // from a checkpoint instead, from that QBER up
    if (ws->spec_stat_pending && hipEventQuery(ws->spec_stat_ev) == hipSuccess) {
        ws->spec_stat_pending = false;
        const bool over = (double)*ws->spec_stat_host > kSpecCkptSwitch * (double)ws->spec_stat_frames;
        if (over) ws->spec_ckpt_q = std::min(ws->spec_ckpt_q, ws->spec_stat_q);
        SpecClean& sc = spec_clean_of(ws, ws->spec_stat_q);
        sc.clean = over ? 0 : sc.clean + 1;
    }
    // at and above that QBER: the checkpointed speculation (QKD_CKPT_UNSAT
    // overrides its trigger; 0: exact iterations only)
    a.ckpt = nullptr;
    a.ckpt_stride = 0;
    a.ckpt_unsat = 0;
    // (QKD_SPEC_CKPT=1: the checkpointed variant at every QBER; tests)
    const DbgOpt force_ck = debug_option(ws, "QKD_SPEC_CKPT");
    if (q >= ws->spec_ckpt_q || (force_ck && force_ck.as_int() == 1)) {
        int cu = kCkptUnsatDefault;
        if (const DbgOpt e = debug_option(ws, "QKD_CKPT_UNSAT")) cu = std::max(0, e.as_int());
        a.ckpt_unsat = (uint32_t)cu;
        if (cu == 0) a.spec_cap = 0;
    }
    qkd_status st = launch_decode(c, ws, a, kModeKeys, flags, stream, DecodeIo{corrected, verify, nullptr});
    if (st != QKD_OK || a.spec_cap == 0 || a.ckpt_unsat || ws->spec_stat_pending) return st;
    // (a QBER whose last two samples stayed under the switch is sampled again
    // only every kSpecStatEvery calls: each sample is a device-to-host copy
    // and an event on the caller's stream)
    {
        SpecClean& sc = spec_clean_of(ws, q);
        if (sc.clean >= 2 && (++sc.skip % kSpecStatEvery) != 0) return st;
    }
    if (!ws->spec_stat_host) {
        if (hipHostMalloc(reinterpret_cast<void**>(&ws->spec_stat_host), 8, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&ws->spec_stat_ev, hipEventDisableTiming) != hipSuccess)
            return QKD_OK;                        // no policy feedback, decoding is unaffected
    }
    if (hipMemcpyAsync(ws->spec_stat_host, ws->counter + 1, 4, hipMemcpyDeviceToHost, stream) == hipSuccess &&
        hipEventRecord(ws->spec_stat_ev, stream) == hipSuccess) {
        ws->spec_stat_pending = true;
        ws->spec_stat_q = q;
        ws->spec_stat_frames = n_frames;
    }
    return QKD_OK;
}

}  // namespace qkd

using namespace qkd;

extern "C" {

qkd_status qkd_decode_batch(const qkd_code* c, qkd_workspace* ws, const double* llr,
                            const uint8_t* syndrome, size_t n_frames, uint32_t max_iterations,
                            double msg_threshold, uint32_t flags, uint8_t* bits_out,
                            uint32_t* iterations, uint8_t* syndromes_match, void* stream) {
    clear_error();
    if (!c || !llr || !syndrome || !iterations || !syndromes_match)
        return set_error(QKD_ERR_INVALID_ARG, "null argument");
    qkd_status s = check_frames(n_frames);
    if (s == QKD_OK) s = check_decode_params(max_iterations, msg_threshold, flags, true);
    if (s != QKD_OK) return s;
    DeviceGuard g(c->device);
    ws = resolve_ws(c, ws);
    if (!ws) return set_error(QKD_ERR_OUT_OF_MEMORY, "no workspace");
    WsSession sess(ws, (hipStream_t)stream);
    DecodeArgs a{};
    a.pinf = std::numeric_limits<float>::infinity();
    a.n_frames = (uint32_t)n_frames;
    a.max_it = max_iterations;
    a.thr = msg_threshold;
    a.clamp_on = (flags & QKD_FLAG_THRESHOLD) ? 1 : 0;
    a.llr = llr;
    a.syn = syndrome;
    a.bits_out = bits_out;
    a.iters = iterations;
    a.sp_ok = syndromes_match;
    // speculative interval iterations (decode_split.hip, qkd_spec.h): binary64
    // rule with clamped messages; QKD_SPEC_CAP overrides how many (0: off)
    int cap = kSpecCapDefault;
    if (const DbgOpt e = debug_option(ws, "QKD_SPEC_CAP")) cap = std::max(0, e.as_int());
    a.spec_cap = (rule_of(flags) == kRuleSp64 && a.clamp_on) ? (uint32_t)cap : 0u;
    a.thr_dn = f32_bound(msg_threshold, false);
    a.thr_up = f32_bound(msg_threshold, true);
    return launch_decode(c, ws, a, kModeLlr, flags, (hipStream_t)stream);
}

qkd_status qkd_qkd_ldpc_batch(const qkd_code* c, qkd_workspace* ws, const uint8_t* alice,
                              const uint8_t* bob, size_t n_frames, double qber, uint32_t max_iterations,
                              double msg_threshold, uint32_t flags, uint8_t* bits_out,
                              uint32_t* iterations, uint8_t* syndromes_match, uint8_t* keys_match,
                              void* stream) {
    clear_error();
    if (!c || !alice || !bob || !iterations || !syndromes_match)
        return set_error(QKD_ERR_INVALID_ARG, "null argument");
    qkd_status s = check_frames(n_frames);
    if (s == QKD_OK) s = check_decode_params(max_iterations, msg_threshold, flags);
    if (s != QKD_OK) return s;
    if (!(qber > 0.0 && qber < 1.0)) return set_error(QKD_ERR_INVALID_ARG, "QBER must be in (0,1)");
    DeviceGuard g(c->device);
    ws = resolve_ws(c, ws);
    if (!ws) return set_error(QKD_ERR_OUT_OF_MEMORY, "no workspace");
    WsSession sess(ws, (hipStream_t)stream);
    s = ws_reserve_keys(ws, n_frames, 1);
    if (s != QKD_OK) return s;
    // the byte keys go to the decode launch, which packs them (the split
    // path inside its frame-syndrome kernel, launch_frame_syn)
    return decode_keys(c, ws, n_frames, qber, max_iterations, msg_threshold, flags, bits_out, iterations,
                       syndromes_match, keys_match, (hipStream_t)stream, alice, bob);
}

// qkd_reconcile_batch and qkd_reconcile_verify_batch after their argument
// checks; verify: the second's tags, nullptr for the first.
static qkd_status reconcile_run(const qkd_code* c, qkd_workspace* ws, const uint8_t* bob, const uint8_t* syndrome,
                                size_t n_frames, double qber, uint32_t max_iterations, double msg_threshold,
                                uint32_t flags, uint8_t* bits_out, uint32_t* iterations, uint8_t* syndromes_match,
                                uint32_t* corrected, const VerifyArgs* verify, void* stream) {
    qkd_status s = check_decode_params(max_iterations, msg_threshold, flags);
    if (s != QKD_OK) return s;
    DeviceGuard g(c->device);
    ws = resolve_ws(c, ws);
    if (!ws) return set_error(QKD_ERR_OUT_OF_MEMORY, "no workspace");
    WsSession sess(ws, (hipStream_t)stream);
    s = ws_reserve_keys(ws, n_frames, 1);
    if (s != QKD_OK) return s;
    // keys mode with the target given: no Alice key, no key compare (the
    // interleaved long-code decoder, which has no decisions to give, is
    // excluded by bits_out; codes it alone takes run the classic kernel)
    return decode_keys(c, ws, n_frames, qber, max_iterations, msg_threshold, flags, bits_out, iterations,
                       syndromes_match, nullptr, (hipStream_t)stream, nullptr, bob, syndrome, corrected, verify);
}

qkd_status qkd_reconcile_batch(const qkd_code* c, qkd_workspace* ws, const uint8_t* bob,
                               const uint8_t* syndrome, size_t n_frames, double qber, uint32_t max_iterations,
                               double msg_threshold, uint32_t flags, uint8_t* bits_out, uint32_t* iterations,
                               uint8_t* syndromes_match, uint32_t* corrected, void* stream) {
    clear_error();
    if (const char* bad = qkda::reconcile_args_error(c, bob, syndrome, n_frames, qber, bits_out, iterations,
                                                     syndromes_match))
        return set_error(QKD_ERR_INVALID_ARG, "%s", bad);
    return reconcile_run(c, ws, bob, syndrome, n_frames, qber, max_iterations, msg_threshold, flags, bits_out,
                         iterations, syndromes_match, corrected, nullptr, stream);
}

// one class byte per bit and frame: the only per-bit input the class-mode decoder reads
static qkd_status ws_reserve_classes(qkd_workspace* ws, size_t n_frames) {
    const size_t need = n_frames * (size_t)ws->code->n;
    if (ws->cls.reserve(need) != hipSuccess)
        return set_error(QKD_ERR_OUT_OF_MEMORY, "workspace: cannot allocate %zu B of class bytes", need);
    return QKD_OK;
}

// the class-mode launch arguments of qkd_reconcile_adaptive_batch and of a
// round of qkd_reconcile_blind_batch
static DecodeArgs class_decode_args(const qkd_adapt* ad, const uint8_t* syndrome, size_t n_frames, double qber,
                                    double known_llr, uint32_t max_iterations, double msg_threshold, uint32_t flags,
                                    uint8_t* payload_out, uint8_t* frames_out, uint32_t* iterations,
                                    uint8_t* syndromes_match, uint32_t* corrected) {
    DecodeArgs a{};
    a.pinf = std::numeric_limits<float>::infinity();
    a.n_frames = (uint32_t)n_frames;
    a.max_it = max_iterations;
    a.thr = msg_threshold;
    a.clamp_on = (flags & QKD_FLAG_THRESHOLD) ? 1 : 0;
    a.log_p = std::log((1. - qber) / qber);    // as qkd_reconcile_batch (decode_keys)
    a.known = known_llr;
    a.syn = syndrome;
    a.bits_out = frames_out;
    a.payload_out = payload_out;
    a.n_payload = (uint32_t)ad->n_payload;
    a.flips = corrected;
    a.iters = iterations;
    a.sp_ok = syndromes_match;
    a.thr_dn = f32_bound(msg_threshold, false);
    a.thr_up = f32_bound(msg_threshold, true);
    return a;
}

// Key verification of a class-mode call (qkd_reconcile_adaptive_verify_batch,
// qkd_reconcile_blind_verify_batch), as the caller gave it.
struct ClassVerify {
    uint64_t seed;
    const uint64_t* words;
    uint32_t tag_bits;
    const uint64_t* alice_tags;
    uint64_t* tags_out;
    uint8_t* verified;
};

// The key string of a verifying class-mode call, once per call: the caller's
// words as they are, or the seed's expansion into the workspace's buffer
// (grow-on-demand; one small launch on the stream).
static qkd_status class_verify_key(qkd_workspace* ws, const qkd_adapt* ad, const ClassVerify& cv, hipStream_t stream,
                                   const uint64_t** key) {
    if (cv.words) {
        *key = cv.words;
        return QKD_OK;
    }
    const size_t words = qkdv::verify_key_words(ad->n_payload);
    if (ws->vkey.reserve(words) != hipSuccess)
        return set_error(QKD_ERR_OUT_OF_MEMORY, "workspace: cannot allocate the verification key string");
    QKD_HIP(launch_verify_expand(cv.seed, (uint32_t)words, ws->vkey, stream));
    *key = ws->vkey;
    return QKD_OK;
}

static void class_verify_into(DecodeArgs& a, const ClassVerify& cv, const uint64_t* key) {
    a.vkey = key;
    a.vmask = qkdv::verify_tag_mask(cv.tag_bits);
    a.valice = cv.alice_tags;
    a.vtags = cv.tags_out;
    a.vok = cv.verified;
}

// qkd_reconcile_adaptive_batch and qkd_reconcile_adaptive_verify_batch after
// their argument checks; cv: the second's tags, nullptr for the first.
static qkd_status adaptive_run(const char* entry, const qkd_code* c, qkd_workspace* ws, const qkd_adapt* ad,
                               const uint8_t* bob_payload, const uint8_t* syndrome, size_t n_frames, double qber,
                               double known_llr, uint32_t max_iterations, double msg_threshold, uint32_t flags,
                               uint8_t* payload_out, uint8_t* frames_out, uint32_t* iterations,
                               uint8_t* syndromes_match, uint32_t* corrected, const ClassVerify* cv, void* stream) {
    if (ad->code != c) return set_error(QKD_ERR_INVALID_ARG, "the plan was created for another code");
    if (!(known_llr > 0.0) || !std::isfinite(known_llr))
        return set_error(QKD_ERR_INVALID_ARG, "known_llr must be finite and > 0");
    // QKD_FLAG_ERASURES is implied; the decode parameters as qkd_reconcile_batch
    qkd_status s = check_decode_params(max_iterations, msg_threshold, flags & ~QKD_FLAG_ERASURES);
    if (s != QKD_OK) return s;
    if ((flags & QKD_VARIANT_MASK) != QKD_VARIANT_SP_F64)
        return set_error(QKD_ERR_UNSUPPORTED, "%s: QKD_VARIANT_SP_F64 only", entry);
    DeviceGuard g(c->device);
    ws = resolve_ws(c, ws);
    if (!ws) return set_error(QKD_ERR_OUT_OF_MEMORY, "no workspace");
    WsSession sess(ws, (hipStream_t)stream);
    s = ws_reserve_classes(ws, n_frames);
    if (s != QKD_OK) return s;
    DecodeArgs a = class_decode_args(ad, syndrome, n_frames, qber, known_llr, max_iterations, msg_threshold, flags,
                                     payload_out, frames_out, iterations, syndromes_match, corrected);
    if (cv) {
        const uint64_t* key = nullptr;
        s = class_verify_key(ws, ad, *cv, (hipStream_t)stream, &key);
        if (s != QKD_OK) return s;
        class_verify_into(a, *cv, key);
    }
    const ClassArgs ca{ad->d_src_orig, ad->d_src_int, bob_payload, ws->cls};
    return launch_decode(c, ws, a, kModeClass, flags & ~QKD_FLAG_ERASURES, (hipStream_t)stream,
                         DecodeIo{nullptr, nullptr, &ca});
}

qkd_status qkd_reconcile_adaptive_batch(const qkd_code* c, qkd_workspace* ws, const qkd_adapt* ad,
                                        const uint8_t* bob_payload, const uint8_t* syndrome, size_t n_frames,
                                        double qber, double known_llr, uint32_t max_iterations,
                                        double msg_threshold, uint32_t flags, uint8_t* payload_out,
                                        uint8_t* frames_out, uint32_t* iterations, uint8_t* syndromes_match,
                                        uint32_t* corrected, void* stream) {
    clear_error();
    if (const char* bad = qkda::reconcile_args_error(c, bob_payload, syndrome, n_frames, qber, payload_out,
                                                     iterations, syndromes_match))
        return set_error(QKD_ERR_INVALID_ARG, "%s", bad);
    if (!ad) return set_error(QKD_ERR_INVALID_ARG, "null argument");
    return adaptive_run("qkd_reconcile_adaptive_batch", c, ws, ad, bob_payload, syndrome, n_frames, qber, known_llr,
                        max_iterations, msg_threshold, flags, payload_out, frames_out, iterations, syndromes_match,
                        corrected, nullptr, stream);
}

qkd_status qkd_reconcile_adaptive_verify_batch(const qkd_code* c, qkd_workspace* ws, const qkd_adapt* ad,
                                               const uint8_t* bob_payload, const uint8_t* syndrome, size_t n_frames,
                                               double qber, double known_llr, uint32_t max_iterations,
                                               double msg_threshold, uint32_t flags, uint8_t* payload_out,
                                               uint8_t* frames_out, uint32_t* iterations, uint8_t* syndromes_match,
                                               uint32_t* corrected, uint64_t hash_seed, const uint64_t* hash_words,
                                               uint32_t tag_bits, const uint64_t* alice_tags, uint64_t* tags_out,
                                               uint8_t* verified, void* stream) {
    clear_error();
    const char* bad = qkda::reconcile_args_error(c, bob_payload, syndrome, n_frames, qber, payload_out, iterations,
                                                 syndromes_match);
    if (!bad) bad = qkda::reconcile_adaptive_verify_args_error(ad, tag_bits, alice_tags, tags_out, verified);
    if (bad) return set_error(QKD_ERR_INVALID_ARG, "%s", bad);
    const ClassVerify cv{hash_seed, hash_words, tag_bits, alice_tags, tags_out, verified};
    return adaptive_run("qkd_reconcile_adaptive_verify_batch", c, ws, ad, bob_payload, syndrome, n_frames, qber,
                        known_llr, max_iterations, msg_threshold, flags, payload_out, frames_out, iterations,
                        syndromes_match, corrected, &cv, stream);
}

// qkd_reconcile_blind_batch and qkd_reconcile_blind_verify_batch after their
// argument checks; cv: the second's tags, nullptr for the first.
static qkd_status blind_run(const char* entry, const qkd_code* c, qkd_workspace* ws, const qkd_adapt* ad,
                            const uint8_t* bob_payload, const uint8_t* syndrome, size_t n_frames, double qber,
                            double known_llr, uint32_t max_iterations, double msg_threshold, uint32_t flags,
                            const uint8_t* revealed, uint32_t* n_revealed, const uint8_t* skip, uint32_t step,
                            uint32_t max_rounds, uint8_t* payload_out, uint8_t* frames_out, uint32_t* iterations,
                            uint8_t* syndromes_match, uint32_t* corrected, uint32_t* rounds, const ClassVerify* cv,
                            void* stream) {
    if (ad->code != c) return set_error(QKD_ERR_INVALID_ARG, "the plan was created for another code");
    if (const char* bad = qkda::reconcile_blind_revealed_error(ad->p, revealed))
        return set_error(QKD_ERR_INVALID_ARG, "%s", bad);
    if (!(known_llr > 0.0) || !std::isfinite(known_llr))
        return set_error(QKD_ERR_INVALID_ARG, "known_llr must be finite and > 0");
    qkd_status s = check_decode_params(max_iterations, msg_threshold, flags & ~QKD_FLAG_ERASURES);
    if (s != QKD_OK) return s;
    if ((flags & QKD_VARIANT_MASK) != QKD_VARIANT_SP_F64)
        return set_error(QKD_ERR_UNSUPPORTED, "%s: QKD_VARIANT_SP_F64 only", entry);
    DeviceGuard g(c->device);
    ws = resolve_ws(c, ws);
    if (!ws) return set_error(QKD_ERR_OUT_OF_MEMORY, "no workspace");
    WsSession sess(ws, (hipStream_t)stream);
    s = ws_reserve_classes(ws, n_frames);
    if (s != QKD_OK) return s;
    s = ws_reserve_decode(ws, 0);             // (the counter words)
    if (s != QKD_OK) return s;
    if (ws->blind_frames < n_frames) {
        ws->blind_frames = 0;
        if (ws->blind_list.reserve(n_frames) != hipSuccess || ws->blind_open.reserve(n_frames) != hipSuccess)
            return set_error(QKD_ERR_OUT_OF_MEMORY, "workspace: cannot allocate the open-frame list");
        ws->blind_frames = n_frames;
    }
    // counter word 4: the round's open frames ([0..3]: the decoders' queues)
    uint32_t* const count = ws->counter + 4;
    const BlindArgs ba{ad->d_rank_orig, ad->d_rank_int, revealed, n_revealed, (uint32_t)ad->p, ws->blind_list, count};
    ClassArgs ca{ad->d_src_orig, ad->d_src_int, bob_payload, ws->cls};
    ca.blind = &ba;
    const uint64_t* vkey = nullptr;
    if (cv) {
        s = class_verify_key(ws, ad, *cv, (hipStream_t)stream, &vkey);
        if (s != QKD_OK) return s;
    }
    // every round: settle the round before and list the open frames, then
    // their class bytes and the decoder over the list (launch_decode), all on
    // the stream; the host never learns how many frames a round has
    // (a frame is decoded at most 1 + ceil(p / step) times: later rounds would find no open frame)
    const uint64_t useful = step ? 1 + ((uint64_t)ad->p + step - 1) / step : 1;
    const uint32_t n_rounds = (uint32_t)std::min<uint64_t>(max_rounds, useful);
    for (uint32_t t = 0; t < n_rounds; ++t) {
        // (closed: verified when Alice's tags are given, else matched)
        const BlindRound br{t, (uint32_t)n_frames, (uint32_t)ad->p, step, skip, syndromes_match, n_revealed, rounds,
                            ws->blind_open, ws->blind_list, count, (cv && cv->alice_tags) ? cv->verified : nullptr};
        QKD_HIP(launch_blind_round(br, (hipStream_t)stream));
        DecodeArgs a = class_decode_args(ad, syndrome, n_frames, qber, known_llr, max_iterations, msg_threshold,
                                         flags, payload_out, frames_out, iterations, syndromes_match, corrected);
        a.frame_list = ws->blind_list;
        a.frame_count = count;
        if (cv) class_verify_into(a, *cv, vkey);
        s = launch_decode(c, ws, a, kModeClass, flags & ~QKD_FLAG_ERASURES, (hipStream_t)stream,
                          DecodeIo{nullptr, nullptr, &ca});
        if (s != QKD_OK) return s;
    }
    return QKD_OK;
}

qkd_status qkd_reconcile_blind_batch(const qkd_code* c, qkd_workspace* ws, const qkd_adapt* ad,
                                     const uint8_t* bob_payload, const uint8_t* syndrome, size_t n_frames,
                                     double qber, double known_llr, uint32_t max_iterations, double msg_threshold,
                                     uint32_t flags, const uint8_t* revealed, uint32_t* n_revealed,
                                     const uint8_t* skip, uint32_t step, uint32_t max_rounds, uint8_t* payload_out,
                                     uint8_t* frames_out, uint32_t* iterations, uint8_t* syndromes_match,
                                     uint32_t* corrected, uint32_t* rounds, void* stream) {
    clear_error();
    if (const char* bad = qkda::reconcile_args_error(c, bob_payload, syndrome, n_frames, qber, payload_out,
                                                     iterations, syndromes_match))
        return set_error(QKD_ERR_INVALID_ARG, "%s", bad);
    if (const char* bad = qkda::reconcile_blind_args_error(ad, n_revealed, step, max_rounds))
        return set_error(QKD_ERR_INVALID_ARG, "%s", bad);
    return blind_run("qkd_reconcile_blind_batch", c, ws, ad, bob_payload, syndrome, n_frames, qber, known_llr,
                     max_iterations, msg_threshold, flags, revealed, n_revealed, skip, step, max_rounds, payload_out,
                     frames_out, iterations, syndromes_match, corrected, rounds, nullptr, stream);
}

qkd_status qkd_reconcile_blind_verify_batch(const qkd_code* c, qkd_workspace* ws, const qkd_adapt* ad,
                                            const uint8_t* bob_payload, const uint8_t* syndrome, size_t n_frames,
                                            double qber, double known_llr, uint32_t max_iterations,
                                            double msg_threshold, uint32_t flags, const uint8_t* revealed,
                                            uint32_t* n_revealed, const uint8_t* skip, uint32_t step,
                                            uint32_t max_rounds, uint8_t* payload_out, uint8_t* frames_out,
                                            uint32_t* iterations, uint8_t* syndromes_match, uint32_t* corrected,
                                            uint32_t* rounds, uint64_t hash_seed, const uint64_t* hash_words,
                                            uint32_t tag_bits, const uint64_t* alice_tags, uint64_t* tags_out,
                                            uint8_t* verified, void* stream) {
    clear_error();
    const char* bad = qkda::reconcile_args_error(c, bob_payload, syndrome, n_frames, qber, payload_out, iterations,
                                                 syndromes_match);
    if (!bad)
        bad = qkda::reconcile_blind_verify_args_error(ad, n_revealed, step, max_rounds, tag_bits, alice_tags,
                                                      tags_out, verified);
    if (bad) return set_error(QKD_ERR_INVALID_ARG, "%s", bad);
    const ClassVerify cv{hash_seed, hash_words, tag_bits, alice_tags, tags_out, verified};
    return blind_run("qkd_reconcile_blind_verify_batch", c, ws, ad, bob_payload, syndrome, n_frames, qber, known_llr,
                     max_iterations, msg_threshold, flags, revealed, n_revealed, skip, step, max_rounds, payload_out,
                     frames_out, iterations, syndromes_match, corrected, rounds, &cv, stream);
}

qkd_status qkd_reconcile_verify_batch(const qkd_code* c, qkd_workspace* ws, const uint8_t* bob,
                                      const uint8_t* syndrome, size_t n_frames, double qber,
                                      uint32_t max_iterations, double msg_threshold, uint32_t flags,
                                      uint8_t* bits_out, uint32_t* iterations, uint8_t* syndromes_match,
                                      uint32_t* corrected, uint64_t hash_seed, const uint64_t* hash_words,
                                      uint32_t tag_bits, const uint64_t* alice_tags, uint64_t* tags_out,
                                      uint8_t* verified, void* stream) {
    clear_error();
    const char* bad = qkda::reconcile_args_error(c, bob, syndrome, n_frames, qber, bits_out, iterations,
                                                 syndromes_match);
    if (!bad) bad = qkda::reconcile_verify_args_error(tag_bits, alice_tags, tags_out, verified);
    if (bad) return set_error(QKD_ERR_INVALID_ARG, "%s", bad);
    const VerifyArgs v = verify_args(c, hash_seed, hash_words, tag_bits, alice_tags, tags_out, verified,
                                     syndromes_match);
    return reconcile_run(c, ws, bob, syndrome, n_frames, qber, max_iterations, msg_threshold, flags, bits_out,
                         iterations, syndromes_match, corrected, &v, stream);
}

qkd_status qkd_interactive_batch(const qkd_code* c, qkd_workspace* ws, uint64_t simulation_seed, size_t n_points,
                                 const double* q_nominal, uint32_t max_iterations, double msg_threshold,
                                 uint32_t flags, uint32_t* iterations, uint8_t* syndromes_match,
                                 uint8_t* keys_match, double* exact_qber, uint32_t* errors, size_t* points_done) {
    clear_error();
    if (!c || !q_nominal || !iterations || !syndromes_match || !keys_match || !exact_qber || !errors || !points_done)
        return set_error(QKD_ERR_INVALID_ARG, "null argument");
    *points_done = 0;
    if (n_points == 0 || n_points > (1u << 20)) return set_error(QKD_ERR_INVALID_ARG, "bad point count");
    qkd_status s = check_decode_params(max_iterations, msg_threshold, flags);
    if (s != QKD_OK) return s;
    // the reference throws at the first point whose exact QBER is 0 (:105-111),
    // after running the points before it
    std::vector<uint32_t> ne;
    uint32_t max_ne = 1;
    size_t run = n_points;
    for (size_t p = 0; p < n_points; ++p) {
        // (decoded points: log((1 - q) / q) must be finite, as qkd_qkd_ldpc_batch requires)
        if (!(q_nominal[p] > 0.0 && q_nominal[p] < 1.0)) return set_error(QKD_ERR_INVALID_ARG, "QBER must be in (0,1)");
        const uint64_t e = qkdr::num_errors((uint32_t)c->n, q_nominal[p]);
        if (e == 0) {
            run = p;
            break;
        }
        ne.push_back((uint32_t)e);
        max_ne = std::max(max_ne, (uint32_t)e);
    }
    DeviceGuard g(c->device);
    ws = resolve_ws(c, ws);
    if (!ws) return set_error(QKD_ERR_OUT_OF_MEMORY, "no workspace");
    hipStream_t st = nullptr;
    if (run > 0) {
        WsSession sess(ws, st);
        s = ws_reserve_keys(ws, 1, 1);
        if (s != QKD_OK) return s;
        const uint32_t words = (uint32_t)((c->n + 63) / 64);
        DevBuf<uint64_t> d_a, d_b;
        DevBuf<uint32_t> d_ne, d_low, d_it;
        DevBuf<uint8_t> d_flags;
        if (d_a.alloc(run * words) != hipSuccess || d_b.alloc(run * words) != hipSuccess ||
            d_ne.alloc(run) != hipSuccess || d_low.alloc(max_ne) != hipSuccess || d_it.alloc(run) != hipSuccess ||
            d_flags.alloc(run * 2) != hipSuccess)
            return set_error(QKD_ERR_OUT_OF_MEMORY, "interactive: cannot allocate");
        hipError_t e = hipMemcpy(d_ne, ne.data(), run * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(keygen_stream_kernel, dim3(1), dim3(64), 0, st, simulation_seed, (uint32_t)c->n, words,
                               (uint32_t)run, d_ne.get(), d_a.get(), d_b.get(), d_low.get());
            e = hipGetLastError();
        }
        for (size_t p = 0; p < run && e == hipSuccess && s == QKD_OK; ++p) {
            exact_qber[p] = (double)ne[p] / (double)c->n;
            errors[p] = ne[p];   // distinct positions: every flip is a differing bit (:115-119)
            e = hipMemcpyAsync(ws->alice_w, d_a + p * words, words * 8, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(ws->bob_w, d_b + p * words, words * 8, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess)
                s = decode_keys(c, ws, 1, exact_qber[p], max_iterations, msg_threshold, flags, nullptr, d_it + p,
                                d_flags + p, d_flags + run + p, st);
        }
        if (e == hipSuccess && s == QKD_OK) e = hipMemcpy(iterations, d_it, run * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && s == QKD_OK) e = hipMemcpy(syndromes_match, d_flags, run, hipMemcpyDeviceToHost);
        if (e == hipSuccess && s == QKD_OK) e = hipMemcpy(keys_match, d_flags + run, run, hipMemcpyDeviceToHost);
        if (s != QKD_OK) return s;
        if (e != hipSuccess) return set_error(QKD_ERR_DEVICE, "interactive: %s", hipGetErrorString(e));
    }
    *points_done = run;
    if (run < n_points) {
        exact_qber[run] = 0.0;
        return set_error(QKD_ERR_QBER_TOO_SMALL, "Key size '%d' is too small for QBER.", c->n);
    }
    return QKD_OK;
}

qkd_status qkd_trace_decode(const qkd_code* c, const double* llr, const uint8_t* syndrome,
                            uint32_t max_iterations, double msg_threshold, uint32_t flags,
                            double* c2b_trace, double* total_trace, uint32_t* iterations,
                            uint8_t* syndrome_match) {
    clear_error();
    if (!c || !llr || !syndrome || !iterations || !syndrome_match)
        return set_error(QKD_ERR_INVALID_ARG, "null argument");
    qkd_status s = check_decode_params(max_iterations, msg_threshold, flags);
    if (s != QKD_OK) return s;
    if ((flags & QKD_VARIANT_MASK) != QKD_VARIANT_SP_F64)
        return set_error(QKD_ERR_UNSUPPORTED, "trace is provided for the reference rule (QKD_VARIANT_SP_F64) only");
    DeviceGuard g(c->device);
    qkd_workspace* ws = qkd_workspace_create(c, &s);
    if (!ws) return s;
    const size_t stride = (size_t)c->max_dv * c->n_pad + c->n_pad;
    const std::unique_ptr<qkd_workspace> ws_owner(ws);
    DevBuf<double> d_llr, d_tr;
    DevBuf<uint8_t> d_syn, d_ok;
    DevBuf<uint32_t> d_it;
    hipStream_t st = nullptr;
    if (d_llr.alloc((size_t)c->n) != hipSuccess || d_syn.alloc((size_t)c->m) != hipSuccess ||
        d_ok.alloc(1) != hipSuccess || d_it.alloc(1) != hipSuccess ||
        d_tr.alloc(stride * max_iterations) != hipSuccess)
        return set_error(QKD_ERR_OUT_OF_MEMORY, "trace: cannot allocate %zu B", stride * max_iterations * 8);
    std::vector<uint8_t> syn01((size_t)c->m);
    for (int32_t j = 0; j < c->m; ++j) syn01[j] = syndrome[j] ? 1 : 0;
    hipError_t e = hipMemcpy(d_llr, llr, (size_t)c->n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_syn, syn01.data(), (size_t)c->m, hipMemcpyHostToDevice);
    if (e != hipSuccess) return set_error(QKD_ERR_DEVICE, "trace: %s", hipGetErrorString(e));
    DecodeArgs a{};
    a.pinf = std::numeric_limits<float>::infinity();
    a.n_frames = 1;
    a.max_it = max_iterations;
    a.thr = msg_threshold;
    a.clamp_on = (flags & QKD_FLAG_THRESHOLD) ? 1 : 0;
    a.llr = d_llr;
    a.syn = d_syn;
    a.iters = d_it;
    a.sp_ok = d_ok;
    a.trace = d_tr;
    a.trace_stride = stride;
    s = launch_decode(c, ws, a, kModeLlr, flags, st);
    if (s == QKD_OK) {
        std::vector<double> tr(stride * max_iterations);
        e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(iterations, d_it, 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(syndrome_match, d_ok, 1, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(tr.data(), d_tr, tr.size() * 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            s = set_error(QKD_ERR_DEVICE, "trace: %s", hipGetErrorString(e));
        } else {
            // bit-major jagged order of the reference's check_to_bit_msg rows
            const size_t nm = (size_t)c->max_dv * c->n_pad;
            for (uint32_t t = 0; t < *iterations; ++t) {
                const double* src = tr.data() + t * stride;
                if (c2b_trace)
                    for (int32_t i = 0; i < c->n; ++i)
                        for (int32_t k = 0; k < c->bit_ptr[i + 1] - c->bit_ptr[i]; ++k)
                            c2b_trace[(size_t)t * c->e + c->bit_ptr[i] + k] = src[(size_t)k * c->n_pad + i];
                if (total_trace)
                    for (int32_t i = 0; i < c->n; ++i) total_trace[(size_t)t * c->n + i] = src[nm + i];
            }
        }
    }
    return s;
}

qkd_status qkd_trials_batch(const qkd_code* c, qkd_workspace* ws, const uint64_t* seeds,
                            uint64_t seed_offset, size_t n_frames, double q_nominal,
                            uint32_t max_iterations, double msg_threshold, uint32_t flags,
                            uint32_t* iterations, uint8_t* syndromes_match, uint8_t* keys_match,
                            double* exact_qber, qkd_counters* counters, void* stream) {
    clear_error();
    if (!c || !seeds || !iterations || !syndromes_match)
        return set_error(QKD_ERR_INVALID_ARG, "null argument");
    qkd_status s = check_frames(n_frames);
    if (s == QKD_OK) s = check_decode_params(max_iterations, msg_threshold, flags);
    if (s != QKD_OK) return s;
    // (the keys are decoded: log((1 - q) / q) must be finite, as qkd_qkd_ldpc_batch requires)
    if (!(q_nominal > 0.0 && q_nominal < 1.0)) return set_error(QKD_ERR_INVALID_ARG, "QBER must be in (0,1)");
    DeviceGuard g(c->device);
    ws = resolve_ws(c, ws);
    if (!ws) return set_error(QKD_ERR_OUT_OF_MEMORY, "no workspace");
    WsSession sess(ws, (hipStream_t)stream);
    s = keygen_into_ws(c, ws, seeds, seed_offset, n_frames, q_nominal, exact_qber, (hipStream_t)stream);
    if (s != QKD_OK) return s;
    const double q = (double)qkdr::num_errors((uint32_t)c->n, q_nominal) / (double)c->n;
    s = decode_keys(c, ws, n_frames, q, max_iterations, msg_threshold, flags, nullptr, iterations,
                    syndromes_match, keys_match, (hipStream_t)stream);
    if (s != QKD_OK) return s;
    if (counters) QKD_HIP(launch_counters(iterations, syndromes_match, keys_match, n_frames, counters,
                                          (hipStream_t)stream));
    return QKD_OK;
}

}  // extern "C"
