// launch.hip — the workspace and the decode launch; no kernels.
//
// The reference's per-trial decode call (QKD_LDPC_*, src/qkd_ldpc_algorithm.cpp:347-447,
// from run_trial, src/simulation.cpp:161-189) becomes one launch per batch in
// three stages: choose (qkd_launch.h, plain C++), prepare (kernels, resident
// workgroups, workspace buffers, the encoded plan), launch (launch_prepared:
// the kernels of decode.hip, decode_split.hip, decode_ilv.hip and the ones
// around them, frame_syn.hip, frame_out.hip, bits.hip, adapt.hip). Workgroups
// are persistent (grid = resident workgroups) and pull frames from a device
// queue. Also here: the workspace's buffers and lifetime, the per-stream
// session (qkd_host.h WsSession) and the decoder-timing events.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "qkd_decode.h"
#include "qkd_host.h"

namespace qkd {

// Workgroups of `block` threads and `lds` bytes of fn that can be resident on
// the code's device (0: none). (The attribute on every launch, for the current
// device: no process-wide flag to race on or to skip for a second device.)
static qkd_status resident_grid(const qkd_code* c, DecodeFn fn, int block, size_t lds, int* grid) {
    QKD_HIP(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int per_cu = 0;
    QKD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)fn, block, lds));
    *grid = per_cu * c->cu_count;
    return QKD_OK;
}
// ... of decode_kernel or decode_split_kernel, which must have one
static qkd_status decode_grid(const qkd_code* c, DecodeFn fn, size_t lds, int* grid) {
    const qkd_status s = resident_grid(c, fn, kDecodeBlock, lds, grid);
    if (s == QKD_OK && *grid < 1)
        return set_error(QKD_ERR_UNSUPPORTED, "decode kernel cannot be resident (LDS %zu B)", lds);
    return s;
}

qkd_status ws_reserve_decode(qkd_workspace* ws, size_t slots) {
    const qkd_code* c = ws->code;
    if (!ws->counter) {
        QKD_HIP(ws->counter.alloc(32));
        QKD_HIP(hipMemset(ws->counter, 0, 128));
    }
    // per slot: the c2b store (max_dv rows) and, at the end, a total row
    // (large codes keep their bit totals there)
    const size_t elems = slots * ((size_t)c->max_dv + 1) * c->n_pad;
    if (ws->c2b.reserve(elems) != hipSuccess)
        return set_error(QKD_ERR_OUT_OF_MEMORY, "workspace: cannot allocate %zu B of c2b scratch",
                         elems * sizeof(double));
    return QKD_OK;
}

qkd_status ws_reserve_keys(qkd_workspace* ws, size_t frames, size_t low_words) {
    const qkd_code* c = ws->code;
    const size_t words = (size_t)(c->n + 63) / 64;
    if (ws->key_frames < frames) {
        ws->key_frames = 0;
        const size_t syn_words = 2 * (size_t)decode_m_words(c->m);
        if (ws->alice_w.reserve(frames * words) != hipSuccess || ws->bob_w.reserve(frames * words) != hipSuccess ||
            ws->synw.reserve(frames * syn_words) != hipSuccess || ws->zout.reserve(frames * words) != hipSuccess)
            return set_error(QKD_ERR_OUT_OF_MEMORY, "workspace: cannot allocate keys for %zu frames", frames);
        ws->key_frames = frames;
    }
    if (ws->low.reserve(low_words) != hipSuccess)
        return set_error(QKD_ERR_OUT_OF_MEMORY, "workspace: cannot allocate shuffle scratch");
    return QKD_OK;
}

}  // namespace qkd

qkd_workspace::~qkd_workspace() {
    qkd::DeviceGuard g(device);
    if (spec_stat_ev) (void)hipEventSynchronize(spec_stat_ev);
    if (spec_stat_host) (void)hipHostFree(spec_stat_host);
    if (spec_stat_ev) (void)hipEventDestroy(spec_stat_ev);
    if (done) (void)hipEventDestroy(done);
    for (hipEvent_t e : dec_ev) (void)hipEventDestroy(e);
}

namespace qkd {

static std::mutex g_default_ws_mu;

qkd_workspace* resolve_ws(const qkd_code* code, qkd_workspace* ws) {
    if (ws) return ws;
    std::lock_guard<std::mutex> lk(g_default_ws_mu);
    if (!code->default_ws) {
        qkd_status s;
        const_cast<qkd_code*>(code)->default_ws = qkd_workspace_create(code, &s);
    }
    return code->default_ws;
}

unsigned blocks_for(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

// qkd_debug_decoder_timing: one event recorded on the launch stream before
// and one after each decoder kernel while timing is on (events pooled per ws;
// at kDecEvPairsMax recorded pairs the finished ones are folded into a running
// total, so the pool stays bounded)
static constexpr size_t kDecEvPairsMax = 256;
hipError_t decoder_events_fold(qkd_workspace* ws) {
    const size_t pairs = ws->dec_ev_used / 2;
    // summed locally and committed only once every pair has been read: a failure
    // part-way leaves the totals and the pool as they were (a retry folds the
    // same pairs once, not twice)
    double ms_sum = 0.0;
    for (size_t k = 0; k < pairs; ++k) {
        hipError_t r = hipEventSynchronize(ws->dec_ev[2 * k + 1]);
        float ms = 0.0f;
        if (r == hipSuccess) r = hipEventElapsedTime(&ms, ws->dec_ev[2 * k], ws->dec_ev[2 * k + 1]);
        if (r != hipSuccess) return r;
        ms_sum += ms;
    }
    ws->dec_ms_folded += ms_sum;
    ws->dec_pairs_folded += pairs;
    ws->dec_ev_used = 0;
    return hipSuccess;
}
// the start event of a launch (stop: decoder_event_close)
static hipError_t decoder_event(qkd_workspace* ws, hipStream_t stream) {
    if (!ws->time_decoder) return hipSuccess;
    if (ws->dec_ev_used >= 2 * kDecEvPairsMax) {
        const hipError_t r = decoder_events_fold(ws);
        if (r != hipSuccess) return r;
    }
    while (ws->dec_ev.size() < ws->dec_ev_used + 2) {
        hipEvent_t e = nullptr;
        const hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return r;
        ws->dec_ev.push_back(e);
    }
    const hipError_t r = hipEventRecord(ws->dec_ev[ws->dec_ev_used], stream);
    if (r == hipSuccess) ws->dec_ev_used++;
    return r;
}
// after the launch: its stop event, or, when the launch (`launch`) or the
// record failed, the start event taken back, so pairs stay (start, stop)
static hipError_t decoder_event_close(qkd_workspace* ws, hipStream_t stream, hipError_t launch) {
    if (!ws->time_decoder) return launch;
    hipError_t r = launch;
    if (r == hipSuccess) r = hipEventRecord(ws->dec_ev[ws->dec_ev_used], stream);
    if (r == hipSuccess) ws->dec_ev_used++;
    else ws->dec_ev_used--;
    return r;
}

// DeviceCode::plan_slot encoded for a split-kernel layout and check-degree
// bucket: slot words by encode_slot (binary64 slots), segment words by
// encode_seg; built on a layout's first launch and kept with the code
// esz 4 (the binary32 min-sum rules, every slot in LDS): the slot word is
// the slot's LDS byte address itself (no kSlotLds tag, no global form)
// cl_form (binary64 slots): 0 the edge-lane plan alone; 1 / 2 followed by the
// split / pure check-lane plan of the code (qkd_code::cl_host): its
// remainder's edge-lane plan, then the check-lane words (qkd_decode.h
// cl_rem_offset, cl_words_offset)
static qkd_status plan_for_layout(const qkd_code* c, const SplitLds& L, int dc, const uint2** out, int esz = 8,
                                  int cl_form = 0) {
    std::lock_guard<std::mutex> lock(c->plan_mu);
    const auto key = std::make_pair(L.S, ((uint32_t)cl_form << 28) | ((uint32_t)L.msg << 8) | (uint32_t)dc | (esz == 4 ? 0x80u : 0u));
    auto it = c->d_plan_enc.find(key);
    if (it == c->d_plan_enc.end()) {
        std::vector<U2> enc(c->plan_slot);
        for (size_t k = 0; k < enc.size(); ++k) {
            U2& w = enc[k];
            w.x = esz == 4 ? (uint32_t)L.msg + w.x * 4u : encode_slot(w.x, L.S, (uint32_t)L.msg, (uint32_t)sizeof(double));
            w.y = encode_seg(w.y & qkdp::kPlanChkMask, (w.y >> 20) & 63u, (w.y >> 26) + 1, (uint32_t)(k & 63),
                             (uint32_t)dc);
        }
        if (cl_form != 0) {
            const ClHost& h = c->cl_host[cl_form - 1];
            const size_t at = enc.size();
            enc.insert(enc.end(), h.rem.begin(), h.rem.end());
            for (size_t k = at; k < enc.size(); ++k) {
                U2& w = enc[k];
                w.x = encode_slot(w.x, L.S, (uint32_t)L.msg, (uint32_t)sizeof(double));
                w.y = encode_seg(w.y & qkdp::kPlanChkMask, (w.y >> 20) & 63u, (w.y >> 26) + 1, (uint32_t)(k & 63),
                                 (uint32_t)dc);
            }
            // per task dc rows of slot words, then the row of check words;
            // entries past a check's degree as the reserved dead word, which
            // must be out of range for this layout's LDS and for the largest
            // region of global slots a launch gives it (choose_decode: the
            // rest rounded up to an odd multiple of kC2bPad, or padded by at
            // most n_pad)
            const size_t slots = (size_t)c->max_dv * c->n_pad;
            if (!slot_dead_ok(L.bytes, slots - L.S + (size_t)c->n_pad + 2 * kC2bPad))
                return set_error(QKD_ERR_UNSUPPORTED, "check-lane plan: the dead slot word is in range of a layout "
                                                      "of %zu B LDS and %zu slots", L.bytes, slots);
            const size_t tasks = h.chk.size() / 64;
            std::vector<uint32_t> words(tasks * (size_t)(dc + 1) * 64);
            for (size_t t = 0; t < tasks; ++t) {
                for (size_t k = 0; k < (size_t)dc * 64; ++k) {
                    const uint32_t x = h.slot[t * (size_t)dc * 64 + k];
                    words[t * (size_t)(dc + 1) * 64 + k] =
                        x == qkdp::kNoSlot ? kSlotDead : encode_slot(x, L.S, (uint32_t)L.msg, (uint32_t)sizeof(double));
                }
                for (size_t l = 0; l < 64; ++l) words[(t * (size_t)(dc + 1) + (size_t)dc) * 64 + l] = h.chk[t * 64 + l];
            }
            words.resize((words.size() + 1) & ~(size_t)1, 0u);
            for (size_t k = 0; k < words.size(); k += 2) enc.push_back(U2{words[k], words[k + 1]});
        }
        DevBuf<uint2> d;
        if (d.alloc(enc.size()) != hipSuccess)
            return set_error(QKD_ERR_OUT_OF_MEMORY, "code: cannot allocate %zu B for an encoded plan",
                             enc.size() * sizeof(uint2));
        if (hipMemcpy(d, enc.data(), enc.size() * sizeof(uint2), hipMemcpyHostToDevice) != hipSuccess)
            return set_error(QKD_ERR_DEVICE, "code: encoded plan upload failed");
        it = c->d_plan_enc.emplace(key, std::move(d)).first;
    }
    *out = it->second;
    return QKD_OK;
}

// The split kernels' encoded slot words are absolute LDS addresses: their
// dynamic LDS must start at address 0, i.e. no static LDS (checked once per
// kernel).
static qkd_status check_no_static_lds(DecodeFn fn) {
    static std::mutex mu;
    static std::map<const void*, size_t> seen;
    std::lock_guard<std::mutex> lock(mu);
    auto it = seen.find((const void*)fn);
    if (it == seen.end()) {
        hipFuncAttributes fa{};
        QKD_HIP(hipFuncGetAttributes(&fa, (const void*)fn));
        it = seen.emplace((const void*)fn, fa.sharedSizeBytes).first;
    }
    if (it->second != 0)
        return set_error(QKD_ERR_UNSUPPORTED, "split decoder with %zu B of static LDS (its slot words "
                                              "address LDS from 0)", it->second);
    return QKD_OK;
}

// The launch path's debug options, read here and nowhere else on it.
static LaunchOptions launch_options(const qkd_workspace* ws) {
    const auto num = [ws](const char* name, bool wide = false) {
        const DbgOpt e = debug_option(ws, name);
        OptInt r;
        r.set = (bool)e;
        if (r.set) r.v = wide ? e.as_long() : (long)e.as_int();
        return r;
    };
    LaunchOptions o;
    if (debug_options_unset(ws)) return o;
    const DbgOpt ms_store = debug_option(ws, "QKD_MINSUM_STORE");
    o.ms_global = ms_store.is("global");
    o.ms_lds = ms_store.is("lds");
    o.classic = debug_option(ws, "QKD_DECODE_KERNEL").is("classic");
    if (const OptInt b = num("QKD_SPLIT_BUDGET", true); b.set) o.split_budget = std::min(kLdsBytesMax, (size_t)b.v);
    o.fold_table = num("QKD_FOLD_TABLE");
    o.spec_always = debug_option(ws, "QKD_SPEC_POLICY").is("always");
    o.decode_grid = num("QKD_DECODE_GRID");
    o.check_lanes = num("QKD_CHECK_LANES");
    o.c2b_pad = num("QKD_C2B_PAD", true);
    o.phase_timing = (bool)debug_option(ws, "QKD_PHASE_TIMING");
    o.ilv = num("QKD_ILV");
    o.ilv_grid = num("QKD_ILV_GRID");
    o.syn_gather = debug_option(ws, "QKD_SYN_SLICED").is("0");
    o.syn_pack_first = debug_option(ws, "QKD_SYN_BYTES").is("0");
    return o;
}

// Stage 1, choose: the facts of the code and of the call, and the decision
// (qkd_launch.h choose_decode). Touches neither the device nor the workspace.
static DecodeChoice choose_launch(const qkd_code* c, const DecodeArgs& a, int mode, uint32_t flags, const DecodeIo& io,
                                  const LaunchOptions& o, bool allow_ilv) {
    const CodeFacts cf = code_facts(*c, c->d_bit_code ? true : false, c->d_ilv_slots ? true : false, c->cu_count);
    LaunchFacts f;
    f.mode = mode;
    f.flags = flags;
    f.n_frames = a.n_frames;
    f.clamp_on = a.clamp_on != 0;
    f.spec_cap = a.spec_cap;
    f.ckpt_unsat = a.ckpt_unsat;
    f.first_table = a.first_table;
    f.tab2_entries = a.tab2_entries;
    f.trace = a.trace != nullptr;
    f.bits_out = a.bits_out != nullptr;
    f.class_verify = a.vkey != nullptr;
    f.adapt = io.adapt != nullptr;
    return choose_decode(cf, f, o, allow_ilv);
}

// What stage 2 hands to stage 3: fn the kernel of kDecodeBlock threads (the
// decoder; with the interleaved decoder ifn, the kernel of its hand-offs)
struct LaunchPlan {
    DecodeFn fn = nullptr, ifn = nullptr;
    int grid = 0, igrid = 0;
    const uint2* plan_enc = nullptr;
};

// Stage 2, prepare: everything of a launch that can fail -- the kernels of
// the choice, their resident workgroups, the workspace's buffers, the encoded
// plan. *no_ilv_memory (with a failure status and no error text): the
// interleaved decoder's message lines could not be allocated (one region per
// resident workgroup: ~6 GB at N = 60,000) and the choice was not forced: the
// caller chooses again without it.
static qkd_status prepare_launch(const qkd_code* c, qkd_workspace* ws, const DecodeChoice& ch, const LaunchOptions& o,
                                 uint32_t n_frames, LaunchPlan& P, bool* no_ilv_memory) {
    const bool split = ch.path != kPathClassic, ilv = ch.path == kPathSplitIlv;
    DecodeFn exact = nullptr;
    if (split) {
        exact = split_kernel(ch.handoff);
        P.fn = ch.decoder == ch.handoff ? exact : split_kernel(ch.decoder);
        if (!exact || !P.fn)
            return set_error(QKD_ERR_UNSUPPORTED, "no split kernel with the erasure rule for this launch");
        if (ilv && !(P.ifn = ilv_kernel(ch.ilv)))
            return set_error(QKD_ERR_UNSUPPORTED, "no interleaved kernel for this launch");
    } else if (!(P.fn = classic_kernel(ch.decoder))) {
        if (ch.decoder.era)
            return set_error(QKD_ERR_UNSUPPORTED, "no classic kernel with the erasure rule for this launch");
        // (a min-sum split rule whose layout a lowered QKD_SPLIT_BUDGET no longer fits)
        return set_error(QKD_ERR_UNSUPPORTED, "no classic kernel for decode rule %d at check-degree bucket %d",
                         ch.decoder.rule, ch.decoder.dc);
    }
    // resident workgroups, at most one per frame
    // (diagnostic: QKD_DECODE_GRID caps them, i.e. the frames in flight)
    const size_t lds = split ? ch.split.bytes : ch.lds_bytes;
    qkd_status s = decode_grid(c, split ? exact : P.fn, lds, &P.grid);
    if (s != QKD_OK) return s;
    P.grid = (int)std::min<size_t>((size_t)P.grid, n_frames);
    if (o.decode_grid.set) P.grid = std::max(1, std::min(P.grid, (int)o.decode_grid.v));
    if (P.fn != exact && split) {
        // (the speculative kernel in the exact one's place: the fewer of the two)
        int sgrid = 0;
        s = decode_grid(c, P.fn, lds, &sgrid);
        if (s != QKD_OK) return s;
        P.grid = std::min(sgrid, P.grid);
    }
    if (ilv) {
        P.fn = exact;
        s = resident_grid(c, P.ifn, kIlvBlock, ch.ilv_lds.bytes, &P.igrid);
        if (s != QKD_OK) return s;
        if (P.igrid < 1) return set_error(QKD_ERR_UNSUPPORTED, "interleaved decoder cannot be resident");
        P.igrid = (int)std::min<size_t>((size_t)P.igrid, ((size_t)n_frames + kIlvCols - 1) / kIlvCols);
        // (QKD_ILV_GRID caps the workgroups: tests take columns through several frames)
        if (o.ilv_grid.set) P.igrid = std::max(1, std::min(P.igrid, (int)o.ilv_grid.v));
    }
    s = ws_reserve_decode(ws, ch.need_c2b ? (size_t)P.grid : 0);
    if (s != QKD_OK) return s;
    if (ch.need_plan) {
        s = plan_for_layout(c, ch.split, ch.bucket, &P.plan_enc, ch.esz, ch.cl_form);
        if (s != QKD_OK) return s;
    }
    if (!ch.dead_ok)
        return set_error(QKD_ERR_UNSUPPORTED, "code too large for the split decoder's slot words "
                                              "(%zu global slots per frame)", ch.c2b_stride);
    const size_t slots = (size_t)c->max_dv * c->n_pad;
    if (ch.need_ckpt && ws->ckpt.reserve((size_t)P.grid * slots) != hipSuccess)
        return set_error(QKD_ERR_OUT_OF_MEMORY, "workspace: cannot allocate %zu B of checkpoints",
                         (size_t)P.grid * slots * sizeof(double));
    if (ch.win_count && ws->win.reserve(2 * (size_t)ch.win_count) != hipSuccess)
        return set_error(QKD_ERR_OUT_OF_MEMORY, "workspace: cannot allocate the policy windows");
    if (ilv) {
        const size_t need = (size_t)P.igrid * ch.istride;
        if (ws->ilv.reserve(need) != hipSuccess) {
            (void)hipGetLastError();
            if (ch.ilv_forced)
                return set_error(QKD_ERR_OUT_OF_MEMORY, "workspace: cannot allocate %zu B of "
                                                        "interleaved message lines", need * sizeof(double));
            *no_ilv_memory = true;
            return QKD_ERR_OUT_OF_MEMORY;
        }
        if (ws->fb_list.reserve(n_frames) != hipSuccess)
            return set_error(QKD_ERR_OUT_OF_MEMORY, "workspace: cannot allocate the hand-off list");
    }
    return ch.need_plan ? check_no_static_lds(P.fn) : QKD_OK;
}

// kModeClass: the class bytes of a launch, in the bit order of the view its
// choice decodes in
static hipError_t launch_classes(DecodeArgs& a, const DecodeChoice& ch, const ClassArgs* adapt, hipStream_t stream) {
    if (ch.decoder.mode != kModeClass) return hipSuccess;
    const bool internal = ch.path != kPathClassic;
    a.src = internal ? adapt->src_int : adapt->src_orig;
    a.cls = adapt->cls;
    // (a round of qkd_reconcile_blind_batch: the frames of its list only)
    if (adapt->blind)
        return launch_blind_classes(a.src, internal ? adapt->blind->rank_int : adapt->blind->rank_orig,
                                    adapt->bob_payload, *adapt->blind, (uint32_t)a.code.n, a.n_payload, a.n_frames,
                                    adapt->cls, stream);
    return launch_adapt_classes(a.src, adapt->bob_payload, (uint32_t)a.code.n, a.n_payload, a.n_frames, adapt->cls,
                                stream);
}

// Stage 3, launch: the arguments' scratch fields from the choice and the
// workspace, then the kernels. Nothing here can fail but a launch itself,
// which matters on the keys path of the split decoders: frame_syn rewrites
// ws->alice_w / bob_w in place in the internal bit order, and after it only
// the decoder (which reads them in that order) may follow.
static qkd_status launch_prepared(const qkd_code* c, qkd_workspace* ws, DecodeArgs& a, uint32_t flags,
                                  const DecodeChoice& ch, const LaunchPlan& P, const LaunchOptions& o,
                                  const DecodeIo& io, hipStream_t stream) {
    const int mode = ch.decoder.mode;
    const bool split = ch.path != kPathClassic;
    a.ms_sc = (flags & QKD_MINSUM_SELF_CORRECT) ? 1 : 0;
    a.ms_scale = minsum_scale_of(flags);
    a.ms_offset = (float)((flags >> QKD_MINSUM_OFFSET_SHIFT) & 0xffu) / 64.0f;
    a.spec_cap = ch.spec_cap;
    a.first_table = ch.first_table;
    a.tab2_entries = ch.tab2_entries;
    a.code = split ? c->view_split() : c->view();      // (split: the internal bit order, qkd_layout.h)
    a.c2b = ws->c2b;
    a.c2b_stride = ch.c2b_stride;
    // the counter words: [0] frame queue, [1] replays, [2] the hand-off queue,
    // [3] the hand-off count; + 64 B the phase clocks, + 120 B spec_replays
    a.counter = ws->counter;
    char* const counter_bytes = reinterpret_cast<char*>(ws->counter.get());
    a.phase = o.phase_timing ? reinterpret_cast<unsigned long long*>(counter_bytes + 64) : nullptr;
    if (ch.cl_report) {
        ws->last_cl_form = ch.cl_form;
        ws->last_cl_tasks = ch.cl_tasks;
        ws->last_cl_rem_tasks = ch.cl_rem_tasks;
    }
    if (!split) {
        QKD_HIP(launch_classes(a, ch, io.adapt, stream));
        // (byte keys: the classic kernel reads them packed, in the original order)
        if (mode == kModeKeys && a.bob_b) QKD_HIP(launch_pack_keys(a, stream));
        // the workspace holds one total row per slot after all the message stores
        a.totals = ch.gt ? ws->c2b + ws->c2b.size() / ((size_t)c->max_dv + 1) * (size_t)c->max_dv : nullptr;
        a.totals_stride = c->n_pad;
        QKD_HIP(hipMemsetAsync(ws->counter, 0, 4, stream));
        if (a.phase) QKD_HIP(hipMemsetAsync(a.phase, 0, 64, stream));
        QKD_HIP(decoder_event(ws, stream));
        hipLaunchKernelGGL(P.fn, dim3(P.grid), dim3(kDecodeBlock), ch.lds_bytes, stream, a);
        QKD_HIP(decoder_event_close(ws, stream, hipGetLastError()));
        // (the classic kernel wrote bits_out itself)
        if (io.corrected)
            QKD_HIP(launch_count_flips(a.bits_out, a.bob_b, (uint32_t)c->n, a.n_frames, io.corrected, stream));
        if (io.verify) QKD_HIP(launch_verify_tags(a.bits_out, (uint32_t)c->n, a.n_frames, *io.verify, stream));
        return QKD_OK;
    }
    a.plan_enc = P.plan_enc;
    a.cl_split = ch.cl_split;
    a.ftab_entries = ch.ftab_entries;
    if (ch.spec_always) a.spec_always = 1u;
    a.lds_budget = ch.lds_budget;
    a.replay_count = ws->counter + 1;
    a.spec_replays = reinterpret_cast<unsigned long long*>(counter_bytes + 120);
    if (ch.need_ckpt) {
        a.ckpt = ws->ckpt;
        a.ckpt_stride = (uint32_t)((size_t)c->max_dv * c->n_pad);
    }
    // the in-launch policy's windows (zeroed below with the queue)
    a.win = ch.win_count ? ws->win.get() : nullptr;
    a.win_count = ch.win_count;
    if (ch.spec) {
        a.win_shift = kSpecWinShift;
        a.win_lag = kSpecWinLag;
    }
    if (a.phase) QKD_HIP(hipMemsetAsync(a.phase, 0, 64, stream));
    // [0] frame queue, [1] replays: zeroed by frame_syn_kernel on the keys
    // path (it runs first on this stream: block 0 writes both words), by a
    // memset otherwise -- one branch, so a keys-mode launch without frame_syn
    // cannot exist
    if (mode == kModeKeys) {
        a.synw = ws->synw;
        a.zout = ws->zout;
        QKD_HIP(launch_frame_syn(a, stream, o.syn_gather, o.syn_pack_first));
    } else {
        QKD_HIP(launch_classes(a, ch, io.adapt, stream));
        QKD_HIP(hipMemsetAsync(ws->counter, 0, 8, stream));
        if (a.win) QKD_HIP(hipMemsetAsync(a.win, 0, 2 * (size_t)a.win_count * sizeof(uint32_t), stream));
    }
    QKD_HIP(decoder_event(ws, stream));
    if (ch.path == kPathSplitIlv) {
        QKD_HIP(hipMemsetAsync(ws->counter + 2, 0, 8, stream));
        DecodeArgs ai = a;
        ai.ilv_store = ws->ilv;
        ai.ilv_stride = ch.istride;
        ai.fb_list = ws->fb_list;
        ai.fb_count = ws->counter + 3;
        hipLaunchKernelGGL(P.ifn, dim3(P.igrid), dim3(kIlvBlock), ch.ilv_lds.bytes, stream, ai);
        // the hand-offs: the split kernel's exact iterations (their
        // intervals could not certify; speculating again measured 1.7x
        // slower), through the frame list
        DecodeArgs af = a;
        af.counter = ws->counter + 2;
        af.frame_list = ws->fb_list;
        af.frame_count = ws->counter + 3;
        af.spec_cap = 0;
        af.spec_always = 1;
        af.phase = nullptr;       // (QKD_PHASE_TIMING: the interleaved kernel's phases)
        // (the interleaved launch's error is read once and carried to
        // decoder_event_close: a failed launch skips the hand-offs and
        // fails the call instead of leaving stale outputs)
        hipError_t le = hipGetLastError();
        if (le == hipSuccess) {
            hipLaunchKernelGGL(P.fn, dim3(P.grid), dim3(kDecodeBlock), ch.split.bytes, stream, af);
            le = hipGetLastError();
        }
        QKD_HIP(decoder_event_close(ws, stream, le));
    } else {
        hipLaunchKernelGGL(P.fn, dim3(P.grid), dim3(kDecodeBlock), ch.split.bytes, stream, a);
        QKD_HIP(decoder_event_close(ws, stream, hipGetLastError()));
    }
    if (mode == kModeKeys) QKD_HIP(launch_key_match(a, stream, io.corrected, io.verify));
    return QKD_OK;
}

// One decode launch: choose, prepare, launch. `a` comes back with the values
// the launch applied (decode_keys reads spec_cap and ckpt_unsat).
qkd_status launch_decode(const qkd_code* c, qkd_workspace* ws, DecodeArgs& a, int mode, uint32_t flags,
                         hipStream_t stream, const DecodeIo& io) {
    const LaunchOptions o = launch_options(ws);
    DecodeChoice ch = choose_launch(c, a, mode, flags, io, o, true);
    if (ch.status != QKD_OK) return set_error(ch.status, "%s", ch.message);
    LaunchPlan P;
    bool no_ilv_memory = false;
    qkd_status s = prepare_launch(c, ws, ch, o, a.n_frames, P, &no_ilv_memory);
    if (no_ilv_memory) {
        // (the split kernel, which needs far less, decodes the batch instead;
        // a long code: the classic kernel)
        ch = choose_launch(c, a, mode, flags, io, o, false);
        if (ch.status != QKD_OK) return set_error(ch.status, "%s", ch.message);
        P = LaunchPlan();
        s = prepare_launch(c, ws, ch, o, a.n_frames, P, &no_ilv_memory);
    }
    if (s != QKD_OK) return s;
    return launch_prepared(c, ws, a, flags, ch, P, o, io, stream);
}

}  // namespace qkd

using namespace qkd;

extern "C" {

qkd_workspace* qkd_workspace_create(const qkd_code* code, qkd_status* status) {
    if (!code) {
        if (status) *status = set_error(QKD_ERR_INVALID_ARG, "null code");
        return nullptr;
    }
    qkd_workspace* ws = new (std::nothrow) qkd_workspace();
    if (!ws) {
        if (status) *status = set_error(QKD_ERR_OUT_OF_MEMORY, "out of host memory");
        return nullptr;
    }
    ws->code = code;
    ws->device = code->device;
    if (status) *status = QKD_OK;
    return ws;
}

void qkd_workspace_destroy(qkd_workspace* ws) {
    if (!ws) return;
    delete ws;
}

}  // extern "C"
