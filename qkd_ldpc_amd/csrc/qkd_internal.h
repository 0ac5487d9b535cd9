// qkd_internal.h — shared definitions of the HIP library (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/qkd_ldpc.h"
#include "qkd_device.h"
#include "qkd_launch.h"
#include "qkd_layout.h"

namespace qkd {

static_assert(sizeof(U2) == sizeof(uint2) && alignof(U2) <= alignof(uint2), "U2 is uint2's layout");

// Device-resident, immutable view of H.
//   chk_bits[k * m_pad + j]  bit index of slot k of check j (ascending), -1 pad
//                            (thread-per-check syndrome kernel)
//   plan[s]                  the check-phase wave plan (qkd_plan.h): slot
//                            s = task*64 + lane holds one edge: {bit | row,
//                            check | segment start | degree} (qkd_plan.h)
//   bit_chk[k * n_pad + i]   k-th check of bit i (ascending), -1 pad
//   bit_pos[k * n_pad + i]   position of bit i in that check's ascending row
//                            (LDS min-sum state lookups)
// Slot-major ("ELL") layouts keep lane-consecutive bits on consecutive
// addresses.
struct DeviceCode {
    int32_t n, m, e;
    int32_t n_pad, m_pad;
    int32_t max_dv, max_dc, min_dc;
    int32_t min_dv;
    int32_t n_tasks;
    const int32_t* chk_bits;
    const uint8_t* chk_deg;
    const uint2* plan;            // {bit | row << 24, check | start << 20 | (deg-1) << 26}
    const int32_t* bit_chk;
    const uint8_t* bit_pos;
    const uint8_t* bit_deg;
    // degree patterns of the bits (second-iteration tanh table, decode.hip):
    // bit_pat[i] = pattern of bit i; pat_deg[p * max_dv + k] = degree of the
    // k-th check of pattern p (0 past the bit's degree)
    int32_t n_pat;
    const uint16_t* bit_pat;
    const uint8_t* pat_deg;
    // packed per-bit word (speculative bit phases; nullptr unless M <= 65536,
    // bit degree <= 3 and check degree <= 16): bits 0-15 / 16-31 / 32-47 the
    // bit's checks in ascending order (0 past its degree), 48-49 its degree,
    // 50-53 / 54-57 / 58-61 each check's degree - 1
    const uint64_t* bit_code;
    // plan with the message slot row * n_pad + bit in place of {bit, row}
    // (split kernels: their message store is slot-addressed)
    const uint2* plan_slot;
    // The split kernels' view (qkd_code::view_split) numbers bits in an
    // internal order (qkd_layout.h internal_bit_order): bit_chk, bit_deg, bit_pat,
    // bit_code and plan_slot are indexed by internal bit q, whose original
    // bit is perm[q]; inv[bit] = q. nullptr in the classic kernels' view
    // (original order). bit_code and plan_slot exist in the internal order only.
    const int32_t* perm;
    const int32_t* inv;
    // frame_syn_sliced_kernel (split view, N < 65535, check degree <= 16;
    // else nullptr): chk_rows16[j * chk_rs + k] = bit k of check j (0xffff
    // past the row; chk_rs 8 or 16)
    const uint16_t* chk_rows16;
    int32_t chk_rs;
    // the frame-interleaved decoder (decode_ilv.hip; split view, bit_code
    // present, check degree <= 16): ilv_slots[j * ilv_rs + k] = the message
    // line (row * n_pad + internal bit) of the k-th edge of check j, ~0 past
    // its degree (ilv_rs 8 or 16); nullptr otherwise
    const uint32_t* ilv_slots;
    int32_t ilv_rs;
    // chk_odd[w] bit b = deg(check 32 w + b) & 1, in the split kernels'
    // syndrome-word layout (decode_m_words words; the keys path's running
    // syndrome starts from it, decode_split.hip)
    const uint32_t* chk_odd;
};

}  // namespace qkd

// the speculation policy's record of one QBER (api.hip decode_keys): clean =
// consecutive replay samples under the switch; skip = calls since the last
// sample once clean >= 2 (sampled every kSpecStatEvery calls)
struct SpecClean {
    int clean = 0;
    uint64_t skip = 0;
};

struct qkd_workspace {
    const qkd_code* code = nullptr;
    int device = 0;
    std::mutex mu;
    // qkd_debug_set_option values of this workspace (host.cpp debug_option)
    std::map<std::string, std::string> dbg;
    // decode scratch: one c2b region per resident workgroup
    // (per slot max_dv message rows; after all of them one total row per slot)
    qkd::DevBuf<double> c2b;
    // dynamic frame queue counter (zeroed per launch)
    qkd::DevBuf<uint32_t> counter;
    // the check-phase form of the last split-decoder launch (launch.hip;
    // qkd_debug_check_lanes): QKD_CHECK_LANES' value as applied, its check-lane
    // tasks and the edge-lane tasks of its remainder; -1 before any launch
    int last_cl_form = -1, last_cl_tasks = 0, last_cl_rem_tasks = 0;
    // packed alice / bob keys (uint64 words) for the fused paths
    qkd::DevBuf<uint64_t> alice_w, bob_w;
    size_t key_frames = 0;             // alice_w, bob_w, synw and zout hold this many frames
    // split decoder, keys path: per frame the target and first-product
    // syndrome words (frame_syn.hip) and the hard decision words the decoder
    // leaves for launch_key_match (frame_out.hip); sized with the keys
    qkd::DevBuf<uint32_t> synw;
    qkd::DevBuf<uint64_t> zout;
    // keygen shuffle scratch (ne words per frame)
    qkd::DevBuf<uint32_t> low;
    hipEvent_t done = nullptr;
    // speculation policy across calls (api.hip, decode_keys): the replay
    // count of the last speculative call comes back asynchronously; a QBER
    // point whose frames were replayed too often (kSpecCkptSwitch) switches it
    // and every higher QBER on this workspace to the checkpointed speculation
    uint32_t* spec_stat_host = nullptr;     // pinned: replays of the last call
    hipEvent_t spec_stat_ev = nullptr;
    bool spec_stat_pending = false;
    double spec_stat_q = 0.0;
    size_t spec_stat_frames = 0;
    double spec_ckpt_q = 2.0;
    // per QBER: consecutive samples under the switch (decode_keys samples a
    // QBER with two such samples only every kSpecStatEvery calls)
    std::map<double, SpecClean> spec_clean;
    // checkpointed speculation: one saved message store per resident workgroup
    qkd::DevBuf<double> ckpt;
    // the speculative kernel's in-launch policy windows (DecodeArgs::win)
    qkd::DevBuf<uint32_t> win;
    // the frame-interleaved decoder (decode_ilv.hip): message lines of every
    // resident workgroup (16 frames per 128-byte line), and the frames it
    // hands to the split kernel's exact replays
    qkd::DevBuf<double> ilv;
    qkd::DevBuf<uint32_t> fb_list;
    // qkd_reconcile_adaptive_batch: one class byte per bit and frame (adapt.hip)
    qkd::DevBuf<uint8_t> cls;
    // qkd_reconcile_blind_batch: the open frames of a round (their count is
    // counter word 4) and one open flag per frame
    qkd::DevBuf<uint32_t> blind_list;
    qkd::DevBuf<uint8_t> blind_open;
    size_t blind_frames = 0;           // both hold this many frames
    // qkd_reconcile_adaptive_verify_batch / qkd_reconcile_blind_verify_batch
    // with the seeded key string: its words, expanded once per call
    qkd::DevBuf<uint64_t> vkey;
    // qkd_debug_decoder_timing: while on, HIP events bracket every decoder
    // launch on its stream (pairs recorded, read back on collection)
    bool time_decoder = false;
    std::vector<hipEvent_t> dec_ev;        // start, stop, start, stop, ...
    size_t dec_ev_used = 0;
    double dec_ms_folded = 0.0;            // finished pairs folded in (pool bound)
    uint64_t dec_pairs_folded = 0;

    // the events and the pinned word, with the workspace's device current
    // (launch.hip); the buffers free themselves
    ~qkd_workspace();
};

// the host-kept layout (qkd_layout.h CodeHost) and its device copies
struct qkd_code : qkd::CodeHost {
    int device = 0;
    qkd::DevBuf<int32_t> d_chk_bits, d_bit_chk;
    qkd::DevBuf<uint8_t> d_chk_deg, d_bit_pos, d_bit_deg;
    qkd::DevBuf<uint2> d_plan, d_plan_slot;
    // the slot plan's encoded forms by LDS layout ((S, message base) -> device
    // copy, qkd::plan_for_layout; plan_mu guards the map: workspaces on
    // several threads may share the code)
    mutable std::map<std::pair<uint32_t, uint32_t>, qkd::DevBuf<uint2>> d_plan_enc;
    mutable std::mutex plan_mu;
    qkd::DevBuf<uint16_t> d_bit_pat;
    qkd::DevBuf<uint64_t> d_bit_code;
    qkd::DevBuf<uint8_t> d_pat_deg;
    // the split kernels' internal bit order (DeviceCode::perm / inv) and the
    // per-bit arrays in it
    qkd::DevBuf<int32_t> d_perm, d_inv, d_bit_chk_s;
    qkd::DevBuf<uint8_t> d_bit_deg_s;
    qkd::DevBuf<uint16_t> d_bit_pat_s, d_chk_rows16;
    qkd::DevBuf<uint32_t> d_ilv_slots, d_chk_odd;
    qkd::DevBuf<uint64_t> d_jump, d_jpoly, d_jpoly2;       // key generation (CodeHost)
    int cu_count = 0;
    qkd_workspace* default_ws = nullptr;

    // the classic kernels' view (original bit order)
    qkd::DeviceCode view() const {
        qkd::DeviceCode v{};
        v.n = n, v.m = m, v.e = e;
        v.n_pad = n_pad, v.m_pad = m_pad;
        v.max_dv = max_dv, v.max_dc = max_dc, v.min_dc = min_dc, v.min_dv = min_dv;
        v.n_tasks = n_tasks;
        v.chk_bits = d_chk_bits;
        v.chk_deg = d_chk_deg;
        v.plan = d_plan;
        v.bit_chk = d_bit_chk;
        v.bit_pos = d_bit_pos;
        v.bit_deg = d_bit_deg;
        v.n_pat = n_pat;
        v.bit_pat = d_bit_pat;
        v.pat_deg = d_pat_deg;
        v.chk_odd = d_chk_odd;
        return v;
    }
    // the split kernels' view (internal bit order, DeviceCode::perm)
    qkd::DeviceCode view_split() const {
        qkd::DeviceCode v = view();
        v.bit_chk = d_bit_chk_s;
        v.bit_pos = nullptr;
        v.bit_deg = d_bit_deg_s;
        v.bit_pat = d_bit_pat_s;
        v.bit_code = d_bit_code;
        v.plan_slot = d_plan_slot;
        v.perm = d_perm;
        v.inv = d_inv;
        v.chk_rows16 = d_chk_rows16;
        v.chk_rs = chk_rs;
        v.ilv_slots = d_ilv_slots;
        v.ilv_rs = ilv_rs;
        return v;
    }
};

// A rate-adaptation plan (adapt.hip): which bits of a frame are punctured,
// shortened or payload. Immutable after creation, shareable like a code.
//   d_src_orig[i]  original bit i: its payload index k >= 0 (payload bit k is
//                  the k-th position, ascending, that is neither punctured nor
//                  shortened), or kSrcPunctured / kSrcShortened (qkd_decode.h)
//   d_src_int[q]   the same for the split kernels' internal bit q (perm[q])
//   d_emb[i]       embedding: the payload index k >= 0, -1 for a shortened bit,
//                  -2 - r for the punctured bit that takes fill byte r (the
//                  r-th of the caller's punctured list)
//   d_rank_orig[i] that rank r for a punctured original bit i, -1 elsewhere
//   d_rank_int[q]  the same for the internal bit q (qkd_reconcile_blind_batch
//                  reveals the punctured bits in the order of their ranks)
struct qkd_adapt {
    const qkd_code* code = nullptr;
    int device = 0;
    int32_t n = 0, n_payload = 0, p = 0, s = 0;
    qkd::DevBuf<int32_t> d_src_orig, d_src_int, d_emb, d_rank_orig, d_rank_int;
};

namespace qkd {

void clear_error();

// A debug / A-B option (qkd_debug_set_option, host.cpp): the workspace's
// value, else the process-wide one, else unset (the product behaviour). The
// library reads no environment variable.
struct DbgOpt {
    bool set = false;
    std::string v;
    explicit operator bool() const { return set; }
    const char* c_str() const { return v.c_str(); }
    int as_int() const { return atoi(v.c_str()); }
    long as_long() const { return atol(v.c_str()); }
    bool is(const char* s) const { return set && v == s; }
};
DbgOpt debug_option(const qkd_workspace* ws, const char* name);
// no option is set, on the workspace or process-wide (the product path: one lock, no lookup)
bool debug_options_unset(const qkd_workspace* ws);

#define QKD_HIP(call)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess)                                                             \
            return ::qkd::set_error(QKD_ERR_DEVICE, "%s failed: %s (%s:%d)", #call,       \
                                    hipGetErrorString(e_), __FILE__, __LINE__);           \
    } while (0)

}  // namespace qkd
