// qkd_launch.h — the decision of a decode launch (launch.hip launch_decode:
// choose, prepare, launch): which kernels decode a batch, with which LDS
// layouts, buckets and strides, from the scalars of the code, of the call and
// of the debug options. No HIP header and no device call: choose_decode is a
// pure function, also compiled by the native tests
// (tests/native/launch_choice_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/qkd_ldpc.h"
#include "qkd_layout.h"
#include "qkd_limits.h"

namespace qkd {

// Largest check degree the first-iteration table covers.
constexpr int kFirstTableDeg = 16;

enum DecodeMode : int {
    kModeLlr = 0,  // qkd_decode_batch: caller LLRs + syndrome bytes
    kModeKeys = 1, // QKD_LDPC path: packed alice/bob keys, LLR = +-log_p
    // qkd_reconcile_adaptive_batch: one class byte per bit (DecodeArgs::cls, in
    // the launched kernel's bit order) and the caller's syndrome bytes; the LLR
    // of a bit is the level of its class: 0 +log_p, 1 -log_p, 2 +0.0
    // (punctured), 3 +known (shortened), 4 +known / 5 -known (a punctured bit
    // whose value Alice revealed: qkd_reconcile_blind_batch). Always with the
    // erasure rule.
    kModeClass = 2
};

// Check-node rule and message width (QKD_VARIANT_* in qkd_ldpc.h).
//   kRuleSp64   the reference's sum-product in binary64, bit-exact
//   kRuleSp32   the same schedule with binary32 messages and totals, the
//               check rule in Gallager's form with the hardware exp2 / log2
//               (a variant: not bit-exact to anything)
//   kRuleMinSum normalised min-sum in binary32: c2b = scale * sign * min|b2c|
//               over the other edges of the check (a variant, no transcendental)
//   kRuleMinSumLds  the same min-sum with the frame's whole message state in
//               LDS (per check: min1, min2, argmin, sign bits), no global
//               message store; used when the state fits (minsum_lds_fits)
//   kRuleMinSumLdsSc  kRuleMinSumLds with Savin's self-correction
//               (QKD_MINSUM_SELF_CORRECT) compiled in: its own kernel
//               instantiation, so profiles attribute its time to it
//   kRuleMinSumSplit / kRuleMinSumSplitSc  the same min-sum rules (plain /
//               self-corrected) on the split decoder's skeleton: one binary32
//               slot per edge, all in LDS, edge-parallel check phase
//               (decode_split.hip ms_split_check_phase); used whenever that
//               store fits (the default for codes like the reference's)
enum DecodeRule : int {
    kRuleSp64 = 0, kRuleSp32 = 1, kRuleMinSum = 2, kRuleMinSumLds = 3, kRuleMinSumLdsSc = 4,
    kRuleMinSumSplit = 5, kRuleMinSumSplitSc = 6
};

inline int rule_of(uint32_t flags) {
    switch (flags & QKD_VARIANT_MASK) {
        case QKD_VARIANT_SP_F32: return kRuleSp32;
        case QKD_VARIANT_MINSUM: return kRuleMinSum;
        default: return kRuleSp64;
    }
}

inline float minsum_scale_of(uint32_t flags) {
    const uint32_t q = (flags >> QKD_MINSUM_SCALE_SHIFT) & 0xffu;
    return q ? (float)q / 256.0f : (float)QKD_MINSUM_DEFAULT_SCALE;
}

constexpr int kFoldTabMaxEntries = 1024;   // speculative fold table (decode_split.hip), 8 B each
// speculative check phases (decode_split.hip), buckets 4 and 6: 1 one check per
// lane with an edge-lane remainder, 0 one edge per lane (QKD_CHECK_LANES overrides)
constexpr int kCheckLanesDefault = 1;
constexpr size_t kC2bPad = 64;            // split kernels: slots added to each workgroup's global region
// Bit phase: message rows per bit loaded ahead of the ordered sum, and rounds
// (bits tid + r*kDecodeBlock) per load batch.
constexpr int kDvUnroll = 3;
// fold table entries per degree pattern: 2^(1 + kDvUnroll) sign codes x
// (kDvUnroll psi bounds + the hard decision)
constexpr int kFoldTabPat = (2 << kDvUnroll) * (kDvUnroll + 1);
// the second-iteration table index and the first-message fold read a bit's
// messages from the unrolled rows only
static_assert(kTab2MaxDv <= kDvUnroll, "tables need every row of their bits unrolled");
// the LDS a workgroup can have
constexpr size_t kLdsBytesMax = 160 * 1024;
// the in-launch policy's frame windows (DecodeArgs::win): 256 frames, decided
// from the window 8 back (2048 frames earlier, ~8 frame-times at 256 resident
// workgroups: by then it has almost always completed; with the window 4 back
// the waits for a window's last slow frames cost 3.5 % per config-2 batch)
constexpr uint32_t kSpecWinShift = 8;
constexpr uint32_t kSpecWinLag = 8;

// The check-degree buckets (the in-check product reads DC values per lane): the
// smallest of 4 / 6 / 8 / 16 / top that holds max_dc, from `bottom` up. Kernel
// families narrow the ladder (their lookups have no other instantiations):
// top 32 the LDS-state min-sum (sign bits in one word), bottom 16 the large
// codes' kernels; the min-sum split kernels stop at 8 and the long-code kernel
// at 16, which their conditions on max_dc already guarantee.
QKD_LHD inline int dc_bucket(int max_dc, int top = 64, int bottom = 4) {
    const int ladder[4] = {4, 6, 8, 16};
    for (int b : ladder)
        if (b >= bottom && b < top && max_dc <= b) return b;
    return top;
}

// Syndrome bit arrays hold whole 64-check groups (written by one ballot each).
QKD_LHD inline int decode_m_words(int m) { return ((m + 63) / 64) * 2; }

// LDS layout of decode_kernel (bytes):
//   total  [n_pad]          bit totals (the reference's `total`, :256-267), message width
//   tsyn   [m_words]        target syndrome, one bit per check
//   xsyn   [m_words]        syndrome of the current hard decision (XOR-built)
//   qsyn   [m_words]        QKD path: sign of each check's first-iteration product
//   tval   [NW][64 + DC]    per-wave tanh values for the in-check products
//                           (prologue: the frame's Alice + Bob words)
//   ctab   [kFirstTableDeg+1] first-iteration message magnitudes by degree
//   tab2   [tab2_entries]   second-iteration tanh table
//   t2idx  [n_pad]          per-bit base index into tab2 (uint16)
//   ctl    [4]              frame index, block_any flags
//   cst    [m] (uint4)      kRuleMinSumLds: per-check min-sum state (ms_state)
struct DecodeLds {
    size_t tsyn, xsyn, qsyn, tval, ctab, tab2, t2idx, ctl, cst, czf, bytes;
    // total_esz: bytes per bit total in LDS (0: the totals live in global
    // memory, large codes); cst_checks: min-sum state of that many checks (16
    // bytes each, and with zf a word of zero flags each, self-corrected min-sum)
    QKD_LHD DecodeLds(int n_pad, int n_words, int m, int dc, int tab2_entries, int total_esz,
                      int cst_checks = 0, int row_esz = 0, bool zf = false) {
        const int m_words = decode_m_words(m);
        const int esz = row_esz ? row_esz : total_esz;
        tsyn = ((size_t)n_pad * total_esz + 15) & ~(size_t)15;
        xsyn = tsyn + (size_t)m_words * 4;
        qsyn = xsyn + (size_t)m_words * 4;
        tval = (qsyn + (size_t)m_words * 4 + 15) & ~(size_t)15;
        // the tanh rows double as the prologue's staging area for the frame's
        // Alice and Bob words
        const size_t rows = (size_t)(kDecodeBlock / 64) * (64 + dc) * esz;
        const size_t stage = (size_t)n_words * 16;
        ctab = (tval + (rows > stage ? rows : stage) + 15) & ~(size_t)15;
        tab2 = ctab + (size_t)(kFirstTableDeg + 1) * 8;
        t2idx = tab2 + (size_t)tab2_entries * 8;
        ctl = (t2idx + (tab2_entries ? (size_t)n_pad * 2 : 0) + 15) & ~(size_t)15;
        cst = ctl + 16;
        czf = cst + (size_t)cst_checks * 16;
        bytes = czf + (zf ? (size_t)cst_checks * 4 : 0);
    }
};

// ---- split message store (decode_split.hip) ----------------------------------
// LDS layout of decode_split_kernel (bytes):
//   tsyn, xsyn, qsyn [m_words]   target syndrome / XOR-built syndrome / first-product signs
//   xunc  [m_words]              speculative rounds: checks with an uncertain hard decision
//   zw    [n_pad / 64] uint64    hard decision of the last bit phase, one bit per bit
//   aw    [n_words] uint64       keys path: Alice's key words (the epilogue's compare)
//   tval  [NW][64 + DC] T        per-wave rows for the in-check products
//                                (prologue: the frame's Bob words)
//   ctab  [kFirstTableDeg + 1]   first-iteration message magnitudes by degree
//   tab2  [tab2_entries]         second-iteration tanh table
//   ftab  [ftab_entries]         speculative kernel: the folded first
//                                iteration's psi bounds and hard decisions
//   ctl   [12]                   [1] next frame, [4..5] round flags, [7] key mismatch (decode_split.hip)
//   wtab  [dc][dc][dc] float     extrinsic-sum weights by (degree, position, k) (dc <= 8)
//   msg   [S + 64] T             message slots 0 .. S-1 (slots S .. max_dv*n_pad-1
//                                live in the workgroup's global region), then
//                                one trash slot per lane
// S is as many slots as the budget leaves after the rest, in whole 64s.
// Weights of a check phase's extrinsic sums: lane at position p of a
// segment of degree deg sums row entry k with weight (k < deg && k != p).
// Buckets up to 8 read them from an LDS table (wtab[deg - 1][p][k], two
// per ds_read_b64) instead of extracting and converting mask bits per entry.
// Buckets DC <= 8 index their segment-weight rows by deg * 8 + p (encode_seg),
// so a lane's degree is one bit-field read of its plan word instead of a
// division by DC (rows of degree 0 and p >= DC unused; -3 VALU per check-phase
// task; with the check phases' select-free row entries -3.4 % per config-2
// batch, profiles/r06_ab.txt)
QKD_LHD inline int seg_weight_entries(int dc) { return dc <= 8 ? 9 * 8 * dc : 0; }

struct SplitLds {
    size_t tsyn = 0, xsyn = 0, qsyn = 0, xunc = 0, zw = 0, aw = 0, tval = 0, ctab = 0, tab2 = 0, ftab = 0, ctl = 0,
           wtab = 0, msg = 0, bytes = 0;
    uint32_t S = 0;
    SplitLds() = default;
    QKD_LHD SplitLds(int n_pad, int n_words, int m, int max_dv, int dc, int tab2_entries,
                     int ftab_entries, int esz, size_t budget) {
        const int m_words = decode_m_words(m);
        tsyn = 0;
        qsyn = tsyn + (size_t)m_words * 4;
        xsyn = qsyn + (size_t)m_words * 4;
        xunc = xsyn + (size_t)m_words * 4;
        zw = (xunc + (size_t)m_words * 4 + 15) & ~(size_t)15;
        // keys path: Alice's words of the frame, loaded with the prologue's
        // batch for the epilogue's key compare
        aw = (zw + (size_t)(n_pad / 64) * 8 + 15) & ~(size_t)15;
        tval = (aw + (size_t)n_words * 8 + 15) & ~(size_t)15;
        const size_t rows = (size_t)(kDecodeBlock / 64) * (64 + dc) * esz;
        const size_t stage = (size_t)n_words * 8;     // (the prologue stages Bob's words there)
        ctab = (tval + (rows > stage ? rows : stage) + 15) & ~(size_t)15;
        tab2 = ctab + (size_t)(kFirstTableDeg + 1) * 8;
        ftab = (tab2 + (size_t)tab2_entries * 8 + 15) & ~(size_t)15;
        ctl = (ftab + (size_t)ftab_entries * 8 + 15) & ~(size_t)15;
        wtab = ctl + 48;
        msg = (wtab + (size_t)seg_weight_entries(dc) * 4 + 15) & ~(size_t)15;
        const size_t slots = (size_t)max_dv * n_pad;
        // 64 trash slots follow the S message slots (decode_split.hip SplitStore)
        const size_t fit = budget > msg + 64 * (size_t)esz ? (budget - msg) / (size_t)esz - 64 : 0;
        // (a multiple of 64: with n_pad one too, a wave's 64 consecutive bits
        // of one row are all in LDS or all global, SplitStore::ld_row)
        S = (uint32_t)(slots < fit ? slots : fit) & ~63u;
        bytes = msg + ((size_t)S + 64) * esz;
    }
};

// Encoded message-slot words of the split decoder's check phases (its plan,
// DecodeArgs::plan_enc, one per LDS layout): slot x < S (in LDS) as
// kSlotLds | its byte address from the dynamic LDS base; a global slot as
// kSlotGlobalBase + its byte offset in the workgroup's region. The buffer
// descriptor of the region starts kSlotGlobalBase bytes early and spans
// kSlotGlobalBase + the region, so LDS words fail its range check (loads give
// 0, stores are dropped), and global words are LDS addresses past any
// allocation (the same there: tools/mb/lds_oob.hip measures it on gfx950).
constexpr uint32_t kSlotLds = 0x80000000u;
constexpr uint32_t kSlotGlobalBase = 0x40000u;
static_assert(kLdsBytesMax <= kSlotGlobalBase, "global slot words must lie past the LDS");
// The reserved word of a slot that does not exist (the check-lane plan's
// entries past a check's degree): out of range for BOTH halves of an access,
// so it loads 0 and its store goes nowhere. As an LDS address it is past any
// allocation in the way every global word is, whatever number of low address
// bits the hardware compares (all of them are set); as a buffer offset it is
// past the descriptor's range as long as the range ends at or below it.
// slot_dead_ok says so for an LDS allocation and a region of global slots (8
// bytes each): plan_for_layout (launch.hip) checks every layout it encodes
// against the largest region a launch can give it, choose_decode the region
// it gives. 8-byte aligned, as every slot word.
constexpr uint32_t kSlotDead = 0x7ffffff8u;
static_assert((kSlotDead & (kSlotLds | 7u)) == 0, "a global-form word, aligned");
// an encoded global slot word (kSlotGlobalBase + byte offset) must stay below
// kSlotLds, the LDS words' tag bit, and the region's buffer range below the
// dead slot word
static_assert(kSlotDead < kSlotLds, "the dead word bounds the global words");
QKD_LHD inline bool slot_dead_ok(size_t lds_bytes, size_t global_slots) {
    return lds_bytes <= kSlotGlobalBase && (size_t)kSlotGlobalBase + global_slots * 8 <= kSlotDead;
}

// The frame-interleaved decoder (decode_ilv.hip): kIlvCols frames per
// workgroup in lockstep, one per lane of each 16-lane group; one message
// line = one slot of the kIlvCols frames (128 bytes).
constexpr int kIlvCols = 16;
constexpr int kIlvCtlWords = 64;
// its workgroup size (QKD_ILV_BLOCK; one workgroup per CU either way: its LDS)
#ifndef QKD_ILV_BLOCK
#define QKD_ILV_BLOCK 1024
#endif
constexpr int kIlvBlock = QKD_ILV_BLOCK;
// the check phase's index ring: per 16-lane group four stages of kRingStage
// words (a check's line indices, ~0 past its degree)
constexpr int kRingStage = 16;
// LDS: tsyn / xsyn / xunc, one word per check pair (check 2w in bits 0-15,
// 2w + 1 in bits 16-31, bit = column), the column control words, the
// first-iteration magnitudes by check degree.
struct IlvLds {
    size_t tsyn = 0, xsyn = 0, xunc = 0, ctl = 0, ctab = 0, ring = 0, bytes = 0;
    IlvLds() = default;
    // tsyn_global: the target syndrome words in the workgroup's global region
    // instead (decode_ilv_kernel's TG), for codes whose three arrays do not
    // fit; xunc_global (UG, with TG): the uncertainty words there too (M past
    // ~37,000: only the XOR-built syndrome stays in LDS)
    QKD_LHD IlvLds(int m, bool tsyn_global, bool xunc_global = false) {
        const size_t mw2 = (size_t)(m + 1) / 2;
        const size_t k = tsyn_global ? 0 : 1;
        const size_t u = xunc_global ? 0 : 1;
        tsyn = 0;
        xsyn = k * mw2 * 4;
        xunc = (k + 1) * mw2 * 4;
        ctl = ((k + 1 + u) * mw2 * 4 + 15) & ~(size_t)15;
        ctab = ctl + (size_t)kIlvCtlWords * 4;
        ring = ctab + (size_t)(kFirstTableDeg + 1) * 8;
        bytes = ring + (size_t)(kIlvBlock / kIlvCols) * 4 * kRingStage * 4;
    }
};

// ---- the decision's inputs ---------------------------------------------------

// A debug option as the launch reads it: set or not (set but empty reads as 0)
struct OptInt {
    bool set = false;
    long v = 0;
};
// Every debug option of the launch path (qkd_debug_set_option), parsed once
// per call (launch.hip launch_options): the workspace's value, else the
// process-wide one.
struct LaunchOptions {
    bool ms_global = false, ms_lds = false;   // QKD_MINSUM_STORE=global / =lds
    bool classic = false;                     // QKD_DECODE_KERNEL=classic
    size_t split_budget = kLdsBytesMax;       // QKD_SPLIT_BUDGET lowers the split layout's LDS budget
    OptInt fold_table;                        // QKD_FOLD_TABLE (0: the per-bit fold)
    bool spec_always = false;                 // QKD_SPEC_POLICY=always
    OptInt decode_grid;                       // QKD_DECODE_GRID caps the decoder's workgroups
    OptInt check_lanes;                       // QKD_CHECK_LANES 0 / 1 / 2
    OptInt c2b_pad;                           // QKD_C2B_PAD: a fixed pad, in slots
    bool phase_timing = false;                // QKD_PHASE_TIMING set
    OptInt ilv;                               // QKD_ILV forces the interleaved decoder on / off
    OptInt ilv_grid;                          // QKD_ILV_GRID caps its workgroups
    bool syn_gather = false;                  // QKD_SYN_SLICED=0
    bool syn_pack_first = false;              // QKD_SYN_BYTES=0
};

// The scalars of a code the decision reads.
struct CodeFacts {
    int32_t n = 0, m = 0, n_pad = 0, max_dv = 0, max_dc = 0, n_pat = 0, n_tasks = 0;
    int32_t cl_dc = 0, cl_tasks[2] = {0, 0}, cl_rem_tasks[2] = {0, 0};
    int32_t ilv_rs = 0;
    bool has_bit_code = false, has_ilv_slots = false;
    int cu_count = 0;
    size_t slots() const { return (size_t)max_dv * n_pad; }
    int n_words() const { return (n + 63) / 64; }
};
// (a code object keeps CodeHost and the device copies: whether the packed bit
// words and the interleaved lines exist is whether it uploaded them)
inline CodeFacts code_facts(const CodeHost& h, bool has_bit_code, bool has_ilv_slots, int cu_count) {
    CodeFacts c;
    c.n = h.n, c.m = h.m, c.n_pad = h.n_pad, c.max_dv = h.max_dv, c.max_dc = h.max_dc;
    c.n_pat = h.n_pat, c.n_tasks = h.n_tasks, c.cl_dc = h.cl_dc, c.ilv_rs = h.ilv_rs;
    for (int k = 0; k < 2; ++k) c.cl_tasks[k] = h.cl_host[k].cl_tasks, c.cl_rem_tasks[k] = h.cl_host[k].rem_tasks;
    c.has_bit_code = has_bit_code, c.has_ilv_slots = has_ilv_slots, c.cu_count = cu_count;
    return c;
}
inline CodeFacts code_facts(const CodeLayout& L, int cu_count) {
    return code_facts(L, !L.bit_code.empty(), !L.ilv_slots.empty(), cu_count);
}

// What the decision reads of the call.
struct LaunchFacts {
    int mode = kModeLlr;
    uint32_t flags = 0;
    uint32_t n_frames = 0;
    bool clamp_on = false;
    uint32_t spec_cap = 0, ckpt_unsat = 0;
    int first_table = 0, tab2_entries = 0;
    bool trace = false;          // qkd_trace_decode
    bool bits_out = false;       // the caller wants the decisions as bytes
    bool class_verify = false;   // kModeClass with a verification key
    bool adapt = false;          // kModeClass: the plan is given
};

// ---- the decision ------------------------------------------------------------

// One kernel instantiation by its template arguments (the lookups:
// decode.hip classic_kernel, decode_split.hip split_kernel, decode_ilv.hip
// ilv_kernel; a key without an instantiation gives nullptr there).
enum KernelKind : int { kKernelNone = 0, kKernelClassic, kKernelSplit, kKernelIlv };
struct KernelKey {
    int kind = kKernelNone;
    int mode = 0, rule = 0, dc = 0;
    bool clamp = false;
    bool gt = false;             // classic: the bit totals in global memory
    int spec = 0;                // split: 1 speculative, 2 checkpointed
    bool lng = false;            // split: the long-code kernel (LONG)
    bool era = false, vfy = false;
    int rs = 0;                  // interleaved: the check rows' stride
    bool tg = false, ug = false; // interleaved: target / uncertainty words in global memory
    bool operator==(const KernelKey& o) const {
        return kind == o.kind && mode == o.mode && rule == o.rule && dc == o.dc && clamp == o.clamp && gt == o.gt &&
               spec == o.spec && lng == o.lng && era == o.era && vfy == o.vfy && rs == o.rs && tg == o.tg && ug == o.ug;
    }
};

enum DecodePath : int { kPathClassic = 0, kPathSplit = 1, kPathSplitIlv = 2 };

struct DecodeChoice {
    // a refusal: the status and its message (nothing else is then meaningful)
    qkd_status status = QKD_OK;
    const char* message = "";
    int path = kPathClassic;
    int rule = kRuleSp64;        // after the min-sum promotions
    int bucket = 0;              // the check-degree bucket of every kernel of the launch
    // decoder: the kernel that takes the frames (split path with the
    // interleaved decoder: unused). handoff (split path): the exact split
    // kernel, which decodes the interleaved decoder's hand-offs; the resident
    // workgroups are the fewer of its and the decoder's. ilv: the interleaved
    // decoder.
    KernelKey decoder, ilv, handoff;
    size_t lds_bytes = 0;        // classic path: the decoder's LDS
    SplitLds split;              // split paths
    IlvLds ilv_lds;
    uint32_t lds_budget = 0;     // the budget `split` was sized for
    int esz = 8;                 // bytes per message slot
    int ftab_entries = 0;
    bool spec = false, ckpt = false, spec_always = false;
    // the check phases' form (QKD_CHECK_LANES as applied), DecodeArgs::cl_split
    // and the workspace's record of them (qkd_debug_check_lanes); cl_report:
    // this launch updates that record
    int cl_form = 0, cl_tasks = 0, cl_rem_tasks = 0;
    uint32_t cl_split = 0;
    bool cl_report = false;
    size_t c2b_stride = 0, istride = 0;
    bool tsg = false, ug = false, gt = false;
    bool ilv_forced = false;     // QKD_ILV set: no retreat when its lines cannot be allocated
    // a binary64 split layout whose global slot words stay below the dead word
    bool dead_ok = true;
    // what the launch reserves: c2b regions (one per workgroup, or none: the
    // LDS-state min-sum), the encoded plan, checkpoints, policy windows,
    // interleaved lines with the hand-off list
    bool need_c2b = true, need_plan = false, need_ckpt = false, need_ilv = false;
    uint32_t win_count = 0;
    // the call's values as the launch applies them (the erasure rule clears
    // the speculation, large codes the per-bit tables)
    uint32_t spec_cap = 0;
    int first_table = 0, tab2_entries = 0;
};

inline size_t classic_lds_bytes(const CodeFacts& c, int dc, int tab2_entries, int rule, bool gt = false,
                                bool sc = false) {
    const int esz = rule == kRuleSp64 ? 8 : 4;
    const bool msl = rule == kRuleMinSumLds || rule == kRuleMinSumLdsSc;
    return DecodeLds(c.n_pad, c.n_words(), c.m, dc, tab2_entries, gt ? 0 : esz, msl ? c.m : 0, esz, msl && sc).bytes;
}

// The LDS-resident min-sum needs the check state (sign bits in one word:
// degree <= 32) and all of its LDS in one workgroup.
inline bool minsum_lds_fits(const CodeFacts& c, bool sc) {
    if (c.max_dc > 32 || c.n > kMaxBitsLds) return false;
    return classic_lds_bytes(c, dc_bucket(c.max_dc, 32), 0, kRuleMinSumLds, false, sc) <= kLdsBytesMax;
}

inline DecodeChoice refuse_decode(qkd_status s, const char* message) {
    DecodeChoice ch;
    ch.status = s;
    ch.message = message;
    return ch;
}

// The kernels, layouts and reservations of one decode launch. allow_ilv =
// false: without the frame-interleaved decoder (its message lines could not be
// allocated), i.e. the split kernel, or the classic kernel for a long code.
inline DecodeChoice choose_decode(const CodeFacts& c, const LaunchFacts& f, const LaunchOptions& o, bool allow_ilv) {
    DecodeChoice ch;
    const int mode = f.mode;
    int rule = rule_of(f.flags);
    ch.spec_cap = f.spec_cap;
    ch.first_table = f.first_table;
    ch.tab2_entries = f.tab2_entries;
    // QKD_FLAG_ERASURES: the binary64 rule's erasure-aware instantiations,
    // exact iterations only (the interval forms are not defined at t = 0), so
    // the outputs cannot depend on QKD_SPEC_CAP. A dispatch without such an
    // instantiation fails; none applies the reference rule instead.
    const bool era = (f.flags & QKD_FLAG_ERASURES) != 0 || mode == kModeClass;
    if (era) {
        if (rule != kRuleSp64 || mode == kModeKeys || f.trace || (mode == kModeClass && !f.adapt))
            return refuse_decode(QKD_ERR_UNSUPPORTED, "the erasure rule: binary64 variant, LLR or class entry, no trace");
        ch.spec_cap = 0;
    }
    const bool sc = (f.flags & QKD_MINSUM_SELF_CORRECT) != 0;
    const size_t slots = c.slots();
    const int n_words = c.n_words();
    // min-sum: the split skeleton (every binary32 slot in LDS, the binary32
    // rule's bit phase over DeviceCode::bit_code) when it applies, else the
    // LDS-state kernel, else the global message store
    // (QKD_MINSUM_STORE=global / =lds keep the latter two: tests)
    if (rule == kRuleMinSum && !o.ms_global && !o.ms_lds && !o.classic && !f.trace && c.has_bit_code &&
        c.n <= kMaxBitsSplit && c.m <= kMaxChecksSplit && c.max_dc <= 8) {
        // (check degree <= 8: the additive mask table, seg_weight_entries)
        const SplitLds Lm(c.n_pad, n_words, c.m, c.max_dv, dc_bucket(c.max_dc), 0, sc ? 2 * c.n_tasks + n_words : 0,
                          4, kLdsBytesMax);
        if (Lm.S >= (uint32_t)slots && Lm.bytes <= kLdsBytesMax) rule = sc ? kRuleMinSumSplitSc : kRuleMinSumSplit;
    }
    if (rule == kRuleMinSum && !o.ms_global && minsum_lds_fits(c, sc)) rule = kRuleMinSumLds;
    if (sc && rule != kRuleMinSumLds && rule != kRuleMinSumSplitSc)
        return refuse_decode(QKD_ERR_UNSUPPORTED, "self-corrected min-sum needs the split or the LDS-state min-sum "
                                                  "kernel (check degree <= 32, its state in LDS)");
    if (sc && rule == kRuleMinSumLds) rule = kRuleMinSumLdsSc;
    ch.rule = rule;
    const bool class_vfy = mode == kModeClass && f.class_verify;
    // The split-store kernel (decode_split.hip) for the sum-product rules
    // whenever its LDS layout fits; QKD_DECODE_KERNEL=classic keeps
    // decode_kernel (A/B measurements, tests). Trace mode records the classic
    // kernel's store.
    const bool msr = rule == kRuleMinSumSplit || rule == kRuleMinSumSplitSc;
    // codes past kMaxBitsSplit (up to kMaxBitsSplitLong): only the
    // frame-interleaved decoder and its exact hand-off kernel (LONG) take
    // them, on the keys path with the split view's arrays; otherwise the
    // classic kernel below
    const bool long_code = c.n > kMaxBitsSplit;
    const bool long_ok = rule == kRuleSp64 && mode == kModeKeys && c.n <= kMaxBitsSplitLong && c.has_ilv_slots &&
                         c.max_dc <= 16;
    if ((rule == kRuleSp64 || rule == kRuleSp32 || msr) && !o.classic && !f.trace && (!long_code || long_ok) &&
        c.m <= kMaxChecksSplit) {
        DecodeChoice s = ch;
        s.bucket = dc_bucket(c.max_dc);
        s.esz = rule == kRuleSp64 ? 8 : 4;
        // the speculative kernel (interval iterations, qkd_spec.h, exact
        // replays in place) when it applies: QKD path with the folded first
        // iteration, binary64 rule, clamped messages, bit degree <= kDvUnroll
        // (the QKD path needs its folded first iteration; the LLR path starts from the LLRs)
        s.spec = rule == kRuleSp64 && s.spec_cap > 0 && f.clamp_on && (mode == kModeLlr || f.first_table) &&
                 c.max_dv <= kDvUnroll && c.has_bit_code;
        s.ckpt = s.spec && mode == kModeKeys && f.ckpt_unsat > 0;
        // its folded first iteration from a table (decode_split.hip fold_table_fill)
        // (at most kFoldTabMaxEntries: the table's LDS comes off the message slots)
        s.ftab_entries = (s.spec && !s.ckpt && mode == kModeKeys && f.tab2_entries &&
                          c.n_pat * kFoldTabPat <= kFoldTabMaxEntries)
                             ? c.n_pat * kFoldTabPat : 0;
        // (QKD_FOLD_TABLE=0: the per-bit form; tests compare the two)
        if (o.fold_table.set && (int)o.fold_table.v == 0) s.ftab_entries = 0;
        s.spec_always = o.spec_always;
        // (self-corrected min-sum: its previous-b2c ballot words and the
        // frame's Bob words in the ftab region)
        if (rule == kRuleMinSumSplitSc) s.ftab_entries = 2 * c.n_tasks + n_words;
        // (the long-code hand-off kernel: the frame's Bob words there)
        if (long_code && s.ftab_entries < n_words) s.ftab_entries = n_words;
        // diagnostic: QKD_SPLIT_BUDGET lowers the LDS budget (fewer LDS slots)
        const size_t budget = o.split_budget < kLdsBytesMax ? o.split_budget : kLdsBytesMax;
        const SplitLds L(c.n_pad, n_words, c.m, c.max_dv, s.bucket, f.tab2_entries, s.ftab_entries, s.esz, budget);
        // (the binary32 rules' kernels keep every slot in LDS: SplitStore<float, true>)
        // (binary64: any share of the slots in LDS, the rest in the
        // workgroup's global region; long codes keep most of them there)
        const bool fits = rule != kRuleSp64 ? L.S >= (uint32_t)slots : L.S >= 64;
        if (L.bytes <= kLdsBytesMax && fits) {
            s.split = L;
            s.lds_budget = (uint32_t)budget;
            s.need_plan = rule == kRuleSp64 || msr;
            s.cl_report = true;
            s.cl_rem_tasks = c.n_tasks;
            // the speculative check phases one check per lane (the default
            // where the kernel has them: buckets 4 and 6, not the checkpointed
            // form). QKD_CHECK_LANES: 0 edge-lane, 1 check-lane with the
            // edge-lane remainder, 2 every check on a lane
            if (s.spec && !s.ckpt && !long_code && rule == kRuleSp64 && c.cl_dc == s.bucket) {
                s.cl_form = kCheckLanesDefault;
                if (o.check_lanes.set) s.cl_form = (int)o.check_lanes.v < 0 ? 0 : (int)o.check_lanes.v > 2 ? 2 : (int)o.check_lanes.v;
            }
            if (s.cl_form != 0) {
                s.cl_tasks = c.cl_tasks[s.cl_form - 1];
                s.cl_rem_tasks = c.cl_rem_tasks[s.cl_form - 1];
                s.cl_split = 0x80000000u | (uint32_t)s.cl_tasks | ((uint32_t)s.cl_rem_tasks << 16);
            }
            // elements of the message type, plus kC2bPad: the workgroups' regions
            // start off a common alignment (measured: config 2 with the fold table
            // has a region of 13184 slots, 4 % slower than 13248;
            // QKD_C2B_PAD overrides the pad)
            // Default: the region rounded up to an ODD multiple of kC2bPad
            // slots (512 bytes), so consecutive regions never share an
            // alignment above 512 bytes (13248 = 207 x 64 is the measured
            // good case above); QKD_C2B_PAD adds a fixed pad instead.
            if (o.c2b_pad.set) {
                const size_t pad = (size_t)o.c2b_pad.v < (size_t)c.n_pad ? (size_t)o.c2b_pad.v : (size_t)c.n_pad;
                s.c2b_stride = ((slots - L.S + 31) & ~(size_t)31) + pad;
            } else {
                size_t st = (slots - L.S + kC2bPad - 1) / kC2bPad;
                if ((st & 1u) == 0) st++;
                s.c2b_stride = st * kC2bPad;
            }
            s.dead_ok = rule != kRuleSp64 || slot_dead_ok(L.bytes, s.c2b_stride);
            // the exact kernel of the layout, and the speculative one in its
            // place (a long code: the interleaved decoder speculates; no
            // split speculation)
            KernelKey k;
            k.kind = kKernelSplit, k.mode = mode, k.rule = rule, k.dc = s.bucket, k.clamp = f.clamp_on;
            k.lng = long_code, k.era = era, k.vfy = class_vfy;
            s.handoff = s.decoder = k;
            if (s.spec && !long_code) {
                s.decoder.spec = s.ckpt ? 2 : 1;
                // one saved message store per resident workgroup
                s.need_ckpt = s.ckpt;
            }
            // the in-launch policy's windows
            if (s.spec) s.win_count = (uint32_t)((f.n_frames + (1u << kSpecWinShift) - 1) >> kSpecWinShift);
            // Long codes (the split store keeps under a quarter of the slots
            // in LDS): the frame-interleaved decoder (decode_ilv.hip), its
            // hand-offs decoded by this split kernel from a frame list.
            // QKD_ILV=1 / 0 forces it on / off (tests, A/B).
            // (the target syndrome words in LDS when the three arrays fit, else
            // in global memory: measured 30 % slower at N = 40,000, where
            // they fit, and twice as fast as the split kernel at 60,000)
            // (then also the uncertainty words, for M past ~37,000)
            s.tsg = IlvLds(c.m, false).bytes > kLdsBytesMax;
            s.ug = s.tsg && IlvLds(c.m, true).bytes > kLdsBytesMax;
            s.ilv_lds = IlvLds(c.m, s.tsg, s.ug);
            bool ilv = allow_ilv && mode == kModeKeys && s.spec && !s.ckpt && !f.bits_out && f.first_table &&
                       c.has_ilv_slots && s.ilv_lds.bytes <= kLdsBytesMax;
            if (ilv) {
                s.ilv_forced = o.ilv.set;
                ilv = o.ilv.set ? (int)o.ilv.v != 0
                                : (size_t)L.S * 4 < slots && (size_t)f.n_frames * 2 >= (size_t)kIlvCols * c.cu_count;
            }
            // (per workgroup: the message lines, the columns' key words, their
            // target syndrome words: (M + 1) / 2 words, in doubles)
            // rounded to 512 bytes: every workgroup's lines start on a cache
            // line (an unaligned stride splits each line access in two)
            // (and, ug, their uncertainty words as many again)
            s.istride = (slots * kIlvCols + (size_t)n_words * kIlvCols * 2 +
                         (s.ug ? 2 : 1) * (((size_t)(c.m + 1) / 2 + 1) / 2) + 63) & ~(size_t)63;
            if (ilv) {
                s.path = kPathSplitIlv;
                s.need_ilv = true;
                s.ilv.kind = kKernelIlv, s.ilv.rs = c.ilv_rs, s.ilv.dc = s.bucket, s.ilv.tg = s.tsg, s.ilv.ug = s.ug;
                return s;
            }
            if (!long_code) {
                s.path = kPathSplit;
                return s;
            }
            // (a long code the interleaved decoder does not take: the classic
            // kernel, with the call's values as given)
            ch.cl_report = true;
            ch.cl_rem_tasks = c.n_tasks;
        }
    }
    // Totals in LDS unless the code is too long for them (the large-code
    // kernels, which keep no per-bit LDS tables).
    const bool msl = rule == kRuleMinSumLds || rule == kRuleMinSumLdsSc;
    ch.bucket = dc_bucket(c.max_dc, msl ? 32 : 64);
    ch.gt = c.n > kMaxBitsLds || classic_lds_bytes(c, ch.bucket, f.tab2_entries, rule) > kLdsBytesMax;
    if (ch.gt) {
        ch.first_table = 0;
        ch.tab2_entries = 0;
        ch.bucket = dc_bucket(c.max_dc, msl ? 32 : 64, 16);
    }
    ch.path = kPathClassic;
    ch.esz = rule == kRuleSp64 ? 8 : 4;
    KernelKey& k = ch.decoder;
    k.kind = kKernelClassic, k.mode = mode, k.rule = rule, k.dc = ch.bucket, k.clamp = f.clamp_on, k.gt = ch.gt;
    k.era = era, k.vfy = class_vfy;
    ch.lds_bytes = classic_lds_bytes(c, ch.bucket, ch.tab2_entries, rule, ch.gt, sc);
    ch.need_c2b = !msl;                       // (the LDS-state min-sum: no global messages)
    ch.c2b_stride = slots;
    return ch;
}

}  // namespace qkd
