// decode.hip — the classic decoder kernel (decode_kernel) and the lookup of its
// instantiations (classic_kernel); launched by launch.hip.
//
// Hot path: flooding sum-product decoding, reference
// src/qkd_ldpc_algorithm.cpp:175-345 (irregular) / :3-173 (regular, the same
// arithmetic for a regular code), reached through QKD_LDPC_* (:347-447) and
// run_trial (src/simulation.cpp:161-189).
//
// MI355X mapping
//   * One 1024-thread workgroup owns one frame at a time; workgroups are
//     persistent (grid = resident workgroups) and pull frames from a device
//     queue (one atomic per frame), so frames with 2 and 50 iterations mix
//     without tail stalls.
//   * Per-frame state is the reference's two message arrays collapsed to one:
//     c2b messages (E binary64, slot-major per check, in HBM/L2/MALL) plus the
//     bit totals (N binary64) in LDS. The reference's b2c message for edge
//     (j,i) is exactly total_i - c2b(j,i) clamped (its :303-316), so it is
//     recomputed inside the check update instead of being stored: same bits,
//     half the message traffic.
//   * Check phase: thread per check, slot-major coalesced c2b read/write, the
//     d_c tanh values in registers, the extrinsic product by division (keeps
//     the reference's 0/0 -> NaN behaviour). Bit phase: thread per bit,
//     gathers its d_v c2b in ascending check order (the reference's
//     std::accumulate order). Syndrome test: thread per check over LDS totals,
//     block-wide OR.
//   * tanh/atanh are the bit-exact restatements in qkd_math.h; the whole
//     library builds with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "qkd_decode.h"
#include "qkd_host.h"

namespace qkd {

// The check phase of one iteration for one wave: tasks wave, wave + NW, ...
// Per edge (qkd_ldpc_algorithm.cpp:220-249):
//   b2c = FIRST ? LLR_i : clamp(total_i - c2b)                  (:188, :303-316)
//   t   = tanh(b2c / 2)                                         (:224)
//   P   = (s_j ? -1 : 1) * t_0 * t_1 * ...  (ascending bits)    (:231-235)
//   c2b = clamp(2 * atanh(P / t))                               (:239-249)
// Software-pipelined and unrolled by two so that no loaded value is copied
// across the loop back-edge. Each half-trip does, in this order:
//   store the previous task's message  |  issue the look-ahead loads (plan
//   word two tasks ahead, bit total and stored message one task ahead)  |
//   compute this task (its operands were loaded one half-trip earlier).
// vmcnt counts loads and stores in issue order, so a task only ever waits
// for memory operations that had a whole task of arithmetic to complete.
// The plan is padded with idle tasks (qkd_plan.h): no bounds tests on the
// look-ahead loads.
//
// Measured (config 2, three iterations): removing the tanh /
// atanh arithmetic saves only 12 % of the kernel, making the message
// gathers/scatters coalesced saves 24 %: the phase is bound by the two
// together, not by fp64 latency (working on two tasks at once, to interleave
// two dependency chains, measured no gain).
template <int SRC, bool CLAMP, int DC, int RULE, bool ERA = false, typename T>
__device__ __forceinline__ void check_phase(const uint2* __restrict__ plan, const uint32_t* tsyn,
                                            const T* total, const uint16_t* t2idx, const double* tab2,
                                            T* __restrict__ c2b, T* row, int n_tasks, int n_pad, T thr,
                                            int wave, int lane, float ms_scale, float ms_offset) {
    constexpr int NW = kDecodeBlock / 64;
    constexpr bool FIRST = SRC != kSrcGeneral;    // no stored message is read
    int t = wave;
    if (t >= n_tasks) return;
    const uint2* pl = plan + lane;
    auto msg = [&](uint2 p) -> T* { return c2b + pw_row(p) * n_pad + pw_bit(p); };
    // the incoming value: a bit total, or (kSrcTable) the tabulated tanh
    auto src = [&](uint2 p) -> T {
        if constexpr (SRC == kSrcTable) return tab2[t2idx[pw_bit(p)] + pw_row(p)];
        else return total[pw_bit(p)];
    };
    // the target syndrome bit of the lane's check
    auto sbit = [&](uint2 p) -> uint32_t {
        const uint32_t j = pw_chk(p);
        return (tsyn[j >> 5] >> (j & 31)) & 1u;
    };
    auto edge = [&](T x, T o, uint2 w) -> T {
        const T a = edge_in<SRC, CLAMP, RULE>(x, o, thr);
        row[lane] = a;
        wave_lds_sync();
        return edge_out<CLAMP, DC, RULE, ERA>(a, w, sbit(w), lane, thr, row, ms_scale, ms_offset);
    };
    uint2 wa = pl[t * 64];
    uint2 wb = pl[(t + NW) * 64];
    T xa = src(wa);
    T oa = FIRST ? (T)0 : *msg(wa);
    T* pend = nullptr;      // message computed by the previous task, not yet stored
    T pv = 0;
    for (;;) {
        if (pend) msg_store(pend, pv);
        const uint2 wc = pl[(t + 2 * NW) * 64];
        const T xb = src(wb);
        const T ob = FIRST ? (T)0 : *msg(wb);
        pv = edge(xa, oa, wa);
        pend = msg(wa);
        t += NW;
        if (t >= n_tasks) break;
        msg_store(pend, pv);
        wa = pl[(t + 2 * NW) * 64];
        xa = src(wc);
        oa = FIRST ? (T)0 : *msg(wc);
        pv = edge(xb, ob, wb);
        pend = msg(wb);
        t += NW;
        if (t >= n_tasks) break;
        wb = wa;
        wa = wc;
    }
    *pend = pv;
}

// ---- min-sum with the message state in LDS (kRuleMinSumLds) -----------------
// Every min-sum message of a check j is a function of four words (ms_state):
//   x  min1 = min_k |b2c_k|                (binary32 bits)
//   y  min2 = min over k != idx1 of |b2c_k|
//   z  sign bits, bit k = (b2c_k < 0)
//   w  idx1 (bits 0..7; 0xff: none) | par << 31,   par = s_j ^ parity(z)
// and, self-corrected (QKD_MINSUM_SELF_CORRECT), a fifth word czf[j]: bit k =
// (b2c_k == 0). z and czf are then also the previous iteration's b2c signs
// and erasures, which the next check phase compares with (Savin's
// self-corrected min-sum: a b2c whose sign flipped, both nonzero, becomes 0).
// The message to the edge at position k is scale * (k == idx1 ? min2 : min1),
// negated when par ^ z_k, then clamped: the same binary32 operations, on the
// same values, as edge_out's min-sum branch (and tests/test_variants.py's model), so the
// two kernels agree bit for bit. (min over the others of the |b2c| is min2 for
// the argmin and min1 for everyone else, ties included; NaN magnitudes never
// win a comparison, as fminf ignores them.) 16 bytes per check instead of 4
// bytes per edge: the frame's whole message state (m * 16 B) and its bit
// totals (n * 4 B) stay in LDS, and the decode touches no global memory but
// the code's own (L2-resident) arrays.
template <bool CLAMP>
__device__ __forceinline__ float ms_msg(uint4 st, uint32_t pos, float scale, float off, float thr) {
    const float m = pos == (st.w & 0xffu) ? __uint_as_float(st.y) : __uint_as_float(st.x);
    float v = scale * m;
    if (off > 0.0f) v = fmaxf(v - off, 0.0f);
    const uint32_t neg = (st.w >> 31) ^ ((st.z >> pos) & 1u);
    v = neg ? -v : v;
    if (CLAMP) v = clamp_msg(v, thr);
    return v;
}

// Check phase of kRuleMinSumLds for one wave: per lane (edge), b2c from the
// bit total and the check's previous state; the segment's first lane then
// folds the segment's b2c (through the wave's LDS row) into the new state.
// Check phase of kRuleMinSumLds: one THREAD per check (rounds of 1024
// checks). The min-sum check rule costs a handful of operations per edge, so
// unlike the sum-product phase (one edge per lane, to spread the per-edge
// transcendentals) a thread walks its check's row itself: bit totals from
// LDS, the previous state from LDS, the row's bits from the code's ELL array
// (coalesced across threads, L2-resident), the next round's row loaded ahead.
//   b2c_k = FIRST ? total : clamp(total - message_k(previous state))
//   state = (min |b2c|, second min, argmin, signs, s_j ^ parity)
template <int SRC, bool CLAMP, int DC>
__device__ __forceinline__ void ms_check_phase(const DeviceCode& c, const uint32_t* tsyn, const float* total,
                                               uint4* cst, uint32_t* czf, bool sc, float thr, float scale,
                                               float off) {
    const int m = c.m;
    int j = threadIdx.x;
    if (j >= m) return;
    int nb[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) nb[k] = k < c.max_dc ? c.chk_bits[k * c.m_pad + j] : -1;
    for (;;) {
        int bl[DC];
#pragma unroll
        for (int k = 0; k < DC; ++k) bl[k] = nb[k];
        const int jn = j + kDecodeBlock;
        if (jn < m) {
#pragma unroll
            for (int k = 0; k < DC; ++k) nb[k] = k < c.max_dc ? c.chk_bits[k * c.m_pad + jn] : -1;
        }
        uint4 st = make_uint4(0, 0, 0, 0);
        uint32_t zp = 0;
        if (SRC == kSrcGeneral) {
            st = cst[j];
            if (sc) zp = czf[j];
        }
        float m1 = __builtin_inff(), m2 = __builtin_inff();
        uint32_t idx = 0xffu, sg = 0, zf = 0;
#pragma unroll
        for (int k = 0; k < DC; ++k) {
            if (bl[k] >= 0) {
                float x = total[bl[k]];
                if (SRC == kSrcGeneral) {
                    x = x - ms_msg<CLAMP>(st, (uint32_t)k, scale, off, thr);
                    if (CLAMP) x = clamp_msg(x, thr);
                    // self-correction: the previous b2c nonzero, this one too,
                    // signs differ -> erased
                    if (sc && !((zp >> k) & 1u) && x != 0.0f && (x < 0.0f) != (((st.z >> k) & 1u) != 0u)) x = 0.0f;
                }
                const float a = fabsf(x);
                sg |= (x < 0.0f ? 1u : 0u) << k;
                zf |= (x == 0.0f ? 1u : 0u) << k;
                if (a < m1) {
                    m2 = m1;
                    m1 = a;
                    idx = (uint32_t)k;
                } else if (a < m2) {
                    m2 = a;
                }
            }
        }
        const uint32_t sbit = (tsyn[j >> 5] >> (j & 31)) & 1u;
        const uint32_t par = sbit ^ ((uint32_t)__popc(sg) & 1u);
        cst[j] = make_uint4(__float_as_uint(m1), __float_as_uint(m2), sg, idx | (par << 31));
        if (sc) czf[j] = zf;
        j = jn;
        if (j >= m) break;
    }
}

// fold_first_message: when the second table is also in use, nothing reads the
// first iteration's stored messages (the second check phase takes its inputs
// from the table), so the first check phase is skipped and the first bit phase
// rebuilds each message from one sign bit per check (qsyn, the sign of P_j,
// computed in the prologue from Bob's bits) and the bit's own LLR sign.
//
// First check phase of the QKD path (QKD_LDPC_irregular, :398-425 -> :220-249
// at it = 0), where b2c = LLR_i = bob_i ? -log_p : +log_p for every edge. Then
//   t_i = tanh(LLR_i / 2) = sign_i * T,  T = |tanh(log_p / 2)|  (tanh is odd)
//   P   = (s_j ? -1 : 1) * t_0 * ... * t_{d-1}: binary64 products round on
//         magnitudes only, so |P| = M_d = (((T * T) * T) ...) and
//         sign(P) = s_j ^ sign_0 ^ ... ^ sign_{d-1}
//   c2b = clamp(2 atanh(P / t_i)) = sign(P) ^ sign_i times
//         C_d = clamp(2 atanh(M_d / T))            (atanh and clamp are odd)
// so every first-iteration message is +-C_d, bit for bit; the host evaluates
// C_d with the same tanh/atanh restatement (decode_keys). sign_i is the sign
// bit of the LLR in `total` (also right for log_p <= 0 and for +-0).
__device__ __forceinline__ void first_check_phase(const uint2* __restrict__ plan, const uint32_t* tsyn,
                                                  const double* total, const double* ctab,
                                                  double* __restrict__ c2b, int n_tasks, int n_pad, int wave,
                                                  int lane) {
    constexpr int NW = kDecodeBlock / 64;
    // kPlanGroup tasks per trip: their plan words are loaded together (the
    // plan is padded, so the loads need no bounds test); stores are predicated.
    for (int t0 = wave; t0 < n_tasks; t0 += NW * kPlanGroup) {
        uint2 w[kPlanGroup];
#pragma unroll
        for (int u = 0; u < kPlanGroup; ++u) w[u] = plan[(t0 + u * NW) * 64 + lane];
#pragma unroll
        for (int u = 0; u < kPlanGroup; ++u) {
            const int t = t0 + u * NW;
            if (t >= n_tasks) break;
            const uint32_t bit = pw_bit(w[u]);
            const uint32_t j = pw_chk(w[u]);
            const uint32_t sg = (uint32_t)qkdm::hi32(total[bit]) >> 31;
            const uint32_t sp = ((tsyn[j >> 5] >> (j & 31)) & 1u) ^ (uint32_t)seg_parity(__ballot(sg), w[u]);
            const double cm = ctab[pw_deg(w[u])];
            c2b[pw_row(w[u]) * n_pad + bit] = (sp ^ sg) ? -cm : cm;
        }
    }
}

// Flooding sum-product decode of whole frames, one frame per workgroup at a
// time (reference sum_product_decoding_irregular, qkd_ldpc_algorithm.cpp:175-345;
// the regular twin :3-173 is the same arithmetic).
//
// Message store: the c2b messages of the frame live bit-major in global memory,
// c2b[k * n_pad + i] = message from the k-th check (ascending) of bit i, i.e.
// the reference's c2b[i][k] layout transposed for coalescing (:192-205). The
// check phase's gather/scatter of it overlaps its transcendental arithmetic;
// the bit phase streams it. (A plan-order store, coalesced in the check phase
// and gathered in the bit phase, measured 10 % slower overall: the gathers
// then stall a phase with nothing to overlap.)
//
// Per iteration:
//  check phase (check_phase above), one edge per lane, wave tasks of whole
//    checks (qkd_plan.h)
//  bit phase (:256-267), one bit per lane, coalesced rows:
//    total_i = LLR_i + c2b[0][i] + c2b[1][i] + ...  (ascending check order)
//    hard decision z_i = total_i <= 0; if z_i, XOR it into the syndrome bit of
//    each of its checks (LDS bit array; XOR is order-free, so exact)
//  syndrome test (:277-285): compare with the target words, block-wide any()
//
// GT (large codes, N beyond what LDS holds): the bit totals live in global
// scratch instead of LDS; everything else is the same kernel. The tables of
// the QKD path (per-bit LDS indices) and the LDS-state min-sum are not used.
// ERA: the binary64 rule extended to zero LLRs (QKD_FLAG_ERASURES; edge_out);
// kModeClass (qkd_reconcile_adaptive_batch, class bytes in the original bit
// order) always has it.
// VFY (kModeClass): the payload's verification tag from the output loop
// (DecodeArgs::vkey). A template parameter, not a branch on vkey: the branch
// cost every class-mode instantiation SGPR spills and a VGPR, and the DC = 64
// ones scratch (profiles/adapt_verify_kernel_resources.txt).
template <int MODE, int RULE, int DC, bool CLAMP, bool GT, bool ERA = false, bool VFY = false>
__global__ __launch_bounds__(kDecodeBlock) void decode_kernel(DecodeArgs a) {
    using T = typename RuleMsg<RULE>::T;
    static_assert(!VFY || MODE == kModeClass, "payload tags: the class-byte mode");
    static_assert(!ERA || RULE == kRuleSp64, "erasure rule: binary64");
    static_assert(MODE != kModeClass || ERA, "class bytes: always with the erasure rule");
    // the exact QKD-path shortcuts (first/second-iteration tables) exist for
    // the reference rule only
    constexpr bool TABLES = MODE == kModeKeys && RULE == kRuleSp64 && !GT;
    constexpr bool MSL = RULE == kRuleMinSumLds || RULE == kRuleMinSumLdsSc;
    constexpr bool SC = RULE == kRuleMinSumLdsSc;      // self-corrected min-sum
    static_assert(!(MSL && GT), "the LDS-state min-sum keeps its totals in LDS");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const DeviceCode& c = a.code;
    const DecodeLds L(c.n_pad, (c.n + 63) / 64, c.m, DC, a.tab2_entries, GT ? 0 : (int)sizeof(T),
                      MSL ? c.m : 0, (int)sizeof(T), SC);
    uint4* cst = reinterpret_cast<uint4*>(smem + L.cst);
    uint32_t* czf = reinterpret_cast<uint32_t*>(smem + L.czf);
    const int m_words = decode_m_words(c.m);
    T* total;
    if constexpr (GT)
        total = reinterpret_cast<T*>(a.totals + (size_t)blockIdx.x * a.totals_stride);
    else
        total = reinterpret_cast<T*>(smem);
    uint32_t* tsyn = reinterpret_cast<uint32_t*>(smem + L.tsyn);
    uint32_t* xsyn = reinterpret_cast<uint32_t*>(smem + L.xsyn);
    uint32_t* qsyn = reinterpret_cast<uint32_t*>(smem + L.qsyn);
    // QKD path with both tables: the first check phase is folded into the
    // first bit phase (fold_first_message)
    const bool fold1 = TABLES && a.first_table && a.tab2_entries;
    const uint32_t lsign = (uint32_t)qkdm::hi32(a.log_p) >> 31;     // sign bit of log_p
    uint32_t* ctl = reinterpret_cast<uint32_t*>(smem + L.ctl);
    double* ctab = reinterpret_cast<double*>(smem + L.ctab);
    double* tab2 = reinterpret_cast<double*>(smem + L.tab2);
    uint16_t* t2idx = reinterpret_cast<uint16_t*>(smem + L.t2idx);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // wave index as a scalar: task loops and plan addresses stay in SGPRs
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    T* row = reinterpret_cast<T*>(smem + L.tval) + wave * (64 + DC);
    const int n_tasks = c.n_tasks;
    const int n_pad = c.n_pad;
    const uint2* plan = c.plan;
    T* c2b = reinterpret_cast<T*>(a.c2b + (size_t)blockIdx.x * a.c2b_stride);
    const T thr = (T)a.thr;
    const T llr_p = (T)a.log_p;
    uint32_t any_k = 0;
    if (tid == 0) { ctl[2] = 0; ctl[3] = 0; }
    if (TABLES && tid <= kFirstTableDeg) ctab[tid] = a.first_c2b[tid];
    if (TABLES && a.tab2_entries) {
        __syncthreads();
        second_table_fill<CLAMP>(c, ctab, a.log_p, a.thr, tab2, a.tab2_entries);
    }
    PhaseClock pc(a.phase);

    for (;;) {
        pc.mark(4);
        if (tid == 0) {
            // the next frame of the queue: frame k, or with a frame list its
            // k-th entry (past the list: no frame)
            uint32_t k = atomicAdd(a.counter, 1u);
            if (a.frame_list != nullptr) k = k < *a.frame_count ? a.frame_list[k] : a.n_frames;
            ctl[0] = k;
            if (MODE == kModeClass) ctl[1] = 0;      // the frame's payload flips
        }
        for (int w = tid; w < m_words; w += kDecodeBlock) xsyn[w] = 0;
        __syncthreads();
        const uint32_t f = ctl[0];
        if (f >= a.n_frames) break;

        // ---- prologue: the frame's Alice and Bob words staged in LDS (the tanh
        //      rows are free until the first check phase)
        const uint64_t* sw = reinterpret_cast<const uint64_t*>(smem + L.tval);   // [alice | bob]
        // (the target syndrome given by the caller, qkd_reconcile_batch:
        // Bob's words only; uniform over the launch)
        const bool given = MODE == kModeKeys && a.syn != nullptr;
        if (MODE == kModeKeys) {
            uint64_t* w = reinterpret_cast<uint64_t*>(smem + L.tval);
            for (int q = tid; q < (int)a.words; q += kDecodeBlock) {
                if (!given) w[q] = a.alice_w[(size_t)f * a.words + q];
                w[a.words + q] = a.bob_w[(size_t)f * a.words + q];
            }
            __syncthreads();
        }
        // ---- prologue: channel LLRs into LDS (:188 / :400-405); the dummy
        //      column n of idle plan lanes gets 0
        // Bob's bits of this thread's bit-phase rounds (round r: bit tid + r *
        // kDecodeBlock), N <= 32 * kDecodeBlock; the large-code kernels read
        // them from the packed key instead (any N)
        uint32_t bobmask = 0;
        {
            int r = 0;
            for (int i = tid; i < c.n; i += kDecodeBlock, ++r) {
                T l;
                if (MODE == kModeLlr) {
                    l = (T)a.llr[(size_t)f * c.n + i];
                } else if (MODE == kModeClass) {
                    l = (T)class_llr(a.cls[(size_t)f * c.n + i], a.log_p, a.known);
                } else {
                    const uint32_t bb = (uint32_t)((sw[a.words + (i >> 6)] >> (i & 63)) & 1u);
                    if (!GT) bobmask |= bb << r;
                    l = bb ? -llr_p : llr_p;
                }
                total[i] = l;
            }
            if (tid == 0) {
                total[c.n] = 0;
                if (TABLES && a.tab2_entries) t2idx[c.n] = 0;   // idle lanes' table reads
            }
        }
        // ---- prologue: target syndrome bits per check (tsyn) and, on the QKD
        //      path, each check's first-product sign (qsyn, fold_first_message);
        //      thread per check, 64 consecutive checks per wave -> one ballot.
        //      ELL pad entries are -1, so the row loads do not wait for the degree.
        for (int j0 = wave * 64; j0 < c.m; j0 += kDecodeBlock) {
            const int j = j0 + lane;
            const bool ok = j < c.m;
            int sj = 0, qj = 0;
            if (MODE == kModeLlr || MODE == kModeClass) {
                sj = ok ? (a.syn[(size_t)f * c.m + j] != 0) : 0;
            } else {
                // calculate_syndrome_irregular on Alice's key (:413-414), and
                // q_j = s_j ^ syn(bob)_j ^ (deg_j & sign(log_p))
                int bl[DC];
#pragma unroll
                for (int k = 0; k < DC; ++k) bl[k] = (ok && k < c.max_dc) ? c.chk_bits[k * c.m_pad + j] : -1;
                uint32_t pa = 0, pb = 0, deg = 0;
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    const int bit = bl[k];
                    if (bit >= 0) {
                        if (!given) pa ^= (uint32_t)(sw[bit >> 6] >> (bit & 63));
                        pb ^= (uint32_t)(sw[a.words + (bit >> 6)] >> (bit & 63));
                        deg++;
                    }
                }
                if (ok && DC < c.max_dc) {
                    for (int k = DC; k < c.max_dc; ++k) {
                        const int bit = c.chk_bits[k * c.m_pad + j];
                        if (bit >= 0) {
                            if (!given) pa ^= (uint32_t)(sw[bit >> 6] >> (bit & 63));
                            pb ^= (uint32_t)(sw[a.words + (bit >> 6)] >> (bit & 63));
                            deg++;
                        }
                    }
                }
                // (given: s_j is the caller's byte, Alice's parity is not computed)
                if (given) pa = (ok && a.syn[(size_t)f * c.m + j] != 0) ? 1u : 0u;
                sj = (int)(pa & 1u);
                qj = (int)((pa ^ pb ^ (lsign & deg)) & 1u);
            }
            const uint64_t sm = __ballot(sj);
            const uint64_t qm = __ballot(qj);
            if (lane == 0) {
                tsyn[j0 >> 5] = (uint32_t)sm;
                tsyn[(j0 >> 5) + 1] = (uint32_t)(sm >> 32);
                qsyn[j0 >> 5] = (uint32_t)qm;
                qsyn[(j0 >> 5) + 1] = (uint32_t)(qm >> 32);
            }
        }
        __syncthreads();
        pc.mark(0);

        // ---- iterations (:212-330)
        bool done = false;
        uint32_t it = 0;
        for (; it < a.max_it; ++it) {
            bool tabled = false;
            if constexpr (MSL) {
                tabled = true;
                if (it == 0)
                    ms_check_phase<kSrcFirst, CLAMP, DC>(c, tsyn, total, cst, czf, SC, thr, a.ms_scale,
                                                         a.ms_offset);
                else
                    ms_check_phase<kSrcGeneral, CLAMP, DC>(c, tsyn, total, cst, czf, SC, thr, a.ms_scale,
                                                           a.ms_offset);
            }
            if constexpr (TABLES) {
                tabled = true;
                if (it == 0 && fold1)
                    ;   // messages rebuilt from signs in the bit phase (fold_first_message)
                else if (it == 0 && a.first_table)
                    first_check_phase(plan, tsyn, total, ctab, c2b, n_tasks, n_pad, wave, lane);
                else if (it == 1 && a.tab2_entries)
                    check_phase<kSrcTable, CLAMP, DC, RULE>(plan, tsyn, total, t2idx, tab2, c2b, row, n_tasks,
                                                            n_pad, thr, wave, lane, a.ms_scale, a.ms_offset);
                else
                    tabled = false;
            }
            if constexpr (!MSL) {
                if (!tabled) {
                    if (it == 0)
                        check_phase<kSrcFirst, CLAMP, DC, RULE, ERA>(plan, tsyn, total, t2idx, tab2, c2b, row,
                                                                     n_tasks, n_pad, thr, wave, lane, a.ms_scale,
                                                                     a.ms_offset);
                    else
                        check_phase<kSrcGeneral, CLAMP, DC, RULE, ERA>(plan, tsyn, total, t2idx, tab2, c2b, row,
                                                                       n_tasks, n_pad, thr, wave, lane, a.ms_scale,
                                                                       a.ms_offset);
                }
            }
            __syncthreads();
            pc.mark((TABLES && it < 2 && a.first_table) ? 5 + (int)it : 1);
            // bit phase: total_i = LLR_i + sum_k c2b[k][i], ascending checks (:256-267),
            // and the hard decision's syndrome (:277, calculate_syndrome_irregular :476-486).
            // kBitChunk rounds at a time: all their message rows and check indices
            // are loaded before any of them is summed.
            for (int r0 = 0; r0 * kDecodeBlock < c.n; r0 += kBitChunk) {
                T v[kBitChunk][kDvUnroll];
                int32_t jc[kBitChunk][kDvUnroll];
                uint32_t ps[kBitChunk][kDvUnroll];     // MSL: positions in the checks
                int dg[kBitChunk];
#pragma unroll
                for (int u = 0; u < kBitChunk; ++u) {
                    const int i = tid + (r0 + u) * kDecodeBlock;
                    const bool ok = i < c.n;
                    dg[u] = ok ? c.bit_deg[i] : 0;
#pragma unroll
                    for (int k = 0; k < kDvUnroll; ++k) {
                        const bool ld = ok && k < c.max_dv;
                        if constexpr (MSL) {
                            v[u][k] = 0;
                            ps[u][k] = ld ? c.bit_pos[k * n_pad + i] : 0u;
                        } else {
                            v[u][k] = (ld && !(fold1 && it == 0)) ? c2b[k * n_pad + i] : (T)0;
                        }
                        jc[u][k] = ld ? c.bit_chk[k * n_pad + i] : 0;
                    }
                }
#pragma unroll
                for (int u = 0; u < kBitChunk; ++u) {
                    const int r = r0 + u;
                    const int i = tid + r * kDecodeBlock;
                    if (i >= c.n) break;
                    const int deg = dg[u];
                    T acc;
                    if (MODE == kModeLlr) acc = (T)a.llr[(size_t)f * c.n + i];
                    else if (MODE == kModeClass)
                        acc = (T)class_llr(a.cls[(size_t)f * c.n + i], a.log_p, a.known);
                    else if constexpr (GT)
                        acc = ((a.bob_w[(size_t)f * a.words + (i >> 6)] >> (i & 63)) & 1u) ? -llr_p : llr_p;
                    else
                        acc = ((bobmask >> r) & 1u) ? -llr_p : llr_p;
                    if constexpr (TABLES) if (fold1 && it == 0) {
                        // fold_first_message: message of the k-th check j of bit i is
                        // +-C_{d_j} with sign = sign(P_j) ^ sign(LLR_i) (first_check_phase)
                        const uint32_t sgi = ((bobmask >> r) & 1u) ^ lsign;
                        const uint8_t* pd = c.pat_deg + c.bit_pat[i] * c.max_dv;
#pragma unroll
                        for (int k = 0; k < kDvUnroll; ++k) {
                            if (k < deg) {
                                const int j = jc[u][k];
                                const uint32_t sp = (qsyn[j >> 5] >> (j & 31)) & 1u;
                                const double cm = ctab[pd[k]];
                                v[u][k] = (sp ^ sgi) ? -cm : cm;
                            }
                        }
                    }
                    if constexpr (MSL) {
#pragma unroll
                        for (int k = 0; k < kDvUnroll; ++k)
                            if (k < deg) v[u][k] = ms_msg<CLAMP>(cst[jc[u][k]], ps[u][k], a.ms_scale, a.ms_offset, thr);
                    }
#pragma unroll
                    for (int k = 0; k < kDvUnroll; ++k) acc = k < deg ? acc + v[u][k] : acc;
                    if constexpr (MSL) {
                        for (int k = kDvUnroll; k < deg; ++k)
                            acc = acc + ms_msg<CLAMP>(cst[c.bit_chk[k * n_pad + i]], c.bit_pos[k * n_pad + i],
                                                      a.ms_scale, a.ms_offset, thr);
                    } else {
                        for (int k = kDvUnroll; k < deg; ++k) acc = acc + c2b[k * n_pad + i];
                    }
                    total[i] = acc;
                    if constexpr (TABLES) if (a.tab2_entries && it == 0) {
                        // second_table_index: bob bit and the signs of the first messages
                        uint32_t code = (bobmask >> r) & 1u;
#pragma unroll
                        for (int k = 0; k < kTab2MaxDv; ++k)
                            if (k < deg) code |= ((uint32_t)qkdm::hi32(v[u][k]) >> 31) << (1 + k);
                        t2idx[i] = (uint16_t)(c.bit_pat[i] * tab2_stride(c.max_dv) + code * c.max_dv);
                    }
                    if (acc <= 0) {
#pragma unroll
                        for (int k = 0; k < kDvUnroll; ++k)
                            if (k < deg) atomicXor(&xsyn[jc[u][k] >> 5], 1u << (jc[u][k] & 31));
                        for (int k = kDvUnroll; k < deg; ++k) {
                            const int j = c.bit_chk[k * n_pad + i];
                            atomicXor(&xsyn[j >> 5], 1u << (j & 31));
                        }
                    }
                }
            }
            __syncthreads();
            pc.mark(2);
            if constexpr (RULE == kRuleSp64) {
                // TRACE_SUM_PRODUCT (:250-275): this iteration's clamped c2b ("E") and totals ("L")
                if (a.trace) {
                    double* tr = a.trace + (size_t)it * a.trace_stride;
                    const int nm = c.max_dv * n_pad;
                    for (int q = tid; q < nm; q += kDecodeBlock) tr[q] = c2b[q];
                    for (int q = tid; q < c.n; q += kDecodeBlock) tr[nm + q] = total[q];
                }
            }
            // syndrome test (:285): any word differing from the target
            bool mismatch = false;
            for (int w = tid; w < m_words; w += kDecodeBlock) {
                mismatch |= xsyn[w] != tsyn[w];
                xsyn[w] = 0;
            }
            const bool any_mismatch = block_any(mismatch, ctl + 2, any_k);
            pc.mark(3);
            if (!any_mismatch) {
                done = true;
                break;
            }
        }

        // ---- outputs: SP_result + last hard decision (+ keys_match)
        bool key_mismatch = false;
        uint32_t nflip = 0;
        constexpr bool vfy = VFY;     // (kModeClass: the payload's verification tag)
        uint64_t vacc = 0;
        for (int i = tid; i < c.n; i += kDecodeBlock) {
            const uint8_t d = total[i] <= 0 ? 1 : 0;
            if (a.bits_out) a.bits_out[(size_t)f * c.n + i] = d;
            if (MODE == kModeClass) {
                // the payload of the decision and its flips against Bob's (class bit 0)
                const int32_t k = a.src[i];
                if (k >= 0) {
                    a.payload_out[(size_t)f * a.n_payload + (uint32_t)k] = d;
                    nflip += (uint32_t)(d ^ (a.cls[(size_t)f * c.n + i] & 1u));
                    if (vfy) vacc ^= class_verify_window(a.vkey, (uint32_t)k, d);
                }
            }
            if (MODE == kModeKeys && !given) {
                const uint64_t w = a.alice_w[(size_t)f * a.words + (i >> 6)];
                key_mismatch |= (uint8_t)((w >> (i & 63)) & 1u) != d;
            }
        }
        if (MODE == kModeKeys) {
            __syncthreads();
            const bool km = block_any(key_mismatch, ctl + 2, any_k);
            if (tid == 0 && a.key_ok) a.key_ok[f] = km ? 0 : 1;   // arrays_equal (:433)
        }
        if (MODE == kModeClass && (a.flips || vfy)) {
            if (a.flips && nflip) atomicAdd(ctl + 1, nflip);
            // the waves' XORs in the tanh rows (free since the last check phase,
            // and until the next frame's first one)
            uint64_t* const vred = reinterpret_cast<uint64_t*>(smem + L.tval);
            if (vfy) {
                const uint64_t wx = wave_xor64(vacc);
                if (lane == 0) vred[wave] = wx;
            }
            __syncthreads();
            if (tid == 0 && a.flips) a.flips[f] = ctl[1];
            if (tid == 0 && vfy) class_verify_finish(vred, a.vmask, a.vtags, a.valice, a.vok, f, done);
        }
        if (tid == 0) {
            a.iters[f] = done ? it + 1 : a.max_it;
            a.sp_ok[f] = done ? 1 : 0;
        }
        __syncthreads();
    }
    pc.flush();
}

// The instantiations of decode_kernel, by key (qkd_launch.h KernelKey).
// Buckets: 4 / 6 / 8 / 16 / 64; the LDS-state min-sum rules end at 32 (sign
// bits in one word) and have no large-code form; the large-code kernels (GT)
// 16 / 64. (The compiler emits the kernels in the order these functions name
// them.)
template <int MODE, int RULE, bool CLAMP, bool GT, bool ERA, bool VFY>
static DecodeFn classic_bucket(int dc) {
    if constexpr (!GT) {
        if (dc == 4) return decode_kernel<MODE, RULE, 4, CLAMP, false, ERA, VFY>;
        if (dc == 6) return decode_kernel<MODE, RULE, 6, CLAMP, false, ERA, VFY>;
        if (dc == 8) return decode_kernel<MODE, RULE, 8, CLAMP, false, ERA, VFY>;
    }
    if (dc == 16) return decode_kernel<MODE, RULE, 16, CLAMP, GT, ERA, VFY>;
    if constexpr (RULE == kRuleMinSumLds || RULE == kRuleMinSumLdsSc) {
        if (dc == 32) return decode_kernel<MODE, RULE, 32, CLAMP, GT, ERA, VFY>;
    } else {
        if (dc == 64) return decode_kernel<MODE, RULE, 64, CLAMP, GT, ERA, VFY>;
    }
    return nullptr;
}
template <int MODE, int RULE, bool GT, bool ERA = false, bool VFY = false>
static DecodeFn classic_clamp(const KernelKey& k) {
    return k.clamp ? classic_bucket<MODE, RULE, true, GT, ERA, VFY>(k.dc)
                   : classic_bucket<MODE, RULE, false, GT, ERA, VFY>(k.dc);
}
template <int MODE, bool GT>
static DecodeFn classic_rule(const KernelKey& k) {
    switch (k.rule) {
        case kRuleSp32: return classic_clamp<MODE, kRuleSp32, GT>(k);
        case kRuleMinSum: return classic_clamp<MODE, kRuleMinSum, GT>(k);
        case kRuleMinSumLds:
            if constexpr (!GT) return classic_clamp<MODE, kRuleMinSumLds, false>(k);
            break;
        case kRuleMinSumLdsSc:
            if constexpr (!GT) return classic_clamp<MODE, kRuleMinSumLdsSc, false>(k);
            break;
        case kRuleSp64: return classic_clamp<MODE, kRuleSp64, GT>(k);
    }
    return nullptr;
}
// the erasure rule's kernels (binary64): the LLR path with QKD_FLAG_ERASURES
// and the class-byte path (always; VFY: the instantiations that take the
// payload's tag, DecodeArgs::vkey)
template <int MODE, bool VFY>
static DecodeFn classic_era(const KernelKey& k) {
    return k.gt ? classic_clamp<MODE, kRuleSp64, true, true, VFY>(k) : classic_clamp<MODE, kRuleSp64, false, true, VFY>(k);
}

DecodeFn classic_kernel(const KernelKey& k) {
    if (k.kind != kKernelClassic || k.spec || k.lng) return nullptr;
    if (k.era || k.mode == kModeClass) {
        if (!k.era || k.rule != kRuleSp64) return nullptr;
        if (k.mode == kModeClass) return k.vfy ? classic_era<kModeClass, true>(k) : classic_era<kModeClass, false>(k);
        return k.mode == kModeLlr && !k.vfy ? classic_era<kModeLlr, false>(k) : nullptr;
    }
    if (k.vfy || (k.mode != kModeLlr && k.mode != kModeKeys)) return nullptr;
    if (k.gt) return k.mode == kModeLlr ? classic_rule<kModeLlr, true>(k) : classic_rule<kModeKeys, true>(k);
    return k.mode == kModeLlr ? classic_rule<kModeLlr, false>(k) : classic_rule<kModeKeys, false>(k);
}

}  // namespace qkd
