// qkd_layout.h — everything a code object derives from H on the host: the
// validated adjacency, the ELL arrays, the check-phase wave plan, the split
// kernels' internal bit order and the arrays in it, the check-lane plans and
// the key-generation jump tables. No HIP header (also compiled by the native
// tests); host.cpp build_code uploads the result as it is.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../include/qkd_ldpc.h"
#include "qkd_limits.h"
#include "qkd_plan.h"
#include "qkd_rng.h"

namespace qkd {

// (host.cpp; a native test supplies its own)
qkd_status set_error(qkd_status s, const char* fmt, ...);

// the kernels' uint2, as the host lays it out
struct U2 {
    uint32_t x, y;
};

// the check-lane plan of the speculative check phases (qkd_plan.h
// CheckLanePlan), slot-addressed on the host. slot: (cl_tasks + pad) * cl_dc *
// 64 slot indices (qkdp::kNoSlot for dead entries); chk: the lanes' check words
// as the builder made them (qkdp::encode_chk; 0: none); rem: the remainder's
// plan in plan_slot's form
struct ClHost {
    int32_t cl_tasks = 0, rem_tasks = 0;
    std::vector<uint32_t> slot, chk;
    std::vector<U2> rem;
};

// The part of the layout a code object keeps on the host (qkd_code's base).
// An array that is empty is not uploaded: its device pointer stays null, which
// is how the launcher reads "this code has no such view". The arrays' meanings:
// DeviceCode (qkd_internal.h).
struct CodeHost {
    int32_t n = 0, m = 0, e = 0;
    int32_t max_dv = 0, max_dc = 0, min_dc = 0, min_dv = 0, is_regular = 0;
    int32_t n_pad = 0, m_pad = 0;
    int32_t n_tasks = 0;
    std::vector<int32_t> check_ptr, check_idx, bit_ptr, bit_idx;
    int32_t n_pat = 0;                  // 0: too many degree patterns for the table
    std::vector<uint8_t> pat_deg;
    // the split kernels' internal bit order (empty without the split view)
    std::vector<int32_t> perm;
    int32_t chk_rs = 0, ilv_rs = 0;     // row strides of chk_rows16 / ilv_slots, 0: none
    // the slot plan (its encoded forms by LDS layout: plan_for_layout, launch.hip)
    std::vector<U2> plan_slot;
    // the check-lane plans (cl_dc = their bucket, 0: none -- check degree past
    // 6 or no bit_code): [0] the split form (whole rounds of check-lane tasks
    // plus an edge-lane remainder), [1] the pure form (every check on a lane;
    // A/B runs)
    int32_t cl_dc = 0;
    ClHost cl_host[2];
    // parallel key generation. keygen_fast_kernel: lane l of a frame's
    // kKeygenLanes-lane slice starts at draw l * keygen_chunk; jump[b] =
    // T^(chunk * 2^b), jpoly[l] = x^(l * chunk) mod P (4 words) the same jumps
    // as polynomials. keygen_split_kernel (the default): a frame's lane l of
    // wave 0 draws Alice's bits [l * kg_cb, (l + 1) * kg_cb), its lane l of
    // wave 1 the shuffle draws from N + l * kg_cs; jpoly2[w * kKgSplitLanes +
    // l] = x^(start) mod P
    uint32_t keygen_chunk = 0, kg_cb = 0, kg_cs = 0;
};

// ... and what is only uploaded.
struct CodeLayout : CodeHost {
    std::vector<int32_t> chk_bits, bit_chk;
    std::vector<uint8_t> chk_deg, bit_pos, bit_deg;
    std::vector<uint32_t> chk_odd;
    std::vector<uint16_t> bit_pat;
    std::vector<U2> plan;
    // the split kernels' data, only for codes they take (split)
    bool split = false;
    std::vector<int32_t> inv, bit_chk_s;
    std::vector<uint8_t> bit_deg_s;
    std::vector<uint16_t> bit_pat_s, chk_rows16;
    std::vector<uint64_t> bit_code;
    std::vector<uint32_t> ilv_slots;
    std::vector<uint64_t> jump, jpoly, jpoly2;
};

inline int32_t round_up(int32_t x, int32_t a) { return (x + a - 1) / a * a; }

// The internal order's second pass (internal_bit_order): inside each task's run
// of last-row bits the order is free (the run stays one run of slots), and it
// decides the LDS banks of the OTHER rows' slots of those bits, which the
// check phases read and write scattered: slot x = row * n_pad + bit sits in
// the bank pair x mod 32 (8-byte slots over 64 four-byte banks), and a
// half-wave's accesses serialise on the busiest pair. A deterministic local
// search swaps bits within runs while the summed excess over the tasks'
// half-waves (busiest pair's count - 1, not-last-row edges) does not grow
// (tools/bank_model.py: 3.06 -> ~1.1 extra bank cycles per task for the
// N = 10240 code).
inline void bank_balance_runs(int32_t n, int32_t n_pad, const std::vector<int32_t>& bdeg,
                              const qkdp::WavePlan& plan, std::vector<int32_t>& perm, std::vector<int32_t>& inv) {
    const int32_t n_tasks = plan.n_tasks;
    std::vector<std::vector<int32_t>> tasks_of(n);
    std::vector<std::vector<int32_t>> runs(n_tasks);
    for (int32_t t = 0; t < n_tasks; ++t)
        for (int l = 0; l < 64; ++l) {
            const uint32_t w = plan.word[(size_t)t * 64 + l];
            const uint32_t b = w & qkdp::kPlanBitMask;
            if (b >= (uint32_t)n) continue;
            if ((int32_t)(w >> 24) == bdeg[b] - 1) runs[t].push_back((int32_t)b);
            if (tasks_of[b].empty() || tasks_of[b].back() != t) tasks_of[b].push_back(t);
        }
    // (the edges of a task are distinct slots; idle lanes are skipped)
    auto cost = [&](int32_t t) {
        int ex = 0;
        for (int h = 0; h < 2; ++h) {
            int cnt[32] = {0};
            for (int l = h * 32; l < h * 32 + 32; ++l) {
                const uint32_t w = plan.word[(size_t)t * 64 + l];
                const uint32_t b = w & qkdp::kPlanBitMask;
                const int32_t row = (int32_t)(w >> 24);
                if (b >= (uint32_t)n || row == bdeg[b] - 1) continue;
                cnt[((uint32_t)row * (uint32_t)n_pad + (uint32_t)inv[b]) & 31u]++;
            }
            int mx = 0;
            for (int k = 0; k < 32; ++k) mx = std::max(mx, cnt[k]);
            ex += mx > 0 ? mx - 1 : 0;
        }
        return ex;
    };
    std::vector<int> cur(n_tasks);
    for (int32_t t = 0; t < n_tasks; ++t) cur[t] = cost(t);
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    const int64_t iters = std::min<int64_t>(200000, (int64_t)20 * n);
    std::vector<int32_t> aff;
    std::vector<int> nc;
    for (int64_t it = 0; it < iters; ++it) {
        const auto& run = runs[next() % (uint64_t)n_tasks];
        if (run.size() < 2) continue;
        const int32_t a = run[next() % run.size()], b = run[next() % run.size()];
        if (a == b) continue;
        aff.clear();
        for (int32_t t : tasks_of[a]) aff.push_back(t);
        for (int32_t t : tasks_of[b]) aff.push_back(t);
        std::sort(aff.begin(), aff.end());
        aff.erase(std::unique(aff.begin(), aff.end()), aff.end());
        int before = 0;
        for (int32_t t : aff) before += cur[t];
        std::swap(inv[a], inv[b]);
        int after = 0;
        nc.resize(aff.size());
        for (size_t k = 0; k < aff.size(); ++k) after += nc[k] = cost(aff[k]);
        if (after <= before) {
            for (size_t k = 0; k < aff.size(); ++k) cur[aff[k]] = nc[k];
        } else {
            std::swap(inv[a], inv[b]);
        }
    }
    for (int32_t i = 0; i < n; ++i) perm[inv[i]] = i;
}

// The split kernels' internal bit order (decode_split.hip, DeviceCode::perm):
// bits numbered in the order the check-phase plan meets their LAST edge (row
// deg - 1), task by task, lane by lane. Each task's last-row edges then have
// consecutive internal bits, and so consecutive message slots (row * n_pad +
// bit): the last row is the one the split store keeps in global memory, so a
// check phase's global accesses come in runs of whole lines instead of one
// line per edge, while the bit phase, which walks the internal order, stays
// coalesced. Then bank_balance_runs orders each run for the LDS banks.
// perm[internal] = bit, inv[bit] = internal; bits without edges go last.
// mode (diagnostics, QKD_BIT_ORDER): "identity" keeps the original order,
// "runs" skips the bank pass.
inline void internal_bit_order(int32_t n, int32_t n_pad, const std::vector<int32_t>& bdeg,
                               const qkdp::WavePlan& plan, std::vector<int32_t>& perm, std::vector<int32_t>& inv,
                               const char* mode) {
    int32_t nx = 0;
    for (size_t k = 0; k < (size_t)plan.n_tasks * 64; ++k) {
        const uint32_t b = plan.word[k] & qkdp::kPlanBitMask;
        if (b < (uint32_t)n && (int32_t)(plan.word[k] >> 24) == bdeg[b] - 1 && inv[b] < 0) {
            inv[b] = nx;
            perm[nx++] = (int32_t)b;
        }
    }
    for (int32_t i = 0; i < n; ++i)
        if (inv[i] < 0) {
            inv[i] = nx;
            perm[nx++] = i;
        }
    if (mode && !strcmp(mode, "identity")) {
        for (int32_t i = 0; i < n; ++i) perm[i] = inv[i] = i;
    } else if (!(mode && !strcmp(mode, "runs"))) {
        bank_balance_runs(n, n_pad, bdeg, plan, perm, inv);
    }
}

// The check-side CSR's invariants (qkd_code_create): cptr[0] = 0, monotone
// offsets, at least one edge, bit indices in range, every row strictly
// ascending (QKD_ERR_UNSORTED when a row descends: the reference would
// silently mis-route its messages). Fills bdeg[n] (bit
// degrees) and max_dc.
inline qkd_status validate_csr(int32_t n, int32_t m, const int32_t* cptr, const int32_t* cidx,
                               std::vector<int32_t>& bdeg, int32_t& max_dc) {
    if (n <= 0 || m <= 0 || !cptr || !cidx)
        return set_error(QKD_ERR_INVALID_ARG, "qkd_code_create: n=%d m=%d, null adjacency", n, m);
    if (cptr[0] != 0) return set_error(QKD_ERR_BAD_CODE, "check_ptr[0] must be 0");
    for (int32_t j = 0; j < m; ++j)
        if (cptr[j + 1] < cptr[j])
            return set_error(QKD_ERR_BAD_CODE, "check_ptr not monotone at check %d", j);
    if (cptr[m] <= 0) return set_error(QKD_ERR_BAD_CODE, "code has no edges");
    max_dc = 0;
    bdeg.assign(n, 0);
    for (int32_t j = 0; j < m; ++j) {
        const int32_t d = cptr[j + 1] - cptr[j];
        max_dc = std::max(max_dc, d);
        for (int32_t k = cptr[j]; k < cptr[j + 1]; ++k) {
            const int32_t b = cidx[k];
            if (b < 0 || b >= n)
                return set_error(QKD_ERR_BAD_CODE, "check %d: bit index %d out of range [0,%d)", j, b, n);
            if (k > cptr[j] && cidx[k - 1] >= b)
                return set_error(cidx[k - 1] == b ? QKD_ERR_BAD_CODE : QKD_ERR_UNSORTED,
                                 "check %d: bit list not strictly ascending at slot %d (%d after %d)",
                                 j, k - cptr[j], b, cidx[k - 1]);
            bdeg[b]++;
        }
    }
    return QKD_OK;
}

// The bit side of a validated CSR: iterating the checks in ascending order
// makes every bit's row ascending. krow[k] (optional) = the position of edge
// k's check in its bit's row.
inline void bit_side_lists(int32_t n, int32_t m, const int32_t* cptr, const int32_t* cidx,
                           const std::vector<int32_t>& bdeg, std::vector<int32_t>& bptr,
                           std::vector<int32_t>& bidx, int32_t* krow) {
    bptr.assign(n + 1, 0);
    for (int32_t i = 0; i < n; ++i) bptr[i + 1] = bptr[i] + bdeg[i];
    bidx.assign(cptr[m], 0);
    std::vector<int32_t> fill(n, 0);
    for (int32_t j = 0; j < m; ++j)
        for (int32_t k = cptr[j]; k < cptr[j + 1]; ++k) {
            const int32_t b = cidx[k];
            if (krow) krow[k] = fill[b];
            bidx[bptr[b] + fill[b]++] = j;
        }
}

// plan words with the message slot row * n_pad + internal bit in place of
// {bit, row} (idle lanes: the dummy column n's slot)
inline uint32_t plan_word_slot(uint32_t word, int32_t n, int32_t n_pad, const std::vector<int32_t>& inv) {
    const uint32_t b = word & qkdp::kPlanBitMask;
    return (word >> 24) * (uint32_t)n_pad + (b < (uint32_t)n ? (uint32_t)inv[b] : b);
}

// Validate the check-side CSR and derive the layout. bit_order: QKD_BIT_ORDER's
// value or nullptr (internal_bit_order's mode). order_only
// (qkd_debug_bit_order): no size limits, and only the wave plan (plan, n_tasks),
// n_pad and the internal order (perm, inv; for any size) are derived.
inline qkd_status derive_code_layout(int32_t n, int32_t m, const int32_t* cptr, const int32_t* cidx,
                                     const char* bit_order, bool order_only, CodeLayout& L) {
    std::vector<int32_t> bdeg;
    int32_t max_dc = 0;
    qkd_status vs = validate_csr(n, m, cptr, cidx, bdeg, max_dc);
    if (vs != QKD_OK) return vs;
    const int32_t e = cptr[m];
    int32_t max_dv = 0;
    for (int32_t i = 0; i < n; ++i) max_dv = std::max(max_dv, bdeg[i]);
    if (!order_only) {
        if (max_dc > kMaxCheckDegree)
            return set_error(QKD_ERR_UNSUPPORTED, "check degree %d exceeds %d", max_dc, kMaxCheckDegree);
        if (max_dv > qkdp::kPlanMaxBitDegree)
            return set_error(QKD_ERR_UNSUPPORTED, "bit degree %d exceeds %d", max_dv, qkdp::kPlanMaxBitDegree);
        if (n >= qkdp::kPlanMaxBits)
            return set_error(QKD_ERR_UNSUPPORTED, "N=%d exceeds the plan limit %d", n, qkdp::kPlanMaxBits - 1);
        if (m > qkdp::kPlanMaxChecks)
            return set_error(QKD_ERR_UNSUPPORTED, "M=%d exceeds the plan limit %d", m, qkdp::kPlanMaxChecks);
    }
    L.n = n;
    L.m = m;
    L.e = e;
    L.max_dc = max_dc;
    L.min_dc = max_dc;
    for (int32_t j = 0; j < m; ++j) L.min_dc = std::min(L.min_dc, cptr[j + 1] - cptr[j]);
    L.max_dv = max_dv;
    L.min_dv = *std::min_element(bdeg.begin(), bdeg.end());
    L.check_ptr.assign(cptr, cptr + m + 1);
    L.check_idx.assign(cidx, cidx + e);
    std::vector<int32_t> krow(e, 0);
    bit_side_lists(n, m, cptr, cidx, bdeg, L.bit_ptr, L.bit_idx, krow.data());
    const int32_t n_pad = L.n_pad = round_up(n + 1, 64);   // column n: dummy target of idle plan lanes
    const int32_t m_pad = L.m_pad = round_up(m, 64);
    qkdp::WavePlan plan;
    if (!qkdp::build_wave_plan(n, m, cptr, cidx, krow.data(), plan))
        return set_error(QKD_ERR_UNSUPPORTED, "check degree outside [1, %d]", qkdp::kPlanMaxDegree);
    L.n_tasks = plan.n_tasks;
    L.plan.resize(plan.word.size());
    for (size_t k = 0; k < plan.word.size(); ++k) L.plan[k] = U2{plan.word[k], plan.seg[k]};
    // The split kernels' data (decode_split.hip, decode_ilv.hip), only for
    // codes they take (N <= kMaxBitsSplitLong, M <= kMaxChecksSplit; past
    // kMaxBitsSplit only the frame-interleaved decoder and its exact hand-off
    // kernel; the launcher checks the same): larger codes run the classic
    // kernel on the original order, so the internal bit order (its bank pass
    // searches up to 200k moves) and the internal-order arrays are not derived
    // for them.
    L.split = order_only || (n <= kMaxBitsSplitLong && m <= kMaxChecksSplit);
    std::vector<int32_t>& perm = L.perm;
    std::vector<int32_t>& inv = L.inv;
    if (L.split) {
        perm.assign(n, 0);
        inv.assign(n, -1);
        internal_bit_order(n, n_pad, bdeg, plan, perm, inv, bit_order);
    }
    if (order_only) return QKD_OK;

    // the ELL arrays
    L.chk_bits.assign((size_t)max_dc * m_pad, -1);
    L.chk_deg.assign(m, 0);
    L.bit_chk.assign((size_t)max_dv * n_pad, -1);
    L.bit_pos.assign((size_t)max_dv * n_pad, 0);
    L.bit_deg.assign(n, 0);
    const std::vector<uint8_t>& chk_deg = L.chk_deg;
    for (int32_t j = 0; j < m; ++j) {
        L.chk_deg[j] = (uint8_t)(cptr[j + 1] - cptr[j]);
        for (int32_t k = cptr[j]; k < cptr[j + 1]; ++k) {
            const int32_t slot = k - cptr[j];
            const int32_t b = cidx[k];
            L.chk_bits[(size_t)slot * m_pad + j] = b;
            L.bit_chk[(size_t)krow[k] * n_pad + b] = j;
            L.bit_pos[(size_t)krow[k] * n_pad + b] = (uint8_t)slot;
        }
    }
    // odd-degree checks as syndrome words (qkd_decode.h decode_m_words)
    L.chk_odd.assign((size_t)((m + 63) / 64) * 2, 0u);
    for (int32_t j = 0; j < m; ++j)
        if (chk_deg[j] & 1u) L.chk_odd[j >> 5] |= 1u << (j & 31);
    // degree patterns of the bits: the ascending checks' degrees
    L.n_pat = 0;
    if (max_dv <= kTab2MaxDv) {
        L.bit_pat.assign(n, 0);
        std::map<std::vector<uint8_t>, int> ids;
        for (int32_t i = 0; i < n; ++i) {
            std::vector<uint8_t> key(max_dv, 0);
            for (int32_t k = L.bit_ptr[i]; k < L.bit_ptr[i + 1]; ++k) key[k - L.bit_ptr[i]] = chk_deg[L.bit_idx[k]];
            auto it = ids.find(key);
            if (it == ids.end()) {
                it = ids.emplace(key, (int)ids.size()).first;
                L.pat_deg.insert(L.pat_deg.end(), key.begin(), key.end());
            }
            L.bit_pat[i] = (uint16_t)it->second;
        }
        L.n_pat = (int32_t)ids.size();
        if ((size_t)L.n_pat * tab2_stride(max_dv) > (size_t)kTab2MaxEntries) {
            L.n_pat = 0;
            L.pat_deg.clear();
            L.bit_pat.clear();
        }
    }
    bool reg = true;
    for (int32_t i = 0; i < n; ++i) {
        L.bit_deg[i] = (uint8_t)bdeg[i];
        reg = reg && bdeg[i] == bdeg[0];
    }
    for (int32_t j = 0; j < m; ++j) reg = reg && chk_deg[j] == chk_deg[0];
    L.is_regular = reg ? 1 : 0;

    if (L.split) {
        // the per-bit arrays in the internal order (the split kernels' DeviceCode view)
        L.bit_chk_s.assign(L.bit_chk.size(), -1);
        L.bit_deg_s.assign(n, 0);
        for (int32_t q = 0; q < n; ++q) {
            const int32_t b = perm[q];
            L.bit_deg_s[q] = L.bit_deg[b];
            for (int32_t k = 0; k < max_dv; ++k)
                L.bit_chk_s[(size_t)k * n_pad + q] = L.bit_chk[(size_t)k * n_pad + b];
        }
        // frame_syn_sliced_kernel's check rows (N < 65535, check degree <= 16):
        // each check's bits as one or two 16-byte rows of uint16 (0xffff past
        // the row), one load per row
        if (n < 65535 && max_dc <= 16) {
            const int32_t rs = L.chk_rs = max_dc <= 8 ? 8 : 16;
            L.chk_rows16.assign((size_t)m * rs, 0xffff);
            for (int32_t j = 0; j < m; ++j)
                for (int32_t k = cptr[j]; k < cptr[j + 1]; ++k)
                    L.chk_rows16[(size_t)j * rs + (k - cptr[j])] = (uint16_t)cidx[k];
        }
        if (L.n_pat > 0) {
            // (padded past the last whole load batch of the bit phases: they load
            // every round of a batch unconditionally, decode_split.hip)
            L.bit_pat_s.assign((size_t)round_up(n, kDecodeBlock) + kBitPadRounds * kDecodeBlock, 0);
            for (int32_t q = 0; q < n; ++q) L.bit_pat_s[q] = L.bit_pat[perm[q]];
        }
        // packed per-bit words for the speculative bit phases (qkd_internal.h),
        // split kernels only: in the internal order
        bool packable = m <= 65536 && max_dv <= 3;
        for (int32_t j = 0; j < m && packable; ++j) packable = chk_deg[j] >= 1 && chk_deg[j] <= 16;
        if (packable) {
            // (padded with zeros to whole kDecodeBlock rounds and kBitPadRounds
            // more: the bit phases load whole batches of rounds unconditionally,
            // decode_split.hip spec_bit_phase / sp32_bit_phase)
            L.bit_code.assign(std::max((size_t)n_pad, (size_t)round_up(n, kDecodeBlock)) +
                                  (size_t)kBitPadRounds * kDecodeBlock, 0);
            for (int32_t q = 0; q < n; ++q) {
                const int32_t i = perm[q];
                uint64_t w = (uint64_t)bdeg[i] << 48;
                for (int32_t k = 0; k < bdeg[i]; ++k) {
                    const int32_t j = L.bit_chk[(size_t)k * n_pad + i];
                    w |= (uint64_t)j << (16 * k);
                    w |= (uint64_t)(chk_deg[j] - 1) << (50 + 4 * k);
                }
                L.bit_code[q] = w;
            }
            // the frame-interleaved decoder's check rows (decode_ilv.hip): each
            // edge's message line, row * n_pad + internal bit, in the check's order
            const int32_t rs = L.ilv_rs = max_dc <= 8 ? 8 : 16;
            L.ilv_slots.assign((size_t)m * rs, 0xffffffffu);
            for (int32_t j = 0; j < m; ++j)
                for (int32_t k = cptr[j]; k < cptr[j + 1]; ++k)
                    L.ilv_slots[(size_t)j * rs + (k - cptr[j])] = (uint32_t)krow[k] * (uint32_t)n_pad + (uint32_t)inv[cidx[k]];
        }
        // the same plan slot-addressed for the split kernels
        L.plan_slot = L.plan;
        for (size_t k = 0; k < plan.word.size(); ++k) L.plan_slot[k].x = plan_word_slot(plan.word[k], n, n_pad, inv);
        // the speculative check phases' check-lane plans (qkd_plan.h), for
        // the buckets that have the kernel (decode_split.hip
        // spec_check_phase_lanes): slot-addressed like plan_slot
        if (packable && max_dc <= 6) {
            const int dc = max_dc <= 4 ? 4 : 6;
            std::vector<int32_t> slot_of(e);
            for (int32_t k = 0; k < e; ++k) slot_of[k] = krow[k] * n_pad + inv[cidx[k]];
            for (int form = 0; form < 2; ++form) {
                qkdp::CheckLanePlan cl;
                if (!qkdp::build_check_lane_plan(n, m, cptr, cidx, krow.data(), dc, kDecodeBlock / 64, form == 1, cl))
                    return set_error(QKD_ERR_UNSUPPORTED, "check-lane plan: check degree outside [1, %d]", dc);
                ClHost& h = L.cl_host[form];
                h.cl_tasks = cl.n_tasks;
                h.rem_tasks = cl.rem.n_tasks;
                h.slot.resize(cl.edge.size());
                for (size_t k = 0; k < cl.edge.size(); ++k)
                    h.slot[k] = cl.edge[k] < 0 ? qkdp::kNoSlot : (uint32_t)slot_of[cl.edge[k]];
                h.chk = cl.chkw;
                h.rem.resize(cl.rem.word.size());
                for (size_t k = 0; k < cl.rem.word.size(); ++k)
                    h.rem[k] = U2{plan_word_slot(cl.rem.word[k], n, n_pad, inv), cl.rem.seg[k]};
            }
            L.cl_dc = dc;
        }
    }
    // Key-generation jump-ahead: chunk = draws per lane, a multiple of 64 so
    // every lane's Alice bits fill whole words.
    const uint64_t draws = qkdr::trial_draws((uint32_t)n);
    const uint64_t per_lane = (draws + kKeygenLanes - 1) / kKeygenLanes;
    L.keygen_chunk = (uint32_t)((per_lane + 63) / 64 * 64);
    L.jump.resize((size_t)kKeygenLevels * 256 * 4);
    qkdr::xoshiro_jump_matrices(L.keygen_chunk, kKeygenLevels, L.jump.data());
    // the same jumps as polynomials, one per lane: x^(l * chunk) mod P (the
    // default form, qkd_rng.h jump_poly_apply)
    L.jpoly.resize((size_t)kKeygenLanes * 4);
    uint64_t P[4];
    if (!qkdr::xoshiro_jump_polys(L.keygen_chunk, kKeygenLanes, L.jpoly.data()) || !qkdr::xoshiro_charpoly(P))
        return set_error(QKD_ERR_DEVICE, "xoshiro256 characteristic polynomial: unexpected degree");
    // the two-wave generator's starts (keygen_split_kernel): Alice's bits in
    // kKgSplitLanes chunks of kg_cb, the shuffle draws (from draw N) in
    // kKgSplitLanes chunks of kg_cs
    const uint32_t kl = kKgSplitLanes;
    // (a multiple of 32: a lane's chunk of Alice's bits is whole 32-bit
    // words, written by that lane alone, keygen_split_kernel)
    L.kg_cb = (uint32_t)(((n + kl - 1) / kl + 31) / 32 * 32);
    L.kg_cs = (uint32_t)((draws - (uint64_t)n + kl - 1) / kl);
    L.jpoly2.resize((size_t)2 * kl * 4);
    for (uint32_t l = 0; l < kl; ++l) {
        qkdr::poly_x_pow((uint64_t)l * L.kg_cb, P, &L.jpoly2[(size_t)l * 4]);
        qkdr::poly_x_pow((uint64_t)n + (uint64_t)l * L.kg_cs, P, &L.jpoly2[(size_t)(kl + l) * 4]);
    }
    return QKD_OK;
}

}  // namespace qkd
