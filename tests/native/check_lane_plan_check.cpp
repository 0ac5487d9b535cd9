// Host check of the check-lane plan (qkd_plan.h build_check_lane_plan), the
// plan of the speculative check phases that run one check per lane:
//   * every edge of H appears exactly once across the check-lane part and the
//     edge-lane remainder;
//   * dead entries appear only past a check's degree, every lane's entries
//     are its own check's edges, and the check word the builder emits for the
//     lane (CheckLanePlan::chkw, the word the kernels read and the host uploads
//     as it is) unpacks, with the kernels' accessors, to the check's syndrome
//     word offset, bit and degree;
//   * pad tasks (and lanes without a check) are all dead;
//   * the split rule yields whole rounds of round_tasks tasks, the pure form
//     has no remainder;
//   * the remainder is a valid edge-lane plan (segments of whole checks, bits
//     in the check's order, check indices of H).
// Shapes: M = 48 (a single partial task), M = 1056 (one whole round plus a
// 32-check remainder), M = 1024 (an empty remainder), a bucket-6 code mixing
// degrees 4, 5 and 6, and, given its check lists on stdin (n m, the m + 1
// offsets, the indices), the N = 10240 code. Prints the number of failures.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../qkd_ldpc_amd/csrc/qkd_plan.h"

static int g_fail = 0;
#define CHECK(c, ...)                                       \
    do {                                                    \
        if (!(c)) {                                         \
            if (g_fail < 20) {                              \
                fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
                fprintf(stderr, __VA_ARGS__);               \
                fprintf(stderr, "\n");                      \
            }                                               \
            ++g_fail;                                       \
        }                                                   \
    } while (0)

struct Code {
    int32_t n = 0, m = 0;
    std::vector<int32_t> cptr, cidx, krow;
    void finish() {
        // krow[e] = position of the edge's check among its bit's checks (ascending)
        std::vector<int32_t> cnt(n, 0);
        krow.assign(cidx.size(), 0);
        for (int32_t j = 0; j < m; ++j)
            for (int32_t e = cptr[j]; e < cptr[j + 1]; ++e) krow[e] = cnt[cidx[e]]++;
    }
};

// m checks over n bits, check j of degree degs[j % degs.size()], bits spread
// by a fixed stride (ascending within the check)
static Code make_code(int32_t n, int32_t m, const std::vector<int>& degs) {
    Code c;
    c.n = n;
    c.m = m;
    c.cptr.push_back(0);
    uint64_t x = 12345;
    for (int32_t j = 0; j < m; ++j) {
        const int d = degs[j % degs.size()];
        std::vector<int32_t> bits;
        while ((int)bits.size() < d) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            const int32_t b = (int32_t)((x >> 33) % (uint64_t)n);
            bool dup = false;
            for (int32_t q : bits) dup = dup || q == b;
            if (!dup) bits.push_back(b);
        }
        std::sort(bits.begin(), bits.end());
        c.cidx.insert(c.cidx.end(), bits.begin(), bits.end());
        c.cptr.push_back((int32_t)c.cidx.size());
    }
    c.finish();
    return c;
}

static void check_plan(const char* name, const Code& c, int dc, int round_tasks, bool pure) {
    const int32_t E = c.cptr[c.m];
    qkdp::CheckLanePlan p;
    const bool ok = qkdp::build_check_lane_plan(c.n, c.m, c.cptr.data(), c.cidx.data(), c.krow.data(), dc, round_tasks,
                                                pure, p);
    CHECK(ok, "%s: build failed", name);
    if (!ok) return;
    // the split rule: whole rounds; pure: every check, no remainder
    const int32_t per_round = 64 * round_tasks;
    if (pure) {
        CHECK(p.n_tasks == (c.m + 63) / 64, "%s: pure tasks %d", name, p.n_tasks);
        CHECK(p.rem_checks.empty() && p.rem.n_tasks == 0, "%s: pure form with a remainder", name);
    } else {
        CHECK(p.n_tasks % round_tasks == 0, "%s: %d tasks are not whole rounds of %d", name, p.n_tasks, round_tasks);
        CHECK(p.n_tasks == (c.m / per_round) * round_tasks, "%s: tasks %d", name, p.n_tasks);
        CHECK((int32_t)p.rem_checks.size() == c.m - p.n_tasks * 64, "%s: remainder of %zu checks", name,
              p.rem_checks.size());
        CHECK((int32_t)p.rem_checks.size() < per_round, "%s: remainder holds a whole round", name);
    }
    CHECK(p.dc == dc, "%s: dc", name);
    const size_t tasks_pad = (size_t)p.n_tasks + qkdp::kPlanPadTasks;
    CHECK(p.edge.size() == tasks_pad * dc * 64 && p.chk.size() == tasks_pad * 64 && p.chkw.size() == p.chk.size(),
          "%s: array sizes", name);
    if (p.edge.size() != tasks_pad * dc * 64 || p.chk.size() != tasks_pad * 64 || p.chkw.size() != p.chk.size()) return;
    std::vector<int> seen(E, 0);
    std::vector<int> chk_seen(c.m, 0);
    for (size_t t = 0; t < tasks_pad; ++t) {
        for (int l = 0; l < 64; ++l) {
            const int32_t j = p.chk[t * 64 + l];
            if (t >= (size_t)p.n_tasks) CHECK(j == -1, "%s: pad task %zu lane %d holds check %d", name, t, l, j);
            CHECK(j >= -1 && j < c.m, "%s: check %d out of range", name, j);
            if (j < -1 || j >= c.m) continue;
            const int32_t d = j < 0 ? 0 : c.cptr[j + 1] - c.cptr[j];
            // the word the builder emitted for this lane, read as the kernels
            // read it: byte offset of the 32-bit syndrome word holding check
            // j's bit, the bit's position in it, the degree (0: no check)
            const uint32_t w = p.chkw[t * 64 + l];
            if (j >= 0) {
                chk_seen[j]++;
                CHECK(qkdp::chk_word_addr(w) % 4u == 0 && qkdp::chk_word_addr(w) * 8u + qkdp::chk_word_bit(w) == (uint32_t)j,
                      "%s: check word %08x of check %d addresses bit %u", name, w, j,
                      qkdp::chk_word_addr(w) * 8u + qkdp::chk_word_bit(w));
                CHECK(qkdp::chk_word_deg(w) == (uint32_t)d, "%s: check word %08x of check %d: degree %u, not %d", name, w,
                      j, qkdp::chk_word_deg(w), d);
            } else {
                CHECK(w == 0u, "%s: task %zu lane %d without a check has word %08x", name, t, l, w);
            }
            for (int k = 0; k < dc; ++k) {
                const int32_t e = p.edge[(t * dc + k) * 64 + l];
                if (k >= d) {
                    CHECK(e == -1, "%s: task %zu lane %d entry %d past degree %d is live", name, t, l, k, d);
                    continue;
                }
                // dead entries only past the degree; a live one is an edge of the lane's check
                CHECK(e >= c.cptr[j] && e < c.cptr[j + 1], "%s: task %zu lane %d entry %d: edge %d not of check %d",
                      name, t, l, k, e, j);
                if (e >= 0 && e < E) seen[e]++;
            }
        }
    }
    // the remainder: an edge-lane plan of whole checks with H's check indices
    const qkdp::WavePlan& r = p.rem;
    CHECK(r.word.size() == (size_t)(r.n_tasks + qkdp::kPlanPadTasks) * 64 && r.seg.size() == r.word.size() &&
              r.chk.size() == r.word.size() && (int32_t)r.slot_of_edge.size() == E,
          "%s: remainder sizes", name);
    std::vector<int> in_rem(c.m, 0);
    for (int32_t j : p.rem_checks) in_rem[j] = 1;
    for (size_t s = 0; s < r.word.size(); ++s) {
        const int32_t j = r.chk[s];
        const uint32_t bit = r.word[s] & qkdp::kPlanBitMask;
        if (j < 0) {
            CHECK(bit == (uint32_t)c.n, "%s: idle remainder lane with bit %u", name, bit);
            continue;
        }
        CHECK(s < (size_t)r.n_tasks * 64, "%s: remainder pad task holds check %d", name, j);
        CHECK(j < c.m && in_rem[j], "%s: remainder lane of check %d, not in the remainder", name, j);
        if (j >= c.m) continue;
        const uint32_t start = (r.seg[s] >> 20) & 63u, deg = (r.seg[s] >> 26) + 1;
        const int32_t k = (int32_t)(s & 63) - (int32_t)start;
        if (k == 0) chk_seen[j]++;
        CHECK((r.seg[s] & qkdp::kPlanChkMask) == (uint32_t)j, "%s: remainder segment word names check %u, not %d",
              name, r.seg[s] & qkdp::kPlanChkMask, j);
        CHECK((int32_t)deg == c.cptr[j + 1] - c.cptr[j] && k >= 0 && k < (int32_t)deg, "%s: remainder segment of %d",
              name, j);
        if (k < 0 || k >= (int32_t)deg) continue;
        const int32_t e = c.cptr[j] + k;
        CHECK(bit == (uint32_t)c.cidx[e] && (r.word[s] >> 24) == (uint32_t)c.krow[e], "%s: remainder edge %d", name, e);
        CHECK(r.slot_of_edge[e] == (int32_t)s, "%s: slot_of_edge[%d]", name, e);
        seen[e]++;
    }
    for (int32_t e = 0; e < E; ++e) CHECK(seen[e] == 1, "%s: edge %d appears %d times", name, e, seen[e]);
    for (int32_t j = 0; j < c.m; ++j) CHECK(chk_seen[j] == 1, "%s: check %d appears %d times", name, j, chk_seen[j]);
    for (int32_t e = 0; e < E; ++e) {
        bool rem_edge = false;
        for (int32_t j : p.rem_checks) rem_edge = rem_edge || (e >= c.cptr[j] && e < c.cptr[j + 1]);
        if (!rem_edge) CHECK(r.slot_of_edge[e] == -1, "%s: slot_of_edge[%d] of a check-lane edge", name, e);
        if (p.rem_checks.size() > 4096) break;      // (quadratic: small remainders only)
    }
}

static void check_all(const char* name, const Code& c, int dc) {
    for (int pure = 0; pure < 2; ++pure) check_plan(name, c, dc, 16, pure != 0);
}

int main(int argc, char** argv) {
    check_all("m48", make_code(200, 48, {6}), 6);
    check_all("m1056", make_code(2112, 1056, {6, 5}), 6);
    check_all("m1024", make_code(2048, 1024, {4}), 4);
    check_all("mixed456", make_code(3000, 1500, {4, 5, 6, 6, 5}), 6);
    check_all("deg8", make_code(700, 300, {8, 7, 3}), 8);
    // a degree past the bucket is refused
    {
        const Code c = make_code(100, 10, {7});
        qkdp::CheckLanePlan p;
        CHECK(!qkdp::build_check_lane_plan(c.n, c.m, c.cptr.data(), c.cidx.data(), c.krow.data(), 6, 16, false, p),
              "degree 7 accepted in bucket 6");
    }
    if (argc > 1) {
        // the golden code from stdin
        Code c;
        if (scanf("%d %d", &c.n, &c.m) != 2) return 2;
        c.cptr.resize(c.m + 1);
        for (int32_t j = 0; j <= c.m; ++j)
            if (scanf("%d", &c.cptr[j]) != 1) return 2;
        c.cidx.resize(c.cptr[c.m]);
        for (size_t e = 0; e < c.cidx.size(); ++e)
            if (scanf("%d", &c.cidx[e]) != 1) return 2;
        c.finish();
        check_all("golden", c, 6);
        qkdp::CheckLanePlan p;
        qkdp::build_check_lane_plan(c.n, c.m, c.cptr.data(), c.cidx.data(), c.krow.data(), 6, 16, false, p);
        fprintf(stderr, "golden: %d check-lane tasks, %zu remainder checks in %d tasks\n", p.n_tasks,
                p.rem_checks.size(), p.rem.n_tasks);
    }
    printf("%d\n", g_fail);
    return g_fail ? 1 : 0;
}
