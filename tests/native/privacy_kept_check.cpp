// Host build of what qkd_privacy_amplify_kept_batch shares with its kernels
// (qkd_ntt.h) and of its argument check (qkd_args.h): the reciprocal division
// against plain / and % on every p < T and at the 32-bit edges; the positions
// of a lane's four residues against (T - i) mod T taken directly, for every
// i < T with N in {1, 3, 70, 193, 10240, 131072} and T up to 2^20; the scan's
// list against a filter written the obvious way, over the flag patterns the
// GPU tests use; the gathered input against a compaction written the obvious
// way, and its hash by transforms against the direct hash of the compacted
// bytes; the scratch size; every branch of the argument checker. Prints the
// number of wrong answers ("0" when all hold). Built plain and under
// AddressSanitizer + UBSan by tests/test_privacy_kept_abi.py; a stand-alone
// program, host code only. Every array has exactly the size the headers state,
// so a read or write past one would be caught by the sanitizer.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../qkd_ldpc_amd/csrc/qkd_args.h"
#include "../../qkd_ldpc_amd/csrc/qkd_ntt.h"
#include "../../qkd_ldpc_amd/csrc/qkd_privacy.h"

static int bad = 0;

static void expect(bool ok, const char* what, long a = 0, long b = 0) {
    if (!ok) {
        if (bad < 50) fprintf(stderr, "%s (%ld, %ld)\n", what, a, b);
        bad++;
    }
}

static void expect_msg(const char* got, const char* want, const char* what) {
    const bool same = (got == nullptr && want == nullptr) || (got && want && !strcmp(got, want));
    if (!same) {
        fprintf(stderr, "%s: got '%s', want '%s'\n", what, got ? got : "(ok)", want ? want : "(ok)");
        bad++;
    }
}

int main() {
    using namespace qkdn;
    uint64_t lcg = 0x13198A2E03707344ull;
    auto next = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return lcg >> 11; };

    // ---- the division ------------------------------------------------------------
    const uint32_t frame_bits[] = {1, 3, 70, 193, 10240, 131072};
    for (uint32_t n : frame_bits) {
        const uint32_t recip = kept_reciprocal(n);
        expect(n == 1 ? recip == 0xffffffffu : recip == (uint32_t)(((uint64_t)1 << 32) / n), "reciprocal", n);
        for (uint32_t p = 0; p < (1u << 20); ++p) {
            uint32_t q, r;
            kept_divmod(p, n, recip, &q, &r);
            expect(q == p / n && r == p % n, "divmod", p, n);
        }
    }
    // ... and where the estimate is furthest off: the largest p, divisors around powers of two and the largest
    {
        const uint32_t ns[] = {1, 2, 3, 5, 7, 70, 193, 641, 10240, 65535, 65536, 65537, 131072, (1u << 27) - 1, 1u << 27,
                               (1u << 27) + 1, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xfffffffeu, 0xffffffffu};
        std::vector<uint32_t> ps = {0u, 1u, (1u << 27) - 1u, 1u << 27, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
        for (int i = 0; i < 2000; ++i) ps.push_back((uint32_t)next());
        for (uint32_t n : ns) {
            const uint32_t recip = kept_reciprocal(n);
            std::vector<uint32_t> here = ps;
            for (uint32_t m = 1; m < 40; ++m) {                    // multiples of n and their neighbours
                const uint64_t v = (uint64_t)n * (uint32_t)(next() % 4096 + m);
                if (v <= 0xffffffffull) {
                    here.push_back((uint32_t)v);
                    here.push_back((uint32_t)v - 1u);
                    if (v < 0xffffffffull) here.push_back((uint32_t)v + 1u);
                }
            }
            for (uint32_t p : here) {
                uint32_t q, r;
                kept_divmod(p, n, recip, &q, &r);
                expect(q == p / n && r == p % n, "divmod at the edges", p, n);
            }
        }
    }

    // ---- a lane's four positions ---------------------------------------------------
    for (uint32_t n : frame_bits) {
        const uint32_t recip = kept_reciprocal(n);
        for (uint32_t k : {6u, 7u, 13u, 20u}) {
            const uint32_t T = 1u << k;
            for (uint32_t g = 0; g < T / 4u; ++g) {
                uint32_t slot[4], off[4];
                kept_lane_positions(T, g, n, recip, slot, off);
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t p = (T - (4u * g + j)) & (T - 1u);
                    expect(slot[j] == p / n && off[j] == p % n, "lane position", p, n);
                }
            }
        }
    }

    // ---- the scan --------------------------------------------------------------------
    const uint8_t values[] = {1, 2, 255};
    for (uint32_t B : {1u, 2u, 3u, 9u, 33u, 64u, 65u, 511u, 512u, 513u, 2500u}) {
        for (int pattern = 0; pattern < 6; ++pattern) {
            std::vector<uint8_t> keep(B);
            for (uint32_t f = 0; f < B; ++f) {
                bool on = false;
                if (pattern == 0) on = true;
                if (pattern == 2) on = f == 0;
                if (pattern == 3) on = f == B - 1;
                if (pattern == 4) on = f & 1u;
                if (pattern == 5) on = next() % 10 != 0;
                keep[f] = on ? values[next() % 3] : 0;
            }
            std::vector<uint32_t> list(B, 12345u), want;
            for (uint32_t f = 0; f < B; ++f)
                if (keep[f] != 0) want.push_back(f);
            const uint32_t kept = kept_scan_ref(keep.data(), B, list.data());
            expect(kept == want.size(), "kept count", B, pattern);
            for (uint32_t r = 0; r < B; ++r)
                expect(list[r] == (r < want.size() ? want[r] : kKeptNone), "list entry", B, r);
        }
    }

    // ---- the gather, and the hash of what it gathers -----------------------------------
    const uint32_t shapes[][3] = {{1, 1, 1}, {70, 1, 70}, {193, 3, 64}, {7, 9, 63}, {3, 100, 64}, {333, 5, 65}};
    for (const auto& sh : shapes) {
        const uint32_t n = sh[0], B = sh[1], L = sh[2], n_in = n * B;
        const uint32_t k = transform_log2(n_in, L), T = 1u << k;
        std::vector<uint64_t> R(long_key_words(n_in, L));
        for (auto& w : R) w = (next() << 32) ^ next();
        for (int pattern = 0; pattern < 6; ++pattern) {
            std::vector<uint8_t> frames((size_t)B * n), keep(B), compact(n_in, 0);
            for (auto& v : frames) v = (uint8_t)next();
            for (uint32_t f = 0; f < B; ++f) {
                bool on = false;
                if (pattern == 0) on = true;
                if (pattern == 2) on = f == 0;
                if (pattern == 3) on = f == B - 1;
                if (pattern == 4) on = f & 1u;
                if (pattern == 5) on = next() % 10 != 0;
                keep[f] = on ? values[next() % 3] : 0;
            }
            uint32_t filled = 0;
            for (uint32_t f = 0; f < B; ++f)
                if (keep[f] != 0) {
                    memcpy(compact.data() + (size_t)filled * n, frames.data() + (size_t)f * n, n);
                    ++filled;
                }
            std::vector<uint32_t> list(B), d(T, 0xdeadbeefu);
            const uint32_t kept = kept_scan_ref(keep.data(), B, list.data());
            expect(kept == filled, "kept of the shape", n, pattern);
            kept_gather_ref(d.data(), T, frames.data(), n, B, list.data());
            for (uint32_t i = 0; i < T; ++i) {
                const uint32_t p = (T - i) & (T - 1u);
                expect(d[i] == (p < n_in ? (uint32_t)(compact[p] & 1) : 0u), "gathered residue", n, i);
            }
            // the transform's own input stage on the compacted bytes fills the same residues,
            // so the hash by transforms of either is the direct hash of the compacted bytes
            std::vector<uint32_t> work((size_t)2 << k);
            std::vector<uint64_t> got(qkdv::privacy_out_words(L), ~0ull), want(got);
            privacy_hash_ntt_ref(R.data(), compact.data(), n_in, L, got.data(), work.data());
            if (qkdv::privacy_key_words(n_in, L)) {
                qkdv::privacy_hash_ref(R.data(), compact.data(), n_in, L, want.data());
                expect(got == want, "hash of the compacted block", n, pattern);
            }
            // the prefix rule: the first L' bits are the hash of the kept frames alone at kept n bits
            const uint32_t short_in = kept * n;
            for (uint32_t Lp : {1u, short_in < L ? short_in : L}) {
                if (short_in == 0 || Lp == 0 || Lp > short_in || Lp > L) continue;
                std::vector<uint64_t> Rp(R.begin(), R.begin() + (long)long_key_words(short_in, Lp));
                std::vector<uint32_t> work_p((size_t)2 << transform_log2(short_in, Lp));
                std::vector<uint64_t> pre(qkdv::privacy_out_words(Lp), ~0ull);
                privacy_hash_ntt_ref(Rp.data(), compact.data(), short_in, Lp, pre.data(), work_p.data());
                for (uint32_t i = 0; i < Lp; ++i)
                    expect(((pre[i >> 6] >> (i & 63u)) & 1u) == ((got[i >> 6] >> (i & 63u)) & 1u), "prefix rule", n, i);
            }
        }
    }

    // ---- the scratch size ----------------------------------------------------------------
    const uint32_t big = 1u << 27, h26 = 1u << 26;
    expect(kept_scratch_bytes(10240, 33, 4096, 2) == long_scratch_bytes(10240 * 33, 4096) + 4u * 66u + 2u + 16u, "scratch");
    expect(kept_scratch_bytes(1, 1, 1, 1) == long_scratch_bytes(1, 1) + 4u + 1u + 16u, "smallest scratch");
    expect(kept_scratch_bytes(10240, 9765, 34000000u, 1) == long_scratch_bytes(99993600u, 34000000u) + 4u * 9765u + 1u + 16u,
           "the benchmark's scratch");
    expect(kept_scratch_bytes(1, h26 + 1, h26, 3) == long_scratch_bytes(h26 + 1, h26) + 4u * 3u * (size_t)(h26 + 1) + 3u + 16u,
           "the largest transform");
    expect(kept_scratch_bytes(65536, 65536, 1, 1) == 0, "B N overflows 32 bits");
    expect(kept_scratch_bytes(0x80000000u, 2, 1, 1) == 0, "B N = 2^32");
    expect(kept_scratch_bytes(0, 5, 1, 1) == 0 && kept_scratch_bytes(5, 0, 1, 1) == 0, "no bits");
    expect(kept_scratch_bytes(big, 1, 2, 1) == 0 && kept_scratch_bytes(1, big, 1, 1) != 0, "the limit");
    expect(kept_scratch_bytes(1, big + 1, 1, 1) == 0, "past the limit");
    expect(kept_scratch_bytes(7, 9, 64, 1) == 0 && kept_scratch_bytes(7, 9, 0, 1) == 0, "out_bits outside 1..B N");
    expect(kept_scratch_bytes(7, 9, 63, 0) == 0, "no block");
    if (sizeof(size_t) > 4) {
        expect(kept_scratch_bytes(7, 9, 63, (size_t)0x100000000ull) == 0, "2^32 blocks");
        expect(kept_scratch_bytes(7, 9, 63, (size_t)477218589u) == 0, "n_blocks B = 2^32 + 5");
        expect(kept_scratch_bytes(7, 9, 63, (size_t)477218588u) != 0, "n_blocks B = 2^32 - 4");
        expect(kept_scratch_bytes(7, 9, 63, ~(size_t)0) == 0 && kept_scratch_bytes(7, 9, 63, (size_t)1 << 62) == 0, "a product past 64 bits");
    }

    // ---- argument checks -----------------------------------------------------------------
    uint8_t frames[8] = {0, 1, 0, 1, 1, 1, 0, 0}, keep[2] = {1, 0};
    uint64_t out[2] = {0, 0};
    uint32_t scratch[1] = {0};
    using qkda::privacy_amplify_kept_args_error;
    const size_t sb = kept_scratch_bytes(4, 2, 8, 1), sbig = kept_scratch_bytes(h26 + 1, 1, h26, 1);
    const char* nul = "null argument";
    const char* ones = "frame_bits and frames_per_block must be >= 1";
    const char* many = "n_blocks * frames_per_block must be below 2^32";
    const char* range_n = "frame_bits * frames_per_block must be in 1..QKD_PRIVACY_LONG_MAX_BITS";
    const char* range_l = "out_bits must be in 1..frame_bits * frames_per_block";
    const char* range_t = "frame_bits * frames_per_block + out_bits - 1 exceeds QKD_PRIVACY_LONG_MAX_BITS";
    const char* short_s =
        "scratch_bytes is below qkd_privacy_kept_scratch_bytes(frame_bits, frames_per_block, out_bits, n_blocks)";
    expect(sb == long_scratch_bytes(8, 8) + 8u + 1u + 16u && sbig > ((size_t)1 << 30), "scratch sizes");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 4, 2, 8, keep, out, scratch, sb), nullptr, "valid");
    expect_msg(privacy_amplify_kept_args_error(frames, 2, 4, 1, 1, keep, out, scratch, sb + 100), nullptr, "two blocks");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, h26 + 1, 1, h26, keep, out, scratch, sbig), nullptr, "the limit");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 1, big, 1, keep, out, scratch, sbig + 4u * (size_t)big), nullptr,
               "B N at the limit");
    expect_msg(privacy_amplify_kept_args_error(nullptr, 1, 4, 2, 8, keep, out, scratch, sb), nul, "frames");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 4, 2, 8, nullptr, out, scratch, sb), nul, "keep");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 4, 2, 8, keep, nullptr, scratch, sb), nul, "out");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 4, 2, 8, keep, out, nullptr, sb), nul, "scratch");
    expect_msg(privacy_amplify_kept_args_error(nullptr, 0, 0, 0, 0, keep, out, scratch, 0), nul, "order");
    expect_msg(privacy_amplify_kept_args_error(frames, 0, 4, 2, 8, keep, out, scratch, sb), "n_blocks must be > 0", "no blocks");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 0, 2, 1, keep, out, scratch, sb), ones, "N = 0");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 4, 0, 1, keep, out, scratch, sb), ones, "B = 0");
    if (sizeof(size_t) > 4) {
        expect_msg(privacy_amplify_kept_args_error(frames, (size_t)0x100000000ull, 4, 1, 1, keep, out, scratch, sb), many, "2^32 blocks");
        expect_msg(privacy_amplify_kept_args_error(frames, (size_t)0x80000000ull, 4, 2, 8, keep, out, scratch, sb), many, "n_blocks B = 2^32");
        expect_msg(privacy_amplify_kept_args_error(frames, ~(size_t)0, 4, 2, 8, keep, out, scratch, sb), many, "a product past 64 bits");
        expect_msg(privacy_amplify_kept_args_error(frames, (size_t)0x7fffffffull, 4, 2, 8, keep, out, scratch, sb), short_s,
                   "n_blocks B = 2^32 - 2 is in range");
    }
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 65536, 65536, 1, keep, out, scratch, sbig), range_n, "B N = 2^32");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 0xffffffffu, 0xffffffffu, 1, keep, out, scratch, sbig), range_n, "B N near 2^64");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, big + 1, 1, 1, keep, out, scratch, sbig), range_n, "N past the limit");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 3, (big / 3) + 1, 1, keep, out, scratch, sbig), range_n, "B N past the limit");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 4, 2, 0, keep, out, scratch, sb), range_l, "L = 0");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 4, 2, 9, keep, out, scratch, sb), range_l, "L = B N + 1");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 4, 2, 0xffffffffu, keep, out, scratch, sb), range_l, "L = 2^32 - 1");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, h26, 2, 2, keep, out, scratch, sbig), range_t, "one past the limit");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, h26 + 1, 1, h26 + 1, keep, out, scratch, sbig), range_t, "2^27 + 1");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 4, 2, 8, keep, out, scratch, sb - 1), short_s, "one byte short");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 4, 2, 8, keep, out, scratch, 0), short_s, "no scratch bytes");
    expect_msg(privacy_amplify_kept_args_error(frames, 2, 4, 2, 8, keep, out, scratch, sb), short_s, "one block's scratch for two");
    expect_msg(privacy_amplify_kept_args_error(frames, 1, 4, 2, 8, keep, out, scratch, long_scratch_bytes(8, 8)), short_s,
               "the long form's scratch");

    printf("%d\n", bad);
    return bad ? 1 : 0;
}
