// keygen.hip — the trial key pairs: Alice's random key and Bob's copy with
// exactly round(q N) errors, bit for bit the reference's
// generate_random_bit_array + introduce_errors
// (src/array_and_matrix_operations.cpp:424-460) on xoshiro256++ (qkd_rng.h).
//
// Three generators of the same pair (keygen_kernel: a thread per frame;
// keygen_fast_kernel: jump-ahead lanes; keygen_split_kernel: two waves, the
// default), chosen by keygen_into_ws, and the interactive mode's one stream
// across QBER points (keygen_stream_kernel, src/simulation.cpp:73-137).
#include <hip/hip_runtime.h>

#include "qkd_decode.h"
#include "qkd_host.h"
#include "qkd_rng.h"

namespace qkd {

// ---- key generation: one thread per frame ------------------------------------
// generate_random_bit_array + introduce_errors (array_and_matrix_operations.cpp:424-460)
__global__ void keygen_kernel(const uint64_t* seeds, uint64_t offset, uint32_t n_frames, uint32_t n,
                              uint32_t words, uint32_t ne, uint64_t* alice_w, uint64_t* bob_w,
                              uint32_t* low_scratch, double* exact_q) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frames) return;
    qkdr::Xoshiro256pp g;
    g.seed(seeds[f] + offset);
    uint64_t* A = alice_w + (size_t)f * words;
    uint64_t* B = bob_w + (size_t)f * words;
    for (uint32_t w = 0; w < words; ++w) {
        const uint32_t nb = min(64u, n - w * 64);
        uint64_t v = 0;
        for (uint32_t b = 0; b < nb; ++b) v |= (g.next() >> 63) << b;
        A[w] = v;
        B[w] = v;
    }
    uint32_t* low = low_scratch + (size_t)f * ne;
    qkdr::shuffle_low_positions(g, n, ne, low);
    for (uint32_t p = 0; p < ne; ++p) {
        const uint32_t pos = low[p];
        B[pos >> 6] ^= 1ull << (pos & 63);
    }
    if (exact_q) exact_q[f] = (double)ne / (double)n;
}

// ---- key generation: kKeygenLanes lanes per frame (jump-ahead) ---------------
// Same key pair as keygen_kernel, drawn in parallel; kKeygenFrames frames per
// workgroup, each on its own kKeygenLanes-lane slice of it. The
// trial's draw stream (qkdr::trial_draws) is cut into kKeygenLanes chunks of
// `chunk` draws; lane l of a frame jumps the seeded state by l * chunk draws
// (jump[b] = T^(chunk * 2^b), applied for the set bits of l: a jump is a
// 256x256 GF(2) product per level and lane, so fewer lanes per frame mean fewer
// levels and less work per frame) and then steps through its chunk:
//   draws [0, N)      Alice's bits (whole words per lane: chunk % 64 == 0)
//   draw N (even N)   the lone swap of std::shuffle
//   the rest          one Lemire draw per shuffle pair (i, i+1)
// Shuffle steps with index < ne need the exact swap sequence: their draws are
// parked in LDS and replayed by the frame's lane 0 (qkdr::shuffle_low_positions,
// steps i < ne). Steps >= ne only ever write "low[x] = i", so the last such
// writer of each low position is found with an LDS atomicMax. A Lemire rejection
// (probability ~ range / 2^64 per draw) shifts every later draw: such a frame
// is regenerated serially by its lane 0 from its seed.
// R32 (N <= 65536): every pair's range (i + 1)(i + 2) < 2^32, so the Lemire
// products are 64 x 32 bits and the pair split x / (i + 2) a binary32
// reciprocal product with one exact integer correction (the lanes of a frame
// diverge between Alice's bits and the shuffle draws, so the wave pays both
// paths on every draw: the binary64 division was most of it).
template <bool R32>
__global__ __launch_bounds__(kKeygenBlock) void keygen_fast_kernel(const uint64_t* seeds, uint64_t offset, uint32_t n,
                                                         uint32_t words, uint32_t ne, uint32_t chunk,
                                                         uint32_t n_frames, const uint64_t* __restrict__ jump,
                                                         const uint64_t* __restrict__ jpoly,
                                                         uint64_t* alice_w, uint64_t* bob_w, double* exact_q,
                                                         uint32_t force_serial) {
    extern __shared__ uint32_t kg_lds[];
    __shared__ uint32_t s_lone[kKeygenFrames], s_reject[kKeygenFrames];
    const uint32_t slot = threadIdx.x / kKeygenLanes;          // this frame's slice of the workgroup
    const uint32_t lane = threadIdx.x % kKeygenLanes;
    // per frame (an even number of words, so every park is 8-byte aligned):
    // low[ne], last[ne], park[ne / 2 + 1]
    const uint32_t frame_words = 2 * ne + 2 * (ne / 2 + 1);
    uint32_t* low = kg_lds + (size_t)slot * frame_words;     // ne: replayed positions
    uint32_t* last = low + ne;                               // ne: last step >= ne writing here (0 = none)
    uint2* park = (uint2*)(last + ne);                       // ne / 2 + 1 parked pair draws

    const uint32_t f = blockIdx.x * kKeygenFrames + slot;
    const bool live = f < n_frames;                          // (the last workgroup may hold fewer frames)
    const bool even = (n & 1u) == 0;
    const uint64_t pair0 = even ? (uint64_t)n + 1 : (uint64_t)n;  // draw index of the first pair
    const uint32_t i0 = even ? 2u : 1u;                             // its step index
    const uint64_t draws = qkdr::trial_draws(n);

    qkdr::Xoshiro256pp g;
    g.seed(live ? seeds[f] + offset : 0);
    uint64_t st[4] = {g.s0, g.s1, g.s2, g.s3};
    if (jpoly) {
        // the lane's jump as a polynomial in T (qkd_rng.h jump_poly_apply):
        // 256 state steps, no matrix reads
        const uint64_t p[4] = {jpoly[lane * 4 + 0], jpoly[lane * 4 + 1], jpoly[lane * 4 + 2], jpoly[lane * 4 + 3]};
        qkdr::jump_poly_apply(p, st);
    } else {
        for (int b = 0; b < kKeygenLevels; ++b) {
            uint64_t t[4] = {st[0], st[1], st[2], st[3]};
            qkdr::jump_apply(jump + (size_t)b * 1024, t);
            if ((lane >> b) & 1u) {
                st[0] = t[0]; st[1] = t[1]; st[2] = t[2]; st[3] = t[3];
            }
        }
    }
    g.s0 = st[0]; g.s1 = st[1]; g.s2 = st[2]; g.s3 = st[3];

    for (uint32_t p = lane; p < ne; p += kKeygenLanes) {
        low[p] = p;
        last[p] = 0;
    }
    if (lane == 0) {
        s_lone[slot] = 0;
        s_reject[slot] = force_serial;
    }
    __syncthreads();

    uint64_t* A = alice_w + (size_t)f * words;
    uint64_t* B = bob_w + (size_t)f * words;
    const uint64_t first = (uint64_t)lane * chunk;
    const uint64_t end = live ? min(first + chunk, draws) : first;
    uint64_t acc = 0;
    for (uint64_t d = first; d < end; ++d) {
        const uint64_t r = g.next();
        if (d < n) {
            acc |= (r >> 63) << (d & 63);
            if ((d & 63) == 63 || d + 1 == n) {
                A[d >> 6] = acc;
                B[d >> 6] = acc;
                acc = 0;
            }
        } else if (d < pair0) {
            s_lone[slot] = (uint32_t)(r >> 63);
        } else {
            const uint32_t i = i0 + 2u * (uint32_t)(d - pair0);
            const uint64_t b1 = (uint64_t)i + 2;
            const uint64_t range = ((uint64_t)i + 1) * b1;
            uint32_t qa, qb;
            if constexpr (R32) {
                // r * range = p1 * 2^32 + p0 with range < 2^32: the low 64 bits
                // (Lemire's test) and the high ones (x < range < 2^32)
                const uint32_t rg = (uint32_t)range, bb = (uint32_t)b1;
                const uint64_t p0 = (uint64_t)(uint32_t)r * rg;
                const uint64_t p1 = (uint64_t)(uint32_t)(r >> 32) * rg;
                const uint64_t lo = p0 + (p1 << 32);
                if (lo < range) {
                    if (lo < (0 - range) % range) s_reject[slot] = 1;
                }
                const uint32_t x = (uint32_t)((p1 + (p0 >> 32)) >> 32);
                // x / bb < 2^16 to 2^-21 relative: off by at most one
                uint32_t q = (uint32_t)((float)x * __builtin_amdgcn_rcpf((float)bb));
                int32_t rem = (int32_t)(x - q * bb);
                if (rem < 0) { --q; rem += (int32_t)bb; }
                else if (rem >= (int32_t)bb) { ++q; rem -= (int32_t)bb; }
                qa = q;
                qb = (uint32_t)rem;
            } else {
                const uint64_t lo = r * range;
                if (lo < range && lo < (0 - range) % range) s_reject[slot] = 1;
                const uint64_t x = qkdr::mul_hi64(r, range);
                // quotient through binary64, corrected to the exact integer one
                uint64_t a = (uint64_t)((double)x / (double)b1);
                if (a * b1 > x) --a;
                else if (x - a * b1 >= b1) ++a;
                qa = (uint32_t)a;
                qb = (uint32_t)(x - a * b1);
            }
            if (i < ne) {
                park[(i - i0) >> 1] = make_uint2(qa, qb);
            } else {
                if (qa < ne) atomicMax(&last[qa], i);
                if (qb < ne) atomicMax(&last[qb], i + 1);
            }
        }
    }
    __syncthreads();

    if (live && s_reject[slot]) {
        // exact serial regeneration of this frame (never observed in practice)
        if (lane == 0) {
            qkdr::Xoshiro256pp h;
            h.seed(seeds[f] + offset);
            for (uint32_t w = 0; w < words; ++w) {
                const uint32_t nb = min(64u, n - w * 64);
                uint64_t v = 0;
                for (uint32_t b = 0; b < nb; ++b) v |= (h.next() >> 63) << b;
                A[w] = v;
                B[w] = v;
            }
            qkdr::shuffle_low_positions(h, n, ne, low);
            for (uint32_t p = 0; p < ne; ++p) B[low[p] >> 6] ^= 1ull << (low[p] & 63);
            if (exact_q) exact_q[f] = (double)ne / (double)n;
        }
    } else if (live && lane == 0) {
        // replay of the steps with index < ne (shuffle_low_positions' step())
        auto step = [&](uint32_t si, uint32_t x) {
            if (si < ne) {
                const uint32_t v = low[x];
                low[x] = si;
                low[si] = v;
            } else if (x < ne) {
                low[x] = si;
            }
        };
        if (n > 1) {
            if (even) step(1, s_lone[slot]);
            for (uint32_t i = i0; i < ne && i < n; i += 2) {
                const uint2 q = park[(i - i0) >> 1];
                step(i, q.x);
                step(i + 1, q.y);
            }
        }
        if (exact_q) exact_q[f] = (double)ne / (double)n;
    }
    __syncthreads();
    if (live && !s_reject[slot]) {
        for (uint32_t p = lane; p < ne; p += kKeygenLanes) {
            const uint32_t pos = last[p] ? last[p] : low[p];
            atomicXor((unsigned long long*)&B[pos >> 6], 1ull << (pos & 63));
        }
    }
}

// The error positions without replaying the shuffle (keygen_split_kernel).
// Step s of the forward shuffle (introduce_errors, qkd_ldpc_algorithm.cpp)
// swaps a[s] with a[x_s], x_s <= s, and a[s] is still s when it does (earlier
// steps touch only lower indices), so afterwards a[x_s] = s. Hence a[q]
// (q < ne) is the last step s with x_s = q (last[q], an LDS atomicMax over
// all steps) when there is one; otherwise the last step to touch q is step q
// itself, which left there the value position x_q held just before it: the
// last step s in [x_q, q) with x_s = x_q, or failing that (recursively) the
// value x_q received from its own step. Position 0 is no step's index (its
// value is 0 until a step writes it). Such positions (no later writer) are
// ~q/N of them, ~2 per config-2 frame: the whole wave resolves each in turn,
// scanning 64 steps per ballot. Every argument is wave-uniform.
template <class XS>
__device__ __forceinline__ uint32_t kg_resolve_wave(uint32_t q, const XS& xs, uint32_t lane) {
    uint32_t t = q, p = xs(q);
    for (;;) {
        const int lo = p > 1u ? (int)p : 1;
        for (int base = (int)t - 1; base >= lo; base -= 64) {
            const int st = base - (int)lane;
            const bool hit = st >= lo && xs((uint32_t)st) == p;
            const uint64_t hb = __ballot(hit);
            if (hb) return (uint32_t)(base - (__ffsll((unsigned long long)hb) - 1));
        }
        if (p == 0) return 0;
        t = p;
        p = xs(p);
    }
}

// The same key pair by two waves per workgroup (the default generator): in the
// one-wave form every lane's chunk mixes Alice's bits and shuffle draws, so
// the wave runs both loop bodies on every draw. Here wave 0 draws only Alice's
// bits (a frame's lane l: draws [l * cb, (l + 1) * cb), cb a multiple of 32,
// written as whole 32-bit LDS words) and wave 1 only the shuffle's
// (lane l: from draw N + l * cs): each lane jumps once (its own polynomial,
// c->d_jpoly2), every loop is uniform. A frame takes kKgSplitLanes lanes of
// each wave, so a workgroup holds kKgSplitFrames frames: fewer lanes per
// frame mean longer chunks but fewer 256-step jumps per frame. Every step's
// swap partner below ne goes into last[] (LDS atomicMax), the low steps'
// partners also into park[]; the error positions then follow without a serial
// replay (kg_resolve_wave). The flips land in a mask beside Alice's words,
// and both keys leave as whole coalesced words (Bob's as Alice ^ mask).
// LDS per frame: low[ne] (the serial path's), last[ne], park[ne / 2 + 1],
// alice[words], flips[words].
template <bool R32>
__global__ __launch_bounds__(kKgBlock) void keygen_split_kernel(const uint64_t* seeds, uint64_t offset, uint32_t n,
                                                           uint32_t words, uint32_t ne, uint32_t cb, uint32_t cs,
                                                           uint32_t n_frames, const uint64_t* __restrict__ jpoly,
                                                           uint64_t* alice_w, uint64_t* bob_w, double* exact_q,
                                                           uint32_t force_serial) {
    constexpr uint32_t KL = kKgSplitLanes, FPW = kKgSplitFrames;
    extern __shared__ uint64_t ks_lds[];
    __shared__ uint32_t s_lone[FPW], s_reject[FPW];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    // (the wave index through readfirstlane: the compiler then knows it, and a
    // frame's seed, wave-uniform, so the jumps' state steps stay scalar)
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const bool shuffle_wave = (wv & 1u) != 0;
    const uint32_t slot = (wv >> 1) * (64 / KL) + lane / KL;   // this lane's frame in the workgroup
    const uint32_t l = lane % KL;                               // and its lane in that frame
    // (per frame an even number of 32-bit words before the key words)
    const uint32_t frame_u64 = (2 * ne + 2 * (ne / 2 + 1)) / 2 + 2 * words;
    auto frame_lds = [&](uint32_t sl) { return ks_lds + (size_t)sl * frame_u64; };
    uint32_t* low = reinterpret_cast<uint32_t*>(frame_lds(slot));
    uint32_t* last = low + ne;
    uint2* park = reinterpret_cast<uint2*>(last + ne);
    uint64_t* aw = reinterpret_cast<uint64_t*>(park + ne / 2 + 1);
    const uint32_t f = blockIdx.x * FPW + slot;
    const bool live = f < n_frames;                             // (the last workgroup may hold fewer)
    const bool even = (n & 1u) == 0;
    const uint64_t pair0 = even ? (uint64_t)n + 1 : (uint64_t)n;
    const uint32_t i0 = even ? 2u : 1u;
    const uint64_t draws = qkdr::trial_draws(n);

    qkdr::Xoshiro256pp g;
    g.seed(live ? seeds[f] + offset : 0);
    {
        uint64_t st[4] = {g.s0, g.s1, g.s2, g.s3};
        const uint32_t pi = (shuffle_wave ? KL : 0u) + l;
        const uint64_t p[4] = {jpoly[pi * 4 + 0], jpoly[pi * 4 + 1], jpoly[pi * 4 + 2], jpoly[pi * 4 + 3]};
        qkdr::jump_poly_apply(p, st);
        g.s0 = st[0]; g.s1 = st[1]; g.s2 = st[2]; g.s3 = st[3];
    }
    for (uint32_t sl = 0; sl < FPW; ++sl) {
        uint32_t* lo = reinterpret_cast<uint32_t*>(frame_lds(sl));
        uint64_t* a = reinterpret_cast<uint64_t*>(reinterpret_cast<uint2*>(lo + 2 * ne) + ne / 2 + 1);
        for (uint32_t q = tid; q < ne; q += kKgBlock) lo[ne + q] = 0;
        for (uint32_t w = tid; w < 2 * words; w += kKgBlock) a[w] = 0;   // Alice's words, then the flip mask
    }
    if (tid < FPW) {
        s_lone[tid] = 0;
        s_reject[tid] = force_serial;
    }
    __syncthreads();

    if (!shuffle_wave) {
        // Alice's bits: cb is a multiple of 32 (qkd_layout.h), so a lane's chunk
        // is whole 32-bit words of the key, written by that lane alone. A
        // block of 32 draws shifts each draw's top bit into a register from
        // the right (one v_alignbit_b32) and reverses it at the end, so draw
        // d lands on bit d & 31.
        const uint32_t first = l * cb;
        const uint32_t end = live ? min(first + cb, n) : first;
        uint32_t* aw32 = reinterpret_cast<uint32_t*>(aw);
        for (uint32_t d = first; d < end; d += 32) {
            uint32_t acc = 0;
            const uint32_t cnt = min(32u, end - d);
            if (cnt == 32) {
#pragma unroll 8
                for (int k = 0; k < 32; ++k)
                    acc = __builtin_amdgcn_alignbit(acc, (uint32_t)(g.next_fast() >> 32), 31);
                aw32[d >> 5] = __builtin_bitreverse32(acc);
            } else {
                for (uint32_t k = 0; k < cnt; ++k)
                    acc = __builtin_amdgcn_alignbit(acc, (uint32_t)(g.next_fast() >> 32), 31);
                aw32[d >> 5] = __builtin_bitreverse32(acc) >> (32 - cnt);
            }
        }
    } else if constexpr (R32) {
        // The shuffle's pair draws, N <= 65536: every range (i + 1)(i + 2) <
        // 2^32 (kept up to date by one add per draw). Lemire's product r *
        // range in 32-bit pieces: x = its high 64 bits is A_hi + carry(A_lo +
        // B_hi) for A = r_hi * range, B = r_lo * range; its low 64 bits are
        // below range (the rejection test, probability ~2^-32) only if A_lo +
        // B_hi wraps to 0, and only then is B_lo needed. The pair split x /
        // (i + 2) as a binary32 reciprocal product with one exact correction
        // (checked on the host for every divisor), its remainder by a 24-bit
        // multiply (q, i + 2 < 2^17).
        uint64_t d = (uint64_t)n + (uint64_t)l * cs;
        const uint64_t end = live ? min(d + cs, draws) : d;
        if (d < end && d < pair0) {                      // the lone draw (even N): lane 0
            const uint32_t x = (uint32_t)(g.next_fast() >> 63);
            s_lone[slot] = x;
            if (x < ne) atomicMax(&last[x], 1u);
            ++d;
        }
        uint32_t i = i0 + 2u * (uint32_t)(d - pair0);
        uint32_t rg = (i + 1u) * (i + 2u);
        for (; d < end; ++d) {
            const uint64_t r = g.next_fast();
            const uint32_t rl = (uint32_t)r, rh = (uint32_t)(r >> 32);
            const uint32_t alo = rh * rg, ahi = __umulhi(rh, rg), bhi = __umulhi(rl, rg);
            const uint32_t t = alo + bhi;
            const uint32_t x = ahi + (t < alo ? 1u : 0u);
            if (t == 0u) {
                const uint32_t blo = rl * rg;
                if (blo < rg && (uint64_t)blo < (0ull - (uint64_t)rg) % (uint64_t)rg) s_reject[slot] = 1;
            }
            const uint32_t bb = i + 2u;
            const uint32_t q0 = (uint32_t)((float)x * __builtin_amdgcn_rcpf((float)bb));
            const int32_t r0 = (int32_t)(x - __umul24(q0, bb));
            // (the correction as selects, no divergent branch)
            const bool lo = r0 < 0, hi = r0 >= (int32_t)bb;
            const uint32_t q = q0 + (hi ? 1u : 0u) - (lo ? 1u : 0u);
            const int32_t rem = r0 + (lo ? (int32_t)bb : 0) - (hi ? (int32_t)bb : 0);
            if (i < ne) park[(i - i0) >> 1] = make_uint2(q, (uint32_t)rem);
            if (q < ne) atomicMax(&last[q], i);
            if ((uint32_t)rem < ne) atomicMax(&last[rem], i + 1);
            rg += 4u * i + 10u;                          // (i + 3)(i + 4)
            i += 2u;
        }
    } else {
        const uint64_t first = (uint64_t)n + (uint64_t)l * cs;
        const uint64_t end = live ? min(first + cs, draws) : first;
        for (uint64_t d = first; d < end; ++d) {
            const uint64_t r = g.next();
            if (d < pair0) {
                const uint32_t x = (uint32_t)(r >> 63);
                s_lone[slot] = x;
                if (x < ne) atomicMax(&last[x], 1u);
                continue;
            }
            const uint32_t i = i0 + 2u * (uint32_t)(d - pair0);
            const uint64_t b1 = (uint64_t)i + 2;
            const uint64_t range = ((uint64_t)i + 1) * b1;
            uint32_t qa, qb;
            {
                const uint64_t lo = r * range;
                if (lo < range && lo < (0 - range) % range) s_reject[slot] = 1;
                const uint64_t x = qkdr::mul_hi64(r, range);
                uint64_t a = (uint64_t)((double)x / (double)b1);
                if (a * b1 > x) --a;
                else if (x - a * b1 >= b1) ++a;
                qa = (uint32_t)a;
                qb = (uint32_t)(x - a * b1);
            }
            if (i < ne) park[(i - i0) >> 1] = make_uint2(qa, qb);
            if (qa < ne) atomicMax(&last[qa], i);
            if (qb < ne) atomicMax(&last[qb], i + 1);
        }
    }
    __syncthreads();

    uint64_t* A = alice_w + (size_t)f * words;
    uint64_t* B = bob_w + (size_t)f * words;
    const bool rej = live && s_reject[slot];
    if (rej && !shuffle_wave && l == 0) {
        // exact serial regeneration of this frame (never observed in practice)
        qkdr::Xoshiro256pp h;
        h.seed(seeds[f] + offset);
        for (uint32_t w = 0; w < words; ++w) {
            const uint32_t nb = min(64u, n - w * 64);
            uint64_t v = 0;
            for (uint32_t b = 0; b < nb; ++b) v |= (h.next() >> 63) << b;
            A[w] = v;
            B[w] = v;
        }
        qkdr::shuffle_low_positions(h, n, ne, low);
        for (uint32_t q = 0; q < ne; ++q) B[low[q] >> 6] ^= 1ull << (low[q] & 63);
        if (exact_q) exact_q[f] = (double)ne / (double)n;
    }
    if (live && !rej && shuffle_wave && l == 0 && exact_q) exact_q[f] = (double)ne / (double)n;
    // (the rest per frame slot, all kKgBlock threads; a rejected frame is done):
    // the flips into a mask beside Alice's words, Bob's key = Alice's ^ mask
    for (uint32_t sl = 0; sl < FPW; ++sl) {
        const uint32_t fs = blockIdx.x * FPW + sl;
        if (fs >= n_frames || s_reject[sl]) continue;                // (workgroup-uniform)
        uint32_t* lo = reinterpret_cast<uint32_t*>(frame_lds(sl));
        const uint2* pk = reinterpret_cast<const uint2*>(lo + 2 * ne);
        uint64_t* b = reinterpret_cast<uint64_t*>(reinterpret_cast<uint2*>(lo + 2 * ne) + ne / 2 + 1) + words;
        // x_s: the position step s (1 <= s < ne) swaps with
        auto xs = [&](uint32_t st) -> uint32_t {
            if (even && st == 1) return s_lone[sl];
            const uint2 pr = pk[(st - i0) >> 1];
            return ((st - i0) & 1u) ? pr.y : pr.x;
        };
        for (uint32_t q0 = 0; q0 < ne; q0 += kKgBlock) {       // (uniform trip count: the scans use every lane)
            const uint32_t q = q0 + tid;
            uint32_t pos = q < ne ? lo[ne + q] : 1u;
            uint64_t rare = __ballot(pos == 0 && q > 0);
            while (rare) {
                const uint32_t src = (uint32_t)(__ffsll((unsigned long long)rare) - 1);
                rare &= rare - 1;
                const uint32_t r = kg_resolve_wave(q0 + (tid & ~63u) + src, xs, lane);
                if (lane == src) pos = r;
            }
            if (q < ne) atomicXor(reinterpret_cast<unsigned long long*>(&b[pos >> 6]), 1ull << (pos & 63u));
        }
    }
    __syncthreads();
    for (uint32_t sl = 0; sl < FPW; ++sl) {
        const uint32_t fs = blockIdx.x * FPW + sl;
        if (fs >= n_frames || s_reject[sl]) continue;
        const uint64_t* a = reinterpret_cast<const uint64_t*>(reinterpret_cast<const uint2*>(
                                reinterpret_cast<const uint32_t*>(frame_lds(sl)) + 2 * ne) + ne / 2 + 1);
        for (uint32_t w = tid; w < words; w += kKgBlock) {
            alice_w[(size_t)fs * words + w] = a[w];
            bob_w[(size_t)fs * words + w] = a[w] ^ a[words + w];
        }
    }
}

qkd_status keygen_into_ws(const qkd_code* c, qkd_workspace* ws, const uint64_t* seeds,
                          uint64_t offset, size_t n_frames, double q_nom, double* exact_q,
                          hipStream_t stream) {
    if (!(q_nom > 0.0 && q_nom <= 1.0)) return set_error(QKD_ERR_INVALID_ARG, "QBER must be in (0,1]");
    const uint64_t ne = qkdr::num_errors((uint32_t)c->n, q_nom);
    if (ne == 0)
        return set_error(QKD_ERR_QBER_TOO_SMALL, "Key size '%d' is too small for QBER.", c->n);
    qkd_status s = ws_reserve_keys(ws, n_frames, n_frames * ne);
    if (s != QKD_OK) return s;
    const uint32_t words = (uint32_t)((c->n + 63) / 64);
    // QKD_KEYGEN=serial forces the one-thread-per-frame kernel, QKD_KEYGEN=replay
    // the two-wave kernel's serial path for every frame, QKD_KEYGEN=lanes the
    // one-wave kernel (keygen_fast_kernel), QKD_KEYGEN=matrix that kernel with its
    // lane jumps as GF(2) matrix products instead of polynomials (tests of all).
    const DbgOpt mode = debug_option(ws, "QKD_KEYGEN");
    const bool serial = mode.is("serial");
    const uint32_t replay = mode.is("replay") ? 1u : 0u;
    const bool matrix = mode.is("matrix");
    const bool lanes = mode.is("lanes");
    // the two-wave generator (default; QKD_KEYGEN=replay forces its serial path)
    const size_t lds2 = (size_t)kKgSplitFrames * ((2 * (size_t)ne + 2 * (ne / 2 + 1)) * sizeof(uint32_t) +
                                                  2 * (size_t)words * sizeof(uint64_t));
    if (ne <= kKeygenFastMaxErrors && c->d_jpoly2 && !serial && !matrix && !lanes && lds2 <= kLdsBytesMax) {
        auto* const kg = c->n <= 65536 ? keygen_split_kernel<true> : keygen_split_kernel<false>;
        hipLaunchKernelGGL(kg, dim3((unsigned)((n_frames + kKgSplitFrames - 1) / kKgSplitFrames)), dim3(kKgBlock), lds2,
                           stream, seeds, offset, (uint32_t)c->n, words, (uint32_t)ne, c->kg_cb, c->kg_cs,
                           (uint32_t)n_frames, c->d_jpoly2, ws->alice_w, ws->bob_w, exact_q, replay);
        QKD_HIP(hipGetLastError());
        return QKD_OK;
    }
    // (the fast kernel's per-frame LDS times kKeygenFrames must fit a workgroup's LDS)
    const size_t lds = (size_t)kKeygenFrames * (2 * (size_t)ne * sizeof(uint32_t) + (ne / 2 + 1) * sizeof(uint2));
    if (ne <= kKeygenFastMaxErrors && c->d_jump && !serial && lds <= kLdsBytesMax) {
        auto* const kg = c->n <= 65536 ? keygen_fast_kernel<true> : keygen_fast_kernel<false>;
        hipLaunchKernelGGL(kg, dim3((unsigned)((n_frames + kKeygenFrames - 1) / kKeygenFrames)),
                           dim3(kKeygenBlock), lds, stream, seeds, offset, (uint32_t)c->n, words, (uint32_t)ne,
                           c->keygen_chunk, (uint32_t)n_frames, c->d_jump, matrix ? nullptr : c->d_jpoly,
                           ws->alice_w, ws->bob_w, exact_q, replay);
    } else {
        hipLaunchKernelGGL(keygen_kernel, dim3(blocks_for(n_frames, 64)), dim3(64), 0, stream, seeds, offset,
                           (uint32_t)n_frames, (uint32_t)c->n, words, (uint32_t)ne, ws->alice_w, ws->bob_w,
                           ws->low, exact_q);
    }
    QKD_HIP(hipGetLastError());
    return QKD_OK;
}

}  // namespace qkd

using namespace qkd;

extern "C" {

qkd_status qkd_keygen_batch(const qkd_code* c, qkd_workspace* ws, const uint64_t* seeds,
                            uint64_t seed_offset, size_t n_frames, double q_nominal, uint8_t* alice,
                            uint8_t* bob, double* exact_qber, void* stream) {
    clear_error();
    if (!c || !seeds || !alice || !bob) return set_error(QKD_ERR_INVALID_ARG, "null argument");
    qkd_status s = check_frames(n_frames);
    if (s != QKD_OK) return s;
    DeviceGuard g(c->device);
    ws = resolve_ws(c, ws);
    if (!ws) return set_error(QKD_ERR_OUT_OF_MEMORY, "no workspace");
    WsSession sess(ws, (hipStream_t)stream);
    s = keygen_into_ws(c, ws, seeds, seed_offset, n_frames, q_nominal, exact_qber, (hipStream_t)stream);
    if (s != QKD_OK) return s;
    const uint32_t words = (uint32_t)((c->n + 63) / 64);
    const size_t nb = n_frames * (size_t)c->n;
    hipLaunchKernelGGL(unpack_kernel, dim3(blocks_for(nb, 256)), dim3(256), 0, (hipStream_t)stream,
                       ws->alice_w, (uint32_t)c->n, words, (uint32_t)n_frames, alice);
    hipLaunchKernelGGL(unpack_kernel, dim3(blocks_for(nb, 256)), dim3(256), 0, (hipStream_t)stream,
                       ws->bob_w, (uint32_t)c->n, words, (uint32_t)n_frames, bob);
    QKD_HIP(hipGetLastError());
    return QKD_OK;
}

// ---- interactive mode: one key stream across the QBER points ------------------
// QKD_LDPC_interactive_simulation (simulation.cpp:73-137) seeds ONE
// Xoshiro256PlusPlus(SIMULATION_SEED) (:95) and draws every point's Alice key
// and Bob errors from it in turn (:102-103), so point p starts where point p-1's
// shuffle stopped, Lemire rejections included. A handful of points per run and
// no throughput target: one thread walks the stream exactly as the reference
// does (the batch path's jump-ahead keygen needs independent seeds).
__global__ void keygen_stream_kernel(uint64_t sim_seed, uint32_t n, uint32_t words, uint32_t n_points,
                                     const uint32_t* ne, uint64_t* alice_w, uint64_t* bob_w, uint32_t* low) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    qkdr::Xoshiro256pp g;
    g.seed(sim_seed);
    for (uint32_t p = 0; p < n_points; ++p) {
        uint64_t* A = alice_w + (size_t)p * words;
        uint64_t* B = bob_w + (size_t)p * words;
        for (uint32_t w = 0; w < words; ++w) {
            const uint32_t nb = min(64u, n - w * 64);
            uint64_t v = 0;
            for (uint32_t b = 0; b < nb; ++b) v |= (g.next() >> 63) << b;
            A[w] = v;
            B[w] = v;
        }
        qkdr::shuffle_low_positions(g, n, ne[p], low);
        for (uint32_t k = 0; k < ne[p]; ++k) B[low[k] >> 6] ^= 1ull << (low[k] & 63);
    }
}

}  // extern "C"
