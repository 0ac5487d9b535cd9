// qkd_args.h — host-only argument checks of the batched entry points, free of
// HIP so that a stand-alone host program can exercise them
// (tests/native/reconcile_args_check.cpp, tests/native/verify_hash_check.cpp,
// tests/native/privacy_hash_check.cpp, tests/native/blind_args_check.cpp,
// tests/native/adapt_verify_args_check.cpp, tests/native/ntt_mod_check.cpp,
// tests/native/privacy_kept_check.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qkd_ntt.h"
#include "qkd_privacy.h"

namespace qkda {

// qkd_reconcile_batch's own arguments (the decode parameters and flags are
// check_decode_params', as for qkd_qkd_ldpc_batch): nullptr when they are
// acceptable, else the message of the QKD_ERR_INVALID_ARG to return.
// corrected may be NULL and is not looked at. The QBER test is written so
// that a NaN fails it.
inline const char* reconcile_args_error(const void* code, const uint8_t* bob, const uint8_t* syndrome,
                                        size_t n_frames, double qber, const uint8_t* bits_out,
                                        const uint32_t* iterations, const uint8_t* syndromes_match) {
    if (!code || !bob || !syndrome || !bits_out || !iterations || !syndromes_match) return "null argument";
    if (n_frames == 0) return "n_frames must be > 0";
    if (n_frames > 0xffffffffull) return "n_frames too large";
    if (!(qber > 0.0 && qber < 1.0)) return "QBER must be in (0,1)";
    return nullptr;
}

// What qkd_reconcile_blind_batch adds to qkd_reconcile_adaptive_batch's
// arguments (checked after reconcile_args_error, before the plan is looked
// at): the plan and the reveal counts, at least one round, and a step
// whenever a second round can follow.
inline const char* reconcile_blind_args_error(const void* adapt, const uint32_t* n_revealed, uint32_t step,
                                              uint32_t max_rounds) {
    if (!adapt || !n_revealed) return "null argument";
    if (max_rounds < 1) return "max_rounds must be >= 1";
    if (max_rounds > 1 && step < 1) return "step must be >= 1 when max_rounds > 1";
    return nullptr;
}

// ... and, once the plan's punctured count p is known: the revealed bytes
// exist exactly when there is a punctured bit to reveal.
inline const char* reconcile_blind_revealed_error(int32_t p, const uint8_t* revealed) {
    if ((p > 0) != (revealed != nullptr)) return "revealed is required exactly when the plan punctures";
    return nullptr;
}

// qkd_verify_tags_batch's arguments, the same way. hash_words may be NULL
// (the seeded key string) and is not looked at.
inline const char* verify_tags_args_error(const void* code, const uint8_t* bits, size_t n_frames, uint32_t tag_bits,
                                          const uint64_t* tags) {
    if (!code || !bits || !tags) return "null argument";
    if (n_frames == 0) return "n_frames must be > 0";
    if (n_frames > 0xffffffffull) return "n_frames too large";
    if (tag_bits < 1 || tag_bits > 64) return "tag_bits must be in 1..64";
    return nullptr;
}

// What qkd_reconcile_verify_batch adds to qkd_reconcile_batch's arguments
// (checked after reconcile_args_error): a tag to give or a tag to compare
// with, and verified exactly when alice_tags is given.
inline const char* reconcile_verify_args_error(uint32_t tag_bits, const uint64_t* alice_tags,
                                               const uint64_t* tags_out, const uint8_t* verified) {
    if (tag_bits < 1 || tag_bits > 64) return "tag_bits must be in 1..64";
    if (!alice_tags && !tags_out) return "neither alice_tags nor tags_out given";
    if (alice_tags && !verified) return "alice_tags given without verified";
    if (!alice_tags && verified) return "verified given without alice_tags";
    return nullptr;
}

// qkd_adapt_verify_tags_batch's arguments: qkd_verify_tags_batch's, with the
// plan in the code's place.
inline const char* adapt_verify_tags_args_error(const void* adapt, const uint8_t* payload, size_t n_frames,
                                                uint32_t tag_bits, const uint64_t* tags) {
    return verify_tags_args_error(adapt, payload, n_frames, tag_bits, tags);
}

// What qkd_reconcile_adaptive_verify_batch adds to
// qkd_reconcile_adaptive_batch's arguments (checked after
// reconcile_args_error, before the plan is looked at): the plan, then
// reconcile_verify_args_error's rules.
inline const char* reconcile_adaptive_verify_args_error(const void* adapt, uint32_t tag_bits,
                                                        const uint64_t* alice_tags, const uint64_t* tags_out,
                                                        const uint8_t* verified) {
    if (!adapt) return "null argument";
    return reconcile_verify_args_error(tag_bits, alice_tags, tags_out, verified);
}

// What qkd_reconcile_blind_verify_batch adds to qkd_reconcile_adaptive_batch's
// arguments, the same way: reconcile_blind_args_error's rules first, then
// reconcile_verify_args_error's.
inline const char* reconcile_blind_verify_args_error(const void* adapt, const uint32_t* n_revealed, uint32_t step,
                                                     uint32_t max_rounds, uint32_t tag_bits,
                                                     const uint64_t* alice_tags, const uint64_t* tags_out,
                                                     const uint8_t* verified) {
    if (const char* bad = reconcile_blind_args_error(adapt, n_revealed, step, max_rounds)) return bad;
    return reconcile_verify_args_error(tag_bits, alice_tags, tags_out, verified);
}

// qkd_privacy_amplify_batch's arguments, the same way. hash_words and keep may
// be NULL and are not looked at.
inline const char* privacy_amplify_args_error(const uint8_t* keys, size_t n_frames, uint32_t n_in, uint32_t out_bits,
                                              const uint64_t* out_words) {
    if (!keys || !out_words) return "null argument";
    if (n_frames == 0) return "n_frames must be > 0";
    if (n_frames > 0xffffffffull) return "n_frames too large";
    if (n_in < 1 || n_in > qkdv::kPrivacyMaxBits) return "n_in must be in 1..QKD_PRIVACY_MAX_BITS";
    if (out_bits < 1 || out_bits > n_in) return "out_bits must be in 1..n_in";
    return nullptr;
}

// qkd_privacy_amplify_long_batch's arguments, the same way: a block in the
// frame's place, the long form's size range, and the scratch.
inline const char* privacy_amplify_long_args_error(const uint8_t* keys, size_t n_blocks, uint32_t n_in,
                                                   uint32_t out_bits, const uint64_t* out_words, const void* scratch,
                                                   size_t scratch_bytes) {
    if (!keys || !out_words || !scratch) return "null argument";
    if (n_blocks == 0) return "n_blocks must be > 0";
    if (n_blocks > 0xffffffffull) return "n_blocks too large";
    if (n_in < 1 || n_in > qkdn::kLongMaxBits) return "n_in must be in 1..QKD_PRIVACY_LONG_MAX_BITS";
    if (out_bits < 1 || out_bits > n_in) return "out_bits must be in 1..n_in";
    if (qkdn::long_key_words(n_in, out_bits) == 0) return "n_in + out_bits - 1 exceeds QKD_PRIVACY_LONG_MAX_BITS";
    if (scratch_bytes < qkdn::long_scratch_bytes(n_in, out_bits))
        return "scratch_bytes is below qkd_privacy_long_scratch_bytes(n_in, out_bits)";
    return nullptr;
}

// qkd_privacy_amplify_kept_batch's arguments, the same way: a block of
// frames_per_block frames of frame_bits bits in the long form's n_in (their
// product taken in 64 bits), the frame flags, and this entry's own scratch
// size. hash_words and kept may be NULL and are not looked at.
inline const char* privacy_amplify_kept_args_error(const uint8_t* frames, size_t n_blocks, uint32_t frame_bits,
                                                   uint32_t frames_per_block, uint32_t out_bits, const uint8_t* keep,
                                                   const uint64_t* out_words, const void* scratch,
                                                   size_t scratch_bytes) {
    if (!frames || !keep || !out_words || !scratch) return "null argument";
    if (n_blocks == 0) return "n_blocks must be > 0";
    if (frame_bits < 1 || frames_per_block < 1) return "frame_bits and frames_per_block must be >= 1";
    if (n_blocks > 0xffffffffull || (uint64_t)n_blocks * frames_per_block > 0xffffffffull)
        return "n_blocks * frames_per_block must be below 2^32";
    const uint64_t n_in = (uint64_t)frame_bits * frames_per_block;
    if (n_in > qkdn::kLongMaxBits) return "frame_bits * frames_per_block must be in 1..QKD_PRIVACY_LONG_MAX_BITS";
    if (out_bits < 1 || out_bits > n_in) return "out_bits must be in 1..frame_bits * frames_per_block";
    if (qkdn::long_key_words((uint32_t)n_in, out_bits) == 0)
        return "frame_bits * frames_per_block + out_bits - 1 exceeds QKD_PRIVACY_LONG_MAX_BITS";
    if (scratch_bytes < qkdn::kept_scratch_bytes(frame_bits, frames_per_block, out_bits, n_blocks))
        return "scratch_bytes is below qkd_privacy_kept_scratch_bytes(frame_bits, frames_per_block, out_bits, n_blocks)";
    return nullptr;
}

}  // namespace qkda
