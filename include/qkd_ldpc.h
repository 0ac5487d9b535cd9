/*
 * qkd_ldpc.h — C ABI of the MI355X-native QKD LDPC sum-product decoder.
 *
 * Drop-in boundary for the hot path of ColdCloudd/QKD_LDPC (snapshot
 * 2024-12-23). Every entry point below names the reference interface it
 * replaces (file:line under the reference tree). Plain C types only: no HIP,
 * no torch. Device pointers are raw addresses on the code's device; `stream`
 * is a hipStream_t passed as void* (NULL = the null stream).
 *
 * Bit-exactness contract: for the same inputs, every per-frame output here
 * (decoded bits, iteration count, syndrome match, key match, exact QBER) is
 * identical to the reference's fp64 CPU path (glibc tanh/atanh, flooding
 * schedule, reference accumulation order).
 *
 * Threading: a qkd_code is immutable after creation and may be shared by any
 * number of host threads. Calls that need device scratch take a
 * qkd_workspace*; pass NULL to use the code's internal workspace, which is
 * guarded by a mutex and therefore serialises such calls at the host (calls
 * on different streams then must not overlap on the device: they are
 * ordered by an internal event). For concurrent streams create one
 * workspace per stream. Stream capture: a call of any entry on a stream that
 * is being captured neither waits on nor records that event (a captured
 * record would tie later, uncaptured calls to the capture), so a graph holds
 * the call's own work only; the caller orders the graph's replays against
 * every other use of the same workspace, most simply by replaying on the one
 * stream that uses it.
 *
 * Errors: no exception crosses this boundary. Every call returns a
 * qkd_status; qkd_last_error() returns a thread-local message for the most
 * recent failure on the calling thread. The reference signals the same
 * conditions by throwing std::runtime_error (e.g.
 * array_and_matrix_operations.cpp:116,159,223; simulation.cpp:174).
 */
#ifndef QKD_LDPC_H
#define QKD_LDPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QKD_LDPC_ABI_VERSION 1

#if defined(__GNUC__)
#define QKD_API __attribute__((visibility("default")))
#else
#define QKD_API
#endif

typedef enum qkd_status {
    QKD_OK = 0,
    QKD_ERR_INVALID_ARG = 1,     /* null pointer, zero size, bad flag        */
    QKD_ERR_BAD_CODE = 2,        /* adjacency out of range / inconsistent    */
    QKD_ERR_UNSORTED = 3,        /* an adjacency row is not ascending: the
                                    reference would silently route messages
                                    to the wrong edges (A1 invariant)        */
    QKD_ERR_QBER_TOO_SMALL = 4,  /* floor(N*q) == 0 (simulation.cpp:170-175) */
    QKD_ERR_DEVICE = 5,          /* HIP runtime failure                      */
    QKD_ERR_OUT_OF_MEMORY = 6,
    QKD_ERR_IO = 7,              /* matrix file unreadable / malformed       */
    QKD_ERR_UNSUPPORTED = 8      /* code shape outside what the kernels take */
} qkd_status;

/* Decoder flags (bitwise OR). */
#define QKD_FLAG_THRESHOLD 0x1u  /* CFG.ENABLE_SUM_PRODUCT_MSG_LLR_THRESHOLD
                                    (qkd_ldpc_algorithm.cpp:246,313)         */

/* The binary64 check rule extended to zero LLRs (QKD_VARIANT_SP_F64 only; taken
 * by qkd_decode_batch, implied by qkd_reconcile_adaptive_batch). The
 * reference's rule, c2b_k = 2 atanh(P / t_k) with P = sigma t_0 t_1 ... over
 * the published t_k = tanh(b2c_k / 2) of a check, is 0 / 0 when a t_k is zero
 * (qkd_ldpc_algorithm.cpp:231-241), and a punctured bit IS a zero LLR. With z
 * the number of t_k equal to zero (either sign) and sigma = -1 if the check's
 * syndrome bit is set, else +1:
 *   z = 0   the reference rule, unchanged;
 *   z = 1   the edge whose t is zero gets 2 atanh(P'), P' = sigma times the
 *           non-zero t in ascending edge order; every other edge gets +0.0;
 *   z >= 2  every edge gets +0.0.
 * Clamp, bit phase, decision, stopping rule, iteration count and flags are the
 * reference's; a frame in which no t is ever zero decodes bit for bit as
 * without the flag. Launches with the flag run exact iterations only. */
#define QKD_FLAG_ERASURES 0x2u

/* Check-node rule (flag bits 4-5). QKD_VARIANT_SP_F64 is the reference's
 * decoder (qkd_ldpc_algorithm.cpp:175-345), bit-exact. The other two are
 * build-defined variants with binary32 messages and totals (SURVEY.md §8(d),
 * config 5): same flooding schedule, stopping rule, clamp and outputs; their
 * frame error rates are compared with the reference's, not their frames. */
#define QKD_VARIANT_MASK   0x30u
#define QKD_VARIANT_SP_F64 0x00u  /* sum-product, binary64 (the reference)    */
#define QKD_VARIANT_SP_F32 0x10u  /* sum-product, binary32, Gallager form:
                                     c2b = sign * phi(sum of the other
                                     phi(|b2c|)), phi(x) = -ln tanh(x/2),
                                     hardware exp2/log2                      */
#define QKD_VARIANT_MINSUM 0x20u  /* normalised min-sum, binary32:
                                     c2b = scale * sign * min |b2c| over the
                                     check's other edges                     */
/* Min-sum scale in flag bits 8-15 as round(scale * 256); 0 selects
 * QKD_MINSUM_DEFAULT_SCALE. */
#define QKD_MINSUM_SCALE_SHIFT 8
#define QKD_MINSUM_SCALE(x) ((((uint32_t)((x) * 256.0 + 0.5)) & 0xffu) << QKD_MINSUM_SCALE_SHIFT)
#define QKD_MINSUM_DEFAULT_SCALE 0.8125  /* best FER of {0.625..0.875} on config 3 */
/* Min-sum offset in flag bits 16-23 as round(offset * 64): the message magnitude
 * is max(scale * min |b2c| - offset, 0) (offset min-sum); 0 = no offset. */
#define QKD_MINSUM_OFFSET_SHIFT 16
#define QKD_MINSUM_OFFSET(x) ((((uint32_t)((x) * 64.0 + 0.5)) & 0xffu) << QKD_MINSUM_OFFSET_SHIFT)
/* Self-corrected min-sum (QKD_VARIANT_MINSUM only; needs the LDS-state
 * min-sum kernel): a bit-to-check message whose sign flipped since the last
 * iteration (both nonzero) is erased to 0 before the check rule. */
#define QKD_MINSUM_SELF_CORRECT 0x1000000u

typedef struct qkd_code qkd_code;
typedef struct qkd_workspace qkd_workspace;
typedef struct qkd_adapt qkd_adapt;

typedef struct qkd_code_info {
    int32_t n_bits;              /* H_matrix::num_bit_nodes                  */
    int32_t n_checks;            /* H_matrix::num_check_nodes                */
    int32_t n_edges;
    int32_t max_bit_degree;      /* H_matrix::max_bit_nodes_weight           */
    int32_t max_check_degree;    /* H_matrix::max_check_nodes_weight         */
    int32_t is_regular;          /* H_matrix::is_regular                     */
    int32_t device;
} qkd_code_info;

/* Per-QBER-point reduction of a trial batch (simulation.cpp:252-312): only
 * frames whose syndrome matched contribute to the iteration statistics, and
 * ldpc_ok counts key matches among them. */
typedef struct qkd_counters {
    uint64_t frames;
    uint64_t sp_ok;              /* trials_successful_sp                     */
    uint64_t ldpc_ok;            /* trials_successful_ldpc                   */
    uint64_t sum_iters;          /* sum of iterations over sp_ok frames      */
    uint64_t sum_iters_sq;       /* sum of squares, same frames              */
    uint32_t min_iters;          /* over sp_ok frames (UINT32_MAX if none)   */
    uint32_t max_iters;          /* over sp_ok frames (0 if none)            */
} qkd_counters;

/* ---- library ----------------------------------------------------------- */
QKD_API int qkd_abi_version(void);
QKD_API const char *qkd_last_error(void);
QKD_API const char *qkd_status_string(qkd_status s);
/* Number of visible HIP devices (0 when none; never fails). */
QKD_API int qkd_device_count(void);

/* ---- code object: replaces H_matrix + its readers -----------------------
 * H_matrix (array_and_matrix_operations.hpp:16-27), read_sparse_alist_matrix
 * (array_and_matrix_operations.cpp:109-292), read_dense_matrix (:295-421),
 * free_matrix_H (:88-94).
 * check_ptr[m+1] / check_idx[E]: 0-based CSR of check_nodes (bits of each
 * check, each row ascending). The bit-side lists (bit_nodes) are derived.
 * Validation: indices in range, no duplicate edge, rows ascending
 * (QKD_ERR_UNSORTED otherwise). Device data is uploaded once. */
QKD_API qkd_code *qkd_code_create(int32_t n_bits, int32_t n_checks, const int32_t *check_ptr,
                          const int32_t *check_idx, int device, qkd_status *status);
/* Reads an alist file with the reference reader's rules (weights line,
 * non-zero counts per line, 1-based entries, the first `weight` entries
 * of each line). */
QKD_API qkd_code *qkd_code_from_alist(const char *path, int device, qkd_status *status);
/* Reader options (reader hardening). QKD_READ_SORT_ROWS: sort
 * every bit and check line before validation, so a file whose rows are not
 * ascending is read as the matrix it describes (default: QKD_ERR_UNSORTED,
 * where the reference would silently mis-route messages, §8(a) A1). */
#define QKD_READ_SORT_ROWS 0x1u
QKD_API qkd_code *qkd_code_from_alist_ex(const char *path, int device, uint32_t read_flags,
                                         qkd_status *status);
/* Reads a dense 0/1 matrix file (one row per line). */
QKD_API qkd_code *qkd_code_from_dense(const char *path, int device, qkd_status *status);
QKD_API void qkd_code_destroy(qkd_code *code);
QKD_API qkd_status qkd_code_get_info(const qkd_code *code, qkd_code_info *info);
/* Host copies of the adjacency (any pointer may be NULL). bit_ptr[n+1],
 * bit_idx[E] are the reference's bit_nodes rows (ascending checks). */
QKD_API qkd_status qkd_code_get_adjacency(const qkd_code *code, int32_t *check_ptr, int32_t *check_idx,
                                  int32_t *bit_ptr, int32_t *bit_idx);

/* ---- workspace ------------------------------------------------------------ */
QKD_API qkd_workspace *qkd_workspace_create(const qkd_code *code, qkd_status *status);
QKD_API void qkd_workspace_destroy(qkd_workspace *ws);

/* ---- batched device entry points (all arrays device-resident) ------------ */

/* calculate_syndrome_irregular / _regular (array_and_matrix_operations.cpp:463-486)
 * bits[F*N] (0/1 bytes) -> syndrome[F*M] (0/1 bytes). */
QKD_API qkd_status qkd_syndrome_batch(const qkd_code *code, const uint8_t *bits, size_t n_frames,
                              uint8_t *syndrome, void *stream);

/* sum_product_decoding_irregular / _regular (qkd_ldpc_algorithm.cpp:3-345):
 * llr[F*N] fp64 channel LLRs, syndrome[F*M] 0/1 bytes -> bits_out[F*N] (last
 * hard decision), iterations[F] (SP_result::iterations_num) and
 * syndromes_match[F] (SP_result::syndromes_match). msg_threshold is
 * CFG.SUM_PRODUCT_MSG_LLR_THRESHOLD, applied when QKD_FLAG_THRESHOLD is set.
 * bits_out may be NULL. The only entry that takes QKD_FLAG_ERASURES (LLRs that
 * may be zero; QKD_VARIANT_SP_F64 only, QKD_ERR_INVALID_ARG with another
 * variant before any device work). */
QKD_API qkd_status qkd_decode_batch(const qkd_code *code, qkd_workspace *ws, const double *llr,
                            const uint8_t *syndrome, size_t n_frames, uint32_t max_iterations,
                            double msg_threshold, uint32_t flags, uint8_t *bits_out,
                            uint32_t *iterations, uint8_t *syndromes_match, void *stream);

/* QKD_LDPC_irregular / _regular (qkd_ldpc_algorithm.cpp:347-447), batched:
 * LLR_i = bob_i ? -log((1-q)/q) : +log((1-q)/q), Alice's syndrome, decode,
 * keys_match = (decoded == alice). alice/bob [F*N] 0/1 bytes; one QBER for
 * the batch. bits_out may be NULL. */
QKD_API qkd_status qkd_qkd_ldpc_batch(const qkd_code *code, qkd_workspace *ws, const uint8_t *alice,
                              const uint8_t *bob, size_t n_frames, double qber,
                              uint32_t max_iterations, double msg_threshold, uint32_t flags,
                              uint8_t *bits_out, uint32_t *iterations, uint8_t *syndromes_match,
                              uint8_t *keys_match, void *stream);

/* Bob's side of one-way LDPC reconciliation: sum_product_decoding_* exactly as
 * QKD_LDPC_* calls it (qkd_ldpc_algorithm.cpp:398-431) with the target
 * syndrome given by the caller instead of computed from Alice's key (Alice's
 * half of the protocol is qkd_syndrome_batch on her key).
 * bob[F*N] 0/1 bytes, syndrome[F*M] bytes (nonzero = 1, as qkd_decode_batch),
 * one QBER for the batch. bits_out[F*N] (required): the last hard decision.
 * corrected[F] (may be NULL): popcount(bits_out ^ bob) per frame. For every
 * frame bits_out, iterations and syndromes_match equal what
 * sum_product_decoding_irregular returns for llr_i = bob_i ? -log_p : +log_p,
 * log_p = log((1-q)/q), and that syndrome; with syndrome = H * alice they
 * equal qkd_qkd_ldpc_batch's on (alice, bob). Validation and flags as
 * qkd_qkd_ldpc_batch. Runs that entry's decoders (folded first iteration,
 * tables, speculation) except the frame-interleaved long-code decoder, which
 * produces no decisions: codes of 65,536 < N <= 131,072 bits run the classic
 * kernel here. */
QKD_API qkd_status qkd_reconcile_batch(const qkd_code *code, qkd_workspace *ws, const uint8_t *bob,
                               const uint8_t *syndrome, size_t n_frames, double qber,
                               uint32_t max_iterations, double msg_threshold, uint32_t flags,
                               uint8_t *bits_out, uint32_t *iterations, uint8_t *syndromes_match,
                               uint32_t *corrected, void *stream);

/* ---- key verification ------------------------------------------------------
 * After error correction Alice announces a short universal-hash tag of her
 * key; Bob hashes his corrected key and compares; a frame whose tags differ is
 * thrown away. (syndromes_match alone cannot tell: a decoder that converges to
 * a different word with the same syndrome reports 1.)
 *
 * The hash is a Hankel (Toeplitz-family) matrix over GF(2), given by a key
 * string R of W = qkd_verify_key_words(N) = ceil((N + 63) / 64) 64-bit words.
 * Bit k of the string is r[k] = (R[k >> 6] >> (k & 63)) & 1, 0 <= k <= N + 62;
 * the window W(p), 0 <= p < N, is the 64-bit word whose bit i is r[p + i];
 *   tag(x) = XOR over the positions p with x_p = 1 of W(p), low tag_bits bits
 * (tag bit i = XOR_p r[p + i] x_p). A t-bit tag is the low t bits of the 64-bit
 * tag, 1 <= tag_bits <= 64; the all-zero key has tag 0. Positions are the
 * caller's original bit positions; a key bit is byte & 1.
 *
 * R is the caller's hash_words[W] (device memory; truly random bits shared by
 * Alice and Bob: the form for which the family is 2^-t universal), or, with
 * hash_words == NULL, expanded from the 64-bit hash_seed by SplitMix64 in
 * counter form:
 *   R[k] = mix(hash_seed + (k + 1) * 0x9E3779B97F4A7C15)   (mod 2^64)
 *   mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *           z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 * The seeded form is a computational stand-in, NOT an information-theoretic
 * one: its key string has at most 64 bits of entropy. In either form a tag
 * discloses tag_bits bits of the key, which the caller's privacy amplification
 * has to account for. */

/* W, the number of 64-bit words of the key string for an N-bit key (0 for
 * n_bits < 1). Host only. */
QKD_API size_t qkd_verify_key_words(int32_t n_bits);

/* The W words the seeded form uses, into host memory (to inspect them, or to
 * upload them as hash_words). Host only, no device work. */
QKD_API qkd_status qkd_verify_expand_key(uint64_t hash_seed, int32_t n_bits, uint64_t *words_host);

/* Alice's half (and anyone's who holds byte keys): tags[f] = tag(bits[f]) for
 * bits[F*N] 0/1 bytes on the device (only byte & 1 counts; rows of any
 * alignment). One kernel launch on the stream, no workspace, no host copy, no
 * synchronisation: capturable in a graph. */
QKD_API qkd_status qkd_verify_tags_batch(const qkd_code *code, const uint8_t *bits, size_t n_frames,
                               uint64_t hash_seed, const uint64_t *hash_words, uint32_t tag_bits,
                               uint64_t *tags, void *stream);

/* Bob's half: qkd_reconcile_batch (same arguments, same order, and bit for bit
 * the same bits_out, iterations, syndromes_match and corrected) followed by
 * verification of the corrected key, in the kernel that writes bits_out where
 * the decoder has one. tags_out[F] (may be NULL): tag(bits_out[f]), masked.
 * alice_tags[F] (may be NULL): Alice's announced tags; then verified[F]
 * (required exactly when alice_tags is given):
 *   verified[f] = syndromes_match[f] && ((tag ^ alice_tags[f]) & mask) == 0.
 * QKD_ERR_INVALID_ARG, before any device work, when both alice_tags and
 * tags_out are NULL, when tag_bits is outside 1..64, or when verified and
 * alice_tags are not given together. */
QKD_API qkd_status qkd_reconcile_verify_batch(const qkd_code *code, qkd_workspace *ws, const uint8_t *bob,
                               const uint8_t *syndrome, size_t n_frames, double qber,
                               uint32_t max_iterations, double msg_threshold, uint32_t flags,
                               uint8_t *bits_out, uint32_t *iterations, uint8_t *syndromes_match,
                               uint32_t *corrected, uint64_t hash_seed, const uint64_t *hash_words,
                               uint32_t tag_bits, const uint64_t *alice_tags, uint64_t *tags_out,
                               uint8_t *verified, void *stream);

/* ---- rate adaptation: punctured and shortened frames -------------------------
 * One mother code serves a range of channels (Elkouss et al.): of the N bits of
 * a frame, p punctured positions hold Alice's private random bits, which are
 * never disclosed (Bob's LLR there is 0: the rate goes up), s shortened
 * positions hold 0 on both sides (Bob's LLR there is +known_llr: the rate goes
 * down), and the other n_payload = N - p - s positions hold the key: payload
 * bit k lives at the k-th position, in ascending order, that is neither
 * punctured nor shortened. A qkd_adapt is such a choice for one code, uploaded
 * once; immutable and shareable like a code. It must be destroyed before its
 * code. No reference counterpart (the reference has one rate per matrix). */
typedef struct qkd_adapt_info {
    int32_t n_bits;
    int32_t n_payload;           /* N - p - s                                */
    int32_t n_punctured;
    int32_t n_shortened;
} qkd_adapt_info;

/* punctured[p], shortened[s]: host arrays of positions (NULL with a count of
 * 0). QKD_ERR_INVALID_ARG unless every position is in [0, N), all p + s are
 * distinct and n_payload >= 1. */
QKD_API qkd_adapt *qkd_adapt_create(const qkd_code *code, const int32_t *punctured, int32_t p,
                                    const int32_t *shortened, int32_t s, qkd_status *status);
QKD_API void qkd_adapt_destroy(qkd_adapt *adapt);
QKD_API qkd_status qkd_adapt_get_info(const qkd_adapt *adapt, qkd_adapt_info *info);

/* A deterministic "untainted" choice of `count` positions of a code given as a
 * check-side CSR (as qkd_code_create), which both sides compute from a shared
 * seed. Host only, no device. Candidates are visited in the order of a
 * Fisher-Yates shuffle of 0..N-1 driven by the library's SplitMix64 counter
 * form: R[k] = mix(seed + (k + 1) * 0x9E3779B97F4A7C15) (qkd_verify_expand_key),
 * j = R[k] mod (i + 1), swap entries i and j, for i from N-1 down to 1, k
 * counting up from 0. Pass 1 takes a candidate when none of its checks is
 * adjacent to an earlier pick and stops at `count`; pass 2 fills any remainder
 * with the untaken candidates in the same order. positions_host[count]: the
 * positions in the order they were taken; *untainted_out (may be NULL): how
 * many pass 1 took. A caller punctures the first p and shortens the next s.
 * 0 <= count <= N. */
QKD_API qkd_status qkd_adapt_positions(int32_t n_bits, int32_t n_checks, const int32_t *check_ptr,
                                       const int32_t *check_idx, int32_t count, uint64_t seed,
                                       int32_t *positions_host, int32_t *untainted_out);

/* Alice's half is qkd_adapt_embed_batch followed by qkd_syndrome_batch.
 * payload[F * n_payload] 0/1 bytes (only byte & 1 counts; rows of any
 * alignment), fill[F * p] her random bits for the punctured positions in the
 * order of the plan's punctured list (required exactly when p > 0; there is
 * deliberately no seeded form), shortened positions are written as 0 ->
 * frames[F * N]. extract: frames[F * N] -> payload[F * n_payload] (byte & 1).
 * All arrays on the plan's device. Kernel launches on the stream only: no
 * workspace, no allocation, no host copy, no synchronisation; capturable. */
QKD_API qkd_status qkd_adapt_embed_batch(const qkd_adapt *adapt, const uint8_t *payload, size_t n_frames,
                                         const uint8_t *fill, uint8_t *frames, void *stream);
QKD_API qkd_status qkd_adapt_extract_batch(const qkd_adapt *adapt, const uint8_t *frames, size_t n_frames,
                                           uint8_t *payload, void *stream);

/* Bob's half. For every frame the N-bit decision, iterations and
 * syndromes_match equal what qkd_decode_batch returns with
 * flags | QKD_FLAG_ERASURES for the LLRs
 *   payload position holding Bob's bit b:  b ? -log_p : +log_p,
 *                                          log_p = log((1 - q) / q) as qkd_reconcile_batch
 *   punctured position:                    +0.0
 *   shortened position:                    +known_llr
 * but no LLR array exists: the decoder reads one class byte per bit, written by
 * one small kernel from bob_payload[F * n_payload] and the plan.
 * payload_out[F * n_payload] (required): the payload of the decision;
 * frames_out[F * N] (may be NULL): the whole decision; corrected[F] (may be
 * NULL): popcount(payload_out ^ bob_payload). known_llr must be finite and > 0
 * (the clamp's value makes a shortened bit publish t = 1.0 exactly); the plan
 * must have been created for `code`; everything else is validated as
 * qkd_reconcile_batch does. QKD_FLAG_ERASURES is implied. Only
 * QKD_VARIANT_SP_F64: another variant returns QKD_ERR_UNSUPPORTED. Code sizes as
 * qkd_decode_batch. Exact iterations only (no folded first iteration, tables or
 * speculation in this mode). */
QKD_API qkd_status qkd_reconcile_adaptive_batch(const qkd_code *code, qkd_workspace *ws, const qkd_adapt *adapt,
                                                const uint8_t *bob_payload, const uint8_t *syndrome,
                                                size_t n_frames, double qber, double known_llr,
                                                uint32_t max_iterations, double msg_threshold, uint32_t flags,
                                                uint8_t *payload_out, uint8_t *frames_out, uint32_t *iterations,
                                                uint8_t *syndromes_match, uint32_t *corrected, void *stream);

/* Blind reconciliation (Martinez-Mateo et al.): rate adaptation made
 * interactive. Alice sends one syndrome; Bob decodes; for the frames that fail,
 * Alice discloses the values of the next punctured bits, in the order of the
 * plan's punctured list, and Bob decodes those frames again with these
 * positions as known bits instead of erasures. No new syndrome, no QBER
 * estimate, and each frame stops at its own rate.
 *
 * revealed[F * p]: byte f * p + j is the value (byte & 1) of frame f's punctured
 * bit of rank j, the j-th of the plan's punctured list, i.e. Alice's fill byte
 * (qkd_adapt_embed_batch). n_revealed[F], in/out: how many of them Bob holds for
 * frame f. The call never reads revealed[f * p + j] for j >= n_revealed[f].
 * skip[F] (may be NULL), rounds[F] (may be NULL); the other arguments as
 * qkd_reconcile_adaptive_batch. All arrays on the plan's device.
 *
 *  - Skipped frames. A frame with skip[f] != 0 is not decoded and none of its
 *    outputs is written (n_revealed[f] and rounds[f] included).
 *  - Rounds. The other frames are open at round 0. In round
 *    t = 0 .. max_rounds-1 every open frame is decoded.
 *  - Decision. The N-bit decision, iterations and syndromes_match equal what
 *    qkd_decode_batch returns with flags | QKD_FLAG_ERASURES for the LLRs
 *      payload position holding Bob's bit b:      b ? -log_p : +log_p
 *      shortened position:                        +known_llr
 *      punctured position of rank j < min(n_revealed[f], p):
 *                                  revealed[f * p + j] & 1 ? -known_llr : +known_llr
 *      other punctured position:                  +0.0
 *  - Outputs. The frame's outputs are overwritten with this round's;
 *    corrected[f] = popcount(payload_out ^ bob_payload) as before.
 *  - Closing a frame. A frame that matched is closed. So is a frame that
 *    failed with n_revealed[f] >= p: it has nothing more to reveal and is not
 *    decoded again on the same input.
 *  - Advancing a frame. A frame that failed with bits left, while another
 *    round follows, gets n_revealed[f] = min(p, n_revealed[f] + step). On
 *    return n_revealed[f] is therefore the count its last decode used.
 *  - rounds[f]: how many rounds decoded frame f; written for every frame that
 *    is not skipped.
 *  - n_revealed[f] > p on entry counts as p (and is returned as p).
 *  - max_rounds = 1 is Bob's step on a real link: he decodes with what he
 *    has, asks Alice for more, and calls again with skip set for the frames
 *    that are done. step is then not used.
 *  - max_rounds > 1: revealed holds Alice's whole fill; the simulation and
 *    benchmark form, as qkd_trials_batch is for the fixed-rate path.
 *  - Zero reveals. With n_revealed all 0, skip NULL and max_rounds = 1 the
 *    call returns exactly what qkd_reconcile_adaptive_batch returns.
 *
 * Validated before any device work: everything qkd_reconcile_adaptive_batch
 * validates; max_rounds >= 1; step >= 1 when max_rounds > 1; n_revealed not
 * NULL; revealed not NULL exactly when p > 0. Only QKD_VARIANT_SP_F64
 * (otherwise QKD_ERR_UNSUPPORTED); exact iterations only.
 *
 * A round is three kernels on the stream: one that settles the round before
 * and lists the open frames, one that writes their class bytes (classes 4 and
 * 5: a revealed 0 and a revealed 1), and the decoder, at its usual grid, over
 * that list; a workgroup that finds the list exhausted exits. The host never
 * reads the list's length: no synchronisation, no host copy, no allocation
 * beyond the workspace's grow-on-demand; capturable once the workspace has its
 * size (see "Stream capture" at the top for the workspace's ordering then). */
QKD_API qkd_status qkd_reconcile_blind_batch(const qkd_code *code, qkd_workspace *ws, const qkd_adapt *adapt,
                                             const uint8_t *bob_payload, const uint8_t *syndrome, size_t n_frames,
                                             double qber, double known_llr, uint32_t max_iterations,
                                             double msg_threshold, uint32_t flags, const uint8_t *revealed,
                                             uint32_t *n_revealed, const uint8_t *skip, uint32_t step,
                                             uint32_t max_rounds, uint8_t *payload_out, uint8_t *frames_out,
                                             uint32_t *iterations, uint8_t *syndromes_match, uint32_t *corrected,
                                             uint32_t *rounds, void *stream);

/* ---- key verification of punctured and shortened frames ----------------------
 * The verification hash above applied to the payload: positions are payload
 * indices k, 0 <= k < n_payload, the key string has
 * W = qkd_verify_key_words(n_payload) words (hash_words[W] on the device, or
 * expanded from hash_seed when hash_words is NULL), tag_bits is 1..64 and a key
 * bit is byte & 1. With the same string the tag is the low tag_bits bits of
 * qkd_privacy_amplify_batch(n_in = n_payload, out_bits = 64) on the payload.
 *
 * Alice's half: tags[f] = tag(payload[f]) for payload[F * n_payload] on the
 * plan's device. One launch of the byte-key tag kernel on the stream, no
 * workspace, no host copy, no synchronisation: capturable. Validated as
 * qkd_verify_tags_batch, with the plan in the code's place. */
QKD_API qkd_status qkd_adapt_verify_tags_batch(const qkd_adapt *adapt, const uint8_t *payload, size_t n_frames,
                                               uint64_t hash_seed, const uint64_t *hash_words, uint32_t tag_bits,
                                               uint64_t *tags, void *stream);

/* Bob's half on the rate-adaptive path: qkd_reconcile_adaptive_batch (same
 * arguments, same order, and bit for bit the same payload_out, frames_out,
 * iterations, syndromes_match and corrected) with the payload's tag taken by
 * the decoder kernel itself, in the loop that writes payload_out: no separate
 * pass over the payload. hash_seed .. verified mean what they mean for
 * qkd_reconcile_verify_batch and follow its rules (at least one of alice_tags
 * and tags_out; verified exactly when alice_tags is given; QKD_ERR_INVALID_ARG
 * before any device work otherwise):
 *   tags_out[f] = tag(payload_out[f]), masked, whether or not the frame matched;
 *   verified[f] = syndromes_match[f] && ((tag ^ alice_tags[f]) & mask) == 0.
 * The seeded key string is expanded once per call by a small kernel into the
 * workspace (grow-on-demand). */
QKD_API qkd_status qkd_reconcile_adaptive_verify_batch(
    const qkd_code *code, qkd_workspace *ws, const qkd_adapt *adapt, const uint8_t *bob_payload,
    const uint8_t *syndrome, size_t n_frames, double qber, double known_llr, uint32_t max_iterations,
    double msg_threshold, uint32_t flags, uint8_t *payload_out, uint8_t *frames_out, uint32_t *iterations,
    uint8_t *syndromes_match, uint32_t *corrected, uint64_t hash_seed, const uint64_t *hash_words,
    uint32_t tag_bits, const uint64_t *alice_tags, uint64_t *tags_out, uint8_t *verified, void *stream);

/* Bob's half of blind reconciliation with verification:
 * qkd_reconcile_blind_batch's arguments followed by the same six. Alice
 * announces one tag per frame together with the syndrome; Bob compares in every
 * round; the disclosure is tag_bits once per frame.
 *  - With alice_tags given, every clause of qkd_reconcile_blind_batch's contract
 *    that reads "a frame that matched" reads "a frame that is verified": a frame
 *    is closed when verified[f] holds. A frame whose syndrome matches but whose
 *    tag differs is treated exactly like a failed frame: closed if
 *    n_revealed[f] >= p, otherwise, while another round follows, given `step`
 *    more bits and decoded again (a revealed bit that contradicts the wrong word
 *    can move the decoder off it; Alice sends nothing new for this).
 *  - With only tags_out given, closing stays on syndromes_match.
 *  - tags_out and verified are overwritten with each round's values like the
 *    other outputs, and are not written for skipped frames.
 *  - max_rounds = 1 stays Bob's step on a real link; he sets skip from verified.
 *  - If every frame whose syndrome matches also has a matching tag, all other
 *    outputs equal qkd_reconcile_blind_batch's.
 * The kernel-and-launch contract of qkd_reconcile_blind_batch holds unchanged
 * (the round kernel reads verified in place of syndromes_match): no host
 * synchronisation, no host copy, no allocation beyond the workspace's
 * grow-on-demand; capturable once the workspace has its size. */
QKD_API qkd_status qkd_reconcile_blind_verify_batch(
    const qkd_code *code, qkd_workspace *ws, const qkd_adapt *adapt, const uint8_t *bob_payload,
    const uint8_t *syndrome, size_t n_frames, double qber, double known_llr, uint32_t max_iterations,
    double msg_threshold, uint32_t flags, const uint8_t *revealed, uint32_t *n_revealed, const uint8_t *skip,
    uint32_t step, uint32_t max_rounds, uint8_t *payload_out, uint8_t *frames_out, uint32_t *iterations,
    uint8_t *syndromes_match, uint32_t *corrected, uint32_t *rounds, uint64_t hash_seed,
    const uint64_t *hash_words, uint32_t tag_bits, const uint64_t *alice_tags, uint64_t *tags_out,
    uint8_t *verified, void *stream);

/* ---- privacy amplification --------------------------------------------------
 * The last step before a secret key: the corrected (and verified) key is
 * hashed down to out_bits bits with a matrix of the same Hankel family as the
 * verification hash, only with a long output. For an input of n_in bits x_p
 * and an output of L = out_bits bits:
 *   out_i = XOR over the positions p with x_p = 1 of r[p + i],  0 <= i < L
 * where r[k] = (R[k >> 6] >> (k & 63)) & 1, 0 <= k <= n_in + L - 2, is bit k of
 * a key string R of Wp = qkd_privacy_key_words(n_in, L) =
 * ceil((n_in + L - 1) / 64) 64-bit words. The all-zero input hashes to all
 * zeros; an input bit is byte & 1. The output of a frame is packed into
 * Wo = ceil(L / 64) words: bit i of frame f is
 * (out_words[f * Wo + (i >> 6)] >> (i & 63)) & 1, and the bits at and above L
 * of the last word are written as 0.
 *
 * R is the caller's hash_words[Wp] (device memory; truly random bits shared
 * by Alice and Bob: the form for which the family is universal), or, with
 * hash_words == NULL, expanded from hash_seed as for verification:
 * R[k] = mix(hash_seed + (k + 1) * 0x9E3779B97F4A7C15). The seeded form is a
 * computational stand-in, NOT an information-theoretic one: its key string has
 * at most 64 bits of entropy.
 *
 * With n_in = N, L = 64 and the same key string the output word IS the 64-bit
 * verification tag (qkd_privacy_key_words(N, 64) == qkd_verify_key_words(N)).
 * A link must therefore NOT reuse its verification string (or seed) for
 * privacy amplification: the announced tag would be 64 bits of the secret key.
 * The two strings must be independent.
 *
 * How many bits to keep (out_bits) is the caller's protocol decision: the
 * syndrome bits disclosed, the tag bits, the finite-key terms and the security
 * parameter all come off there. */
#define QKD_PRIVACY_MAX_BITS (1u << 20)   /* n_in and out_bits */

/* Wp, the 64-bit words of the key string; 0 unless
 * 1 <= out_bits <= n_in <= QKD_PRIVACY_MAX_BITS. Host only. */
QKD_API size_t qkd_privacy_key_words(uint32_t n_in, uint32_t out_bits);

/* The Wp words the seeded form uses, into host memory (to inspect them, or to
 * upload them as hash_words). Host only, no device work. */
QKD_API qkd_status qkd_privacy_expand_key(uint64_t hash_seed, uint32_t n_in, uint32_t out_bits,
                                          uint64_t *words_host);

/* out_words[F * Wo] = the hashes of keys[F * n_in] (0/1 bytes on `device`, only
 * byte & 1 counts; contiguous rows, base address of any alignment). n_in is
 * not tied to a code: to hash B consecutive corrected frames as one block pass
 * the same buffer with n_in = B * N and n_frames = F / B. keep[F] (may be NULL;
 * typically `verified` of qkd_reconcile_verify_batch): a frame with
 * keep[f] == 0 gets Wo zero words, so that an unverified key never leaves as a
 * secret key; the other frames are unaffected. out_words is fully overwritten
 * and nothing is written outside it. QKD_ERR_INVALID_ARG, before any device
 * work, unless 1 <= out_bits <= n_in <= QKD_PRIVACY_MAX_BITS, n_frames >= 1 and
 * keys and out_words are given. Kernel launches on the stream only: no
 * workspace, no allocation, no host copy, no synchronisation, no atomics (the
 * same bits on every run); capturable in a graph. */
QKD_API qkd_status qkd_privacy_amplify_batch(int device, const uint8_t *keys, size_t n_frames,
                                             uint32_t n_in, uint32_t out_bits, uint64_t hash_seed,
                                             const uint64_t *hash_words, const uint8_t *keep,
                                             uint64_t *out_words, void *stream);

/* ---- long-block privacy amplification ----------------------------------------
 * The same hash, bit for bit, for blocks past QKD_PRIVACY_MAX_BITS: a
 * finite-key analysis sets out_bits from the block length and wants blocks of
 * 10^7 to 10^8 bits. Where qkd_privacy_amplify_batch does n_in * out_bits
 * work, this entry takes the hash as a cyclic convolution of the input with
 * the key string by number-theoretic transforms modulo 15 * 2^27 + 1, of
 * length T = the power of two at or above n_in + L - 1 (at least 64):
 * O(T log T). The range is 1 <= out_bits <= n_in with
 * n_in + out_bits - 1 <= QKD_PRIVACY_LONG_MAX_BITS, e.g. 2^26 + 1 bits hashed
 * to 2^26, or 10^8 to 3.4 * 10^7. Every shape both entries accept gives the
 * same words from both. The key string is hash_words[Wp] or the seeded form as
 * above (a computational stand-in, NOT an information-theoretic one), Wp =
 * qkd_privacy_long_key_words(n_in, L) = ceil((n_in + L - 1) / 64), equal to
 * qkd_privacy_key_words wherever that is defined. */
#define QKD_PRIVACY_LONG_MAX_BITS (1u << 27)   /* n_in + out_bits - 1 */

/* Wp of the long form; 0 unless 1 <= out_bits <= n_in and
 * n_in + out_bits - 1 <= QKD_PRIVACY_LONG_MAX_BITS. Host only. */
QKD_API size_t qkd_privacy_long_key_words(uint32_t n_in, uint32_t out_bits);

/* The Wp words the seeded form uses, into host memory: the words of
 * qkd_privacy_expand_key, over the long form's range. Host only. */
QKD_API qkd_status qkd_privacy_long_expand_key(uint64_t hash_seed, uint32_t n_in, uint32_t out_bits,
                                               uint64_t *words_host);

/* The bytes of device scratch one call needs (two arrays of T 32-bit residues
 * and a twiddle table of about 2 sqrt(T) entries: 8 T bytes and a little, about
 * 1 GiB at T = 2^27); 0 for sizes outside the range. Depends on the sizes
 * only, not on n_blocks. Host only. */
QKD_API size_t qkd_privacy_long_scratch_bytes(uint32_t n_in, uint32_t out_bits);

/* out_words[n_blocks * Wo] = the hashes of keys[n_blocks * n_in] (0/1 bytes on
 * `device`, only byte & 1 counts; contiguous blocks, base address of any
 * alignment), Wo = ceil(out_bits / 64), packed as by qkd_privacy_amplify_batch.
 * keep[n_blocks] (may be NULL) is per BLOCK: a block with keep[b] == 0 gets Wo
 * zero words. A caller who wants only the verified frames of a block calls
 * qkd_privacy_amplify_kept_batch (below), which compacts them on the device
 * at the block's fixed length. scratch: device memory of at least
 * qkd_privacy_long_scratch_bytes(n_in, out_bits) bytes, any alignment, any
 * contents; the blocks of a call run one after another through it, and the
 * key string's transform is taken once per call. out_words is fully
 * overwritten and nothing is written outside it and the scratch.
 * QKD_ERR_INVALID_ARG, before any device work, for NULL keys, out_words or
 * scratch, n_blocks of 0 or >= 2^32, sizes outside the range, scratch_bytes
 * below qkd_privacy_long_scratch_bytes, or a bad device. Kernel launches on the
 * stream only: no allocation, no host copy, no synchronisation, no atomics
 * (the same bits on every run); capturable in a graph. */
QKD_API qkd_status qkd_privacy_amplify_long_batch(int device, const uint8_t *keys, size_t n_blocks,
                                                  uint32_t n_in, uint32_t out_bits, uint64_t hash_seed,
                                                  const uint64_t *hash_words, const uint8_t *keep,
                                                  uint64_t *out_words, void *scratch, size_t scratch_bytes,
                                                  void *stream);

/* ---- long-block privacy amplification of the kept frames of a block -----------
 * The link between verification and the long form: a block is
 * B = frames_per_block frames of N = frame_bits bits, keep[] holds one flag per
 * FRAME (typically `verified` of qkd_reconcile_verify_batch), and only the kept
 * frames are hashed, without the host ever reading a flag. With n_in = B * N,
 * L = out_bits and Wo = ceil(L / 64):
 *
 * For block b let x_b be its kept frames set end to end in ascending frame
 * order, followed by zeros up to n_in bits. out_words[b * Wo ..] is, word for
 * word, what qkd_privacy_amplify_long_batch gives for x_b with n_in, L, the
 * same key string (hash_words[Wp], Wp = qkd_privacy_long_key_words(n_in, L), or
 * the same seed) and keep == NULL. kept[b] (may be NULL) is the number of kept
 * frames of block b. So:
 *   - a block with no kept frame gets Wo zero words;
 *   - with every frame kept the call is qkd_privacy_amplify_long_batch on the
 *     same buffer;
 *   - the bytes of a dropped frame have no effect on any output;
 *   - the PREFIX RULE: out_i = XOR_p r[p + i] x_p depends neither on the zeros
 *     behind the input nor on out_bits, so for any L' <= min(L, kept[b] * N)
 *     the first L' output bits of block b are
 *     qkd_privacy_amplify_long_batch(the kept frames compacted,
 *     n_in = kept[b] * N, out_bits = L') under the first
 *     qkd_privacy_long_key_words(kept[b] * N, L') words of the same string, or
 *     under the same seed.
 * The caller's finite-key formula picks the final length l <= out_bits from
 * kept[b] and takes the first l bits. Alice, who makes the same call on her
 * frames, gets the same bits as long as both sides use the same keep flags
 * (they are public), the same B and the same l.
 *
 * frames[n_blocks * B * N]: 0/1 bytes on `device`, only byte & 1 counts, any
 * base alignment. keep[n_blocks * B]: required, device memory; a frame is kept
 * when its byte is nonzero (any nonzero value). kept[n_blocks]: device memory
 * or NULL. scratch: device memory of at least
 * qkd_privacy_kept_scratch_bytes(N, B, L, n_blocks) bytes, any alignment, any
 * contents. out_words and kept are fully overwritten, and nothing is written
 * outside them and the scratch.
 * QKD_ERR_INVALID_ARG, before any device work, for NULL frames, keep,
 * out_words or scratch; n_blocks of 0; n_blocks * B >= 2^32; N < 1 or B < 1;
 * B * N (taken in 64 bits) above QKD_PRIVACY_LONG_MAX_BITS; out_bits outside
 * 1..B * N; B * N + out_bits - 1 > QKD_PRIVACY_LONG_MAX_BITS; scratch_bytes
 * below qkd_privacy_kept_scratch_bytes; or a bad device. Kernel launches on the
 * stream only (one scan of the flags per call, then per block an input stage
 * that gathers the kept frames and the long form's passes): no allocation, no
 * host copy, no synchronisation, no atomics (the same bits on every run);
 * capturable in a graph, and a replay follows the flags' current contents. */

/* The bytes of device scratch one call needs:
 * qkd_privacy_long_scratch_bytes(B * N, out_bits), plus a frame list of
 * n_blocks * B 32-bit entries, one byte per block, and 16 bytes of alignment
 * slack. Unlike the long form's size it depends on n_blocks. 0 for sizes
 * outside the range (B * N in 64 bits or out_bits outside the long form's,
 * n_blocks of 0, n_blocks * B >= 2^32). Host only. */
QKD_API size_t qkd_privacy_kept_scratch_bytes(uint32_t frame_bits, uint32_t frames_per_block,
                                              uint32_t out_bits, size_t n_blocks);

QKD_API qkd_status qkd_privacy_amplify_kept_batch(int device, const uint8_t *frames, size_t n_blocks,
                                                  uint32_t frame_bits, uint32_t frames_per_block,
                                                  uint32_t out_bits, uint64_t hash_seed,
                                                  const uint64_t *hash_words, const uint8_t *keep,
                                                  uint64_t *out_words, uint32_t *kept, void *scratch,
                                                  size_t scratch_bytes, void *stream);

/* generate_random_bit_array + introduce_errors (array_and_matrix_operations.cpp:424-460)
 * for frame k seeded with seeds[k] + seed_offset (simulation.cpp:163,247),
 * on the device. alice/bob [F*N] 0/1 bytes; exact_qber[F] may be NULL.
 * Returns QKD_ERR_QBER_TOO_SMALL when floor(N*q_nominal) == 0. */
QKD_API qkd_status qkd_keygen_batch(const qkd_code *code, qkd_workspace *ws, const uint64_t *seeds,
                            uint64_t seed_offset, size_t n_frames, double q_nominal,
                            uint8_t *alice, uint8_t *bob, double *exact_qber, void *stream);

/* run_trial (simulation.cpp:161-189) for F frames, fused on the device:
 * keygen -> LLR -> Alice syndrome -> decode -> key compare. Per-frame outputs
 * (any may be NULL) and, if counters != NULL (device memory, one
 * qkd_counters), the batch reduction of simulation.cpp:252-312. */
QKD_API qkd_status qkd_trials_batch(const qkd_code *code, qkd_workspace *ws, const uint64_t *seeds,
                            uint64_t seed_offset, size_t n_frames, double q_nominal,
                            uint32_t max_iterations, double msg_threshold, uint32_t flags,
                            uint32_t *iterations, uint8_t *syndromes_match, uint8_t *keys_match,
                            double *exact_qber, qkd_counters *counters, void *stream);

/* QKD_LDPC_interactive_simulation (simulation.cpp:73-137) over n_points
 * nominal QBERs (host array): ONE xoshiro256++(simulation_seed) stream feeds
 * every point's key pair in turn (:95, :102-103), then each point runs
 * QKD_LDPC_* at its exact QBER (:122-129). Outputs are HOST arrays of
 * n_points: iterations, syndromes_match, keys_match (the reference prints
 * SUCCESSFUL when both hold, :131), exact_qber ("Actual QBER"), errors
 * ("Number of errors in a key"). *points_done = points run. Like the
 * reference, a point with floor(N*q) == 0 stops the run there and returns
 * QKD_ERR_QBER_TOO_SMALL with the earlier points' results filled in.
 * Synchronous (device-synchronising); ws may be NULL. */
QKD_API qkd_status qkd_interactive_batch(const qkd_code *code, qkd_workspace *ws, uint64_t simulation_seed,
                                         size_t n_points, const double *q_nominal, uint32_t max_iterations,
                                         double msg_threshold, uint32_t flags, uint32_t *iterations,
                                         uint8_t *syndromes_match, uint8_t *keys_match, double *exact_qber,
                                         uint32_t *errors, size_t *points_done);

/* Reduction alone: per-frame results -> counters (device memory). */
QKD_API qkd_status qkd_counters_batch(const uint32_t *iterations, const uint8_t *syndromes_match,
                              const uint8_t *keys_match, size_t n_frames, qkd_counters *counters,
                              int device, void *stream);

/* Combination of n_records counter records (device memory, e.g. one per rank
 * after an all-gather) into *out (device memory; may alias a record): the
 * reduction the reference's single process performs over every trial of a
 * point (simulation.cpp:252-312) -- sums add, min_iters / max_iters take the
 * minimum / maximum. One launch on `stream`. */
QKD_API qkd_status qkd_counters_merge(const qkd_counters *records, size_t n_records, qkd_counters *out,
                                      int device, void *stream);

/* ---- diagnostics ------------------------------------------------------------
 * Debug and A/B options. The library reads NO environment variable: every
 * option defaults to the product behaviour and changes only through this
 * call. ws != NULL sets the option for that workspace; ws == NULL sets the
 * process-wide value every workspace uses unless it has its own. value NULL
 * restores the default. Options (test infrastructure; outputs are bit-exact
 * under every value unless a variant says otherwise):
 *   QKD_SPEC_CAP <k>           interval iterations per frame before the exact
 *                              ones (0: off; default 8)
 *   QKD_SPEC_CKPT 0|1          force the checkpointed speculation off / on
 *   QKD_CKPT_UNSAT <k>         its trigger (unsatisfied checks; default 128)
 *   QKD_SPEC_POLICY always     the in-launch replay policy never turns off
 *   QKD_FOLD_TABLE 0           the folded first iteration per bit, not tabled
 *   QKD_DECODE_KERNEL classic  the classic message-store decoder
 *   QKD_MINSUM_STORE lds|global  the LDS-state / global-store min-sum kernels
 *   QKD_DECODE_GRID <k>        cap the decoder's resident workgroups
 *   QKD_SPLIT_BUDGET <bytes>   lower the split decoder's LDS budget
 *   QKD_C2B_PAD <slots>        a fixed pad of the split decoder's regions
 *   QKD_ILV 0|1, QKD_ILV_GRID <k>  the interleaved long-code decoder off / on,
 *                              its workgroup cap
 *   QKD_KEYGEN serial|replay|lanes|matrix  the other key generators
 *   QKD_SYN_SLICED 0, QKD_SYN_BYTES 0  the gather frame-syndrome kernel / the
 *                              separate key packing
 *   QKD_BIT_ORDER identity|runs  (ws == NULL, read when a code is created)
 *                              the split decoder's internal bit order
 *   QKD_PHASE_TIMING 1         per-phase shader clocks (qkd_debug_phase_cycles)
 *   QKD_CHECK_LANES 0|1|2      the speculative check phases of check degrees
 *                              <= 6: 0 one edge per lane; 1 (default) one
 *                              check per lane in whole rounds of tasks, the
 *                              remaining checks edge per lane; 2 every check
 *                              on a lane (A/B). Chosen per launch; outputs
 *                              are the same
 *   QKD_PRIVACY_KERNEL direct|table  (ws == NULL) the form of
 *                              qkd_privacy_amplify_batch: one lane per output
 *                              word, or bit-sliced over 32 frames with lookup
 *                              tables in LDS (the default; table1 | table2 |
 *                              table4 fix its outputs per lane, which it
 *                              otherwise chooses from the launch's size)
 *   QKD_PRIVACY_NTT_LOG2 <S>   (ws == NULL) 3..13: log2 of the residues one
 *                              workgroup of qkd_privacy_amplify_long_batch
 *                              transforms in LDS (default 13); a small S
 *                              runs the many-pass paths at a few hundred points
 * An unknown name fails with QKD_ERR_INVALID_ARG. Thread-safe. No reference
 * counterpart (the reference's CFG fields are the decode parameters). */
QKD_API qkd_status qkd_debug_set_option(qkd_workspace *ws, const char *name, const char *value);
/* With QKD_PHASE_TIMING set (qkd_debug_set_option), decode launches on `ws`
 * accumulate shader-clock cycles per phase, summed over workgroups (thread 0
 * between barriers): [0] per-frame prologue, [1] check phase, [2] bit phase,
 * [3] syndrome test, [4] frame fetch + outputs, [5] / [6] the table-driven
 * first / second check phases of the QKD path. Synchronises the device. No
 * reference counterpart (the reference prints TRACE_* arrays instead,
 * qkd_ldpc_algorithm.cpp:42-155). */
QKD_API qkd_status qkd_debug_phase_cycles(qkd_workspace *ws, uint64_t *cycles7);
/* Decoder-kernel timing (the measurement's live roofline figure): start != 0
 * turns it on for `ws` (zeroed): every later decoder launch on ws is bracketed
 * by two HIP events on its stream, so only the decode kernel is timed (not the
 * packing, frame-syndrome or key-compare kernels around it). start == 0
 * synchronises those events, returns the summed kernel milliseconds and the
 * number of launches, and turns timing off. No reference counterpart. */
QKD_API qkd_status qkd_debug_decoder_timing(qkd_workspace *ws, int start, double *ms_total, uint64_t *launches);
/* Frames of the QKD path (qkd_qkd_ldpc_batch / qkd_trials_batch, binary64
 * rule, clamp on) whose speculative interval iterations could not certify a
 * hard decision (or reached the cap) and were decoded again with the exact
 * iterations, accumulated over the launches on `ws` since the last reset;
 * reset != 0 zeroes the count. The QKD_SPEC_CAP option (qkd_debug_set_option)
 * sets how many interval iterations a frame may run first (0: off; default 8).
 * Outputs never depend on it. No reference counterpart. */
QKD_API qkd_status qkd_debug_spec_replays(qkd_workspace *ws, uint64_t *replays, int reset);
/* The check-phase form the last split-decoder launch on `ws` ran with: *form
 * is QKD_CHECK_LANES as applied (0 where the launch's kernel has no check-lane
 * phases, whatever the option says; -1 before any launch), *lane_tasks the
 * 64-check tasks it ran one check per lane, *edge_tasks the tasks of its
 * edge-lane plan (the remainder's, or the whole plan's with form 0). Any
 * pointer may be NULL. No reference counterpart. */
QKD_API qkd_status qkd_debug_check_lanes(qkd_workspace *ws, int32_t *form, int32_t *lane_tasks, int32_t *edge_tasks);
/* Trace of one frame, the reference's TRACE_SUM_PRODUCT / TRACE_SUM_PRODUCT_LLR
 * (qkd_ldpc_algorithm.cpp:212-330): decodes llr[N] / syndrome[M] (host arrays)
 * with the reference rule (QKD_VARIANT_SP_F64 only) and records, for every
 * executed iteration t < *iterations, the messages the reference prints:
 *   c2b_trace[t*E + e]   "E:" check-to-bit messages after the clamp, in the
 *                        reference's check_to_bit_msg order (bit by bit, each
 *                        bit's checks ascending; bit_ptr of get_adjacency)
 *   total_trace[t*N + i] "L:" bit totals
 * (host arrays of max_iterations*E / *N, either may be NULL). "z:", "s:",
 * "M:" and MAX_LLR follow from these exactly (qkd_ldpc_amd.trace_decode). */
QKD_API qkd_status qkd_trace_decode(const qkd_code *code, const double *llr, const uint8_t *syndrome,
                                    uint32_t max_iterations, double msg_threshold, uint32_t flags,
                                    double *c2b_trace, double *total_trace, uint32_t *iterations,
                                    uint8_t *syndrome_match);
/* The decoder's tanh (which = 0) / atanh (which = 1) restatement applied to
 * x[n] -> y[n] (device arrays): the bit-exactness check of the device build
 * against glibc (reference qkd_ldpc_algorithm.cpp:224, :241). which = 2 / 3:
 * the binary32 variant's two transcendental steps (QKD_VARIANT_SP_F32): the
 * published sign(x) * phi(|x|) / ln 2 and phi(S ln 2) of a psi-unit sum S, x
 * rounded to binary32, result widened. which = 4 / 5: certified bounds of
 * phi(x) = -ln tanh(x/2) over [x[2k], x[2k+1]] (the speculative iterations'
 * input / output forms, qkd_spec.h) -> y[2k] = lower, y[2k+1] = upper; n even;
 * which = 5 takes its interval in log2-domain units (x = S / ln 2).
 * which = 8 / 9: quadruples (a, b, s_lo, s_hi) -> raw binary32 (in lo, in hi,
 * out lo, out hi) of the packed phi_pair (8) and of the scalar phi_bounds +
 * phi_bounds_out it must equal bit for bit (9); n a multiple of 4.
 * which = 10 / 11: pairs of exact b2c -> the raw bits of their psi bounds
 * (two binary32 per output double) from the packed psi_of_exact2 (10) and
 * the scalar psi_of_exact (11); n even.
 * which = 12 / 13: pairs (x, S) -> (|sign(x) phi(|x|) / ln 2|, phi(S ln 2))
 * of the binary32 variant, from its packed evaluation (12) and from the
 * scalar forms of which = 2 / 3 (13), which must agree bit for bit; n even.
 * which = 14 / 15: quadruples (a lo, a hi, b lo, b hi) -> the input-form phi
 * bounds of both intervals from the packed phi_bounds2 (14, the interleaved
 * decoder's) and two scalar phi_bounds (15); which = 16 / 17 the same for the
 * output form, phi_bounds_out2 (16) and phi_bounds_out (17); n % 4 == 0. */
QKD_API qkd_status qkd_debug_math(int which, const double *x, double *y, size_t n, void *stream);
/* Exhaustive check of the speculative iterations' phi bounds (qkd_spec.h) at
 * EVERY binary32 a with bit pattern in [first_bits, last_bits] (positive
 * finite): which = 4 the input form phi_bounds (a in nep units, psi result),
 * which = 5 the output form phi_bounds_out (a in log2-domain units, S = a ln 2),
 * both at the degenerate interval [a, a], against a binary64 phi on the
 * device. result[8] (host): [0] points, [1] upper bound below phi(a),
 * [2] lower bound above phi(a), [3] slope bound (with half its 2^-20 margin)
 * below |phi'(a)|, [4] max |eval/phi - 1| / 2^-20 (binary32 bits), [5] max
 * |phi'| / slope bound (binary32 bits), [6] / [7] bit patterns where [4] / [5]
 * peak (either of the tied points); [4]-[7] over normal a with a finite
 * evaluation only (a subnormal argument overflows the reciprocal: infinite
 * upper bound, zero lower bound; the kernel never feeds such an argument to
 * the output form, whose sums are at least phi(80) / ln 2). Synchronous. Test infrastructure: no
 * reference counterpart (the reference has no speculative iterations). */
QKD_API qkd_status qkd_debug_phi_sweep(int which, uint32_t first_bits, uint32_t last_bits, uint64_t *result);

/* The split decoder's internal bit order of a code given as a check-side CSR
 * (as qkd_code_create), computed on the host without a device: perm_out[q]
 * (n_bits entries) = the original bit at internal position q; plan_out
 * (optional, 64 * n_tasks entries, n_tasks from *n_tasks_out when plan_out is
 * null) = the check-phase wave plan's first words (bit | row << 24, idle lanes
 * bit = n_bits); mode: NULL for the shipped order, "runs" without its LDS bank
 * pass, "identity". Test infrastructure (tests/test_bit_order.py, CPU); no
 * reference counterpart. */
QKD_API qkd_status qkd_debug_bit_order(int32_t n_bits, int32_t n_checks, const int32_t *check_ptr,
                                       const int32_t *check_idx, const char *mode, int32_t *perm_out,
                                       uint32_t *plan_out, int32_t *n_tasks_out);

/* ---- host helpers --------------------------------------------------------- */
/* seeds[k] = k-th raw xoshiro256++(simulation_seed) output (simulation.cpp:222-228). */
QKD_API qkd_status qkd_make_seeds(uint64_t simulation_seed, size_t count, uint64_t *seeds_host);
/* get_rate_based_QBER_range (simulation.cpp:48-70) for one table row:
 * writes min(capacity, steps) values, returns the step count in *count. */
QKD_API qkd_status qkd_qber_range(double begin, double end, double step, double *values_host,
                          size_t capacity, size_t *count);

#ifdef __cplusplus
}
#endif

#endif /* QKD_LDPC_H */
