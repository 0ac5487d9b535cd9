"""qkd_ldpc_amd — MI355X-native QKD LDPC sum-product decoding.

Python view of the C ABI (include/qkd_ldpc.h). It mirrors the reference's
hot-path interface (ColdCloudd/QKD_LDPC, src/qkd_ldpc_algorithm.hpp and
src/array_and_matrix_operations.hpp) with batched, device-resident arrays:

  reference (one frame, host int arrays)         here (F frames, torch tensors on the GPU)
  ---------------------------------------------  ------------------------------------------
  H_matrix + read_sparse_alist_matrix             HMatrix.from_alist(path)
  read_dense_matrix                               HMatrix.from_dense(path)
  calculate_syndrome_irregular/_regular           calculate_syndrome(H, bits)
  sum_product_decoding_irregular/_regular         sum_product_decoding(H, llr, syndrome, ...)
  QKD_LDPC_irregular/_regular                     qkd_ldpc(H, alice, bob, qber, ...)
  its decode step alone, Bob's side of a link      reconcile(H, bob, syndrome, qber, ...)
  (no counterpart) key verification tags            verify_tags(H, bits, ...), reconcile(..., alice_tags=)
  (no counterpart) privacy amplification            privacy_amplify(keys, out_bits, ..., keep=verified)
  (no counterpart) ... of blocks up to 2^27 bits     privacy_amplify_long(keys, out_bits, ..., scratch=)
  (no counterpart) ... of a block's verified frames  privacy_amplify_kept(frames, verified, out_bits, ...)
  (no counterpart) punctured / shortened frames     AdaptPlan, adapt_embed, adapt_extract,
                                                    reconcile_adaptive(H, plan, bob_payload, ...)
  (no counterpart) blind reconciliation             reconcile_blind(H, plan, bob_payload, ..., revealed=)
  generate_random_bit_array + introduce_errors    keygen(H, seeds, q_nominal, ...)
  run_trial over a batch + the batch reduction    run_trials(H, seeds, q_nominal, ...)
  seeds of QKD_LDPC_batch_simulation              make_seeds(simulation_seed, count)
  get_rate_based_QBER_range (one table row)       qber_range(begin, end, step)
  QKD_LDPC_interactive_simulation                 interactive_simulation(H, seed, qbers, ...)

Errors surface as QkdError (a RuntimeError, as the reference throws
std::runtime_error). Every call runs HIP kernels; nothing falls back to CPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from ._native import FLAG_THRESHOLD, QkdError

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

__all__ = [
    "HMatrix", "QkdError", "calculate_syndrome", "sum_product_decoding",
    "sum_product_decoding_irregular", "sum_product_decoding_regular", "qkd_ldpc",
    "QKD_LDPC_irregular", "QKD_LDPC_regular", "keygen", "run_trials", "make_seeds",
    "qber_range", "Workspace", "counters_to_stats", "decoder_flags", "trace_decode", "set_debug_option",
    "spec_replays", "check_lanes", "interactive_simulation", "reconcile", "ReconcileResult",
    "verify_key_words", "verify_expand_key", "verify_tags",
    "privacy_key_words", "privacy_expand_key", "privacy_amplify",
    "privacy_long_key_words", "privacy_long_expand_key", "privacy_long_scratch_bytes", "privacy_amplify_long",
    "privacy_kept_scratch_bytes", "privacy_amplify_kept",
    "AdaptPlan", "adapt_positions", "adapt_embed", "adapt_extract", "reconcile_adaptive",
    "reconcile_blind", "BlindResult",
]


def decoder_flags(threshold_enabled: bool = True, variant: str = "sp_f64",
                  minsum_scale: float | None = None, minsum_offset: float | None = None,
                  minsum_self_correct: bool = False, erasures: bool = False) -> int:
    """Flag word of the decode entry points: the reference's threshold switch
    (CFG.ENABLE_SUM_PRODUCT_MSG_LLR_THRESHOLD) and the check-node rule:
    "sp_f64" (the reference, bit-exact), "sp_f32" or "minsum" (build-defined
    binary32 variants; minsum_scale in (0, 1), a multiple of 1/256).
    erasures: QKD_FLAG_ERASURES, the binary64 rule extended to zero LLRs
    (sum_product_decoding only; the library rejects it with another variant)."""
    if variant not in N.VARIANTS:
        raise ValueError(f"unknown decoder variant {variant!r}; one of {sorted(N.VARIANTS)}")
    flags = (FLAG_THRESHOLD if threshold_enabled else 0) | N.VARIANTS[variant]
    if erasures:
        flags |= N.FLAG_ERASURES
    if minsum_scale is not None:
        if variant != "minsum":
            raise ValueError("minsum_scale applies to variant='minsum' only")
        q = round(minsum_scale * 256)
        if not (1 <= q <= 255) or q != minsum_scale * 256:
            raise ValueError("minsum_scale must be k/256 for k in 1..255")
        flags |= q << N.MINSUM_SCALE_SHIFT
    if minsum_offset is not None:
        if variant != "minsum":
            raise ValueError("minsum_offset applies to variant='minsum' only")
        q = round(minsum_offset * 64)
        if not (0 <= q <= 255) or q != minsum_offset * 64:
            raise ValueError("minsum_offset must be k/64 for k in 0..255")
        flags |= q << N.MINSUM_OFFSET_SHIFT
    if minsum_self_correct:
        if variant != "minsum":
            raise ValueError("minsum_self_correct applies to variant='minsum' only")
        flags |= N.MINSUM_SELF_CORRECT
    return flags


def _ptr(t) -> int | None:
    if t is None:
        return None
    return int(t.data_ptr())


def _stream(stream, device: int) -> int | None:
    """The launch stream: the caller's, else torch's current stream of the code's device
    (not of whatever device happens to be current)."""
    if stream is None:
        return int(torch.cuda.current_stream(device).cuda_stream)
    if isinstance(stream, int):
        return stream
    return int(stream.cuda_stream)


def _torch_stream(stream, device: int):
    """The launch stream of _stream(stream, device) as a torch stream, for a wrapper's own
    torch work (an int is a raw stream handle, 0 the null stream)."""
    if stream is None:
        return torch.cuda.current_stream(device)
    if isinstance(stream, int):
        return torch.cuda.ExternalStream(stream, device=device)
    return stream


def _need_cuda(t, dtype, name, H: "HMatrix | None" = None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise QkdError(N.ERR_INVALID_ARG, f"{name} must be a contiguous {dtype} CUDA tensor")
    if H is not None and t.device.index != H.device:
        raise QkdError(N.ERR_INVALID_ARG,
                       f"{name} is on {t.device}, the code lives on cuda:{H.device}")


def _frames(t, width: int, name: str, frames: int | None = None) -> int:
    """Frame count of a [F, width] tensor (a 1-D [width] tensor is one frame). The
    kernels read F * width elements, so a ragged or short buffer is an error, never
    a silent floor (the reference's arrays are exactly N or M long)."""
    if t.dim() == 1 and t.numel() == width:
        f = 1
    elif t.dim() == 2 and t.shape[1] == width:
        f = int(t.shape[0])
    else:
        raise QkdError(N.ERR_INVALID_ARG,
                       f"{name} must have shape [F, {width}], got {list(t.shape)}")
    if frames is not None and f != frames:
        raise QkdError(N.ERR_INVALID_ARG, f"{name} holds {f} frames, expected {frames}")
    return f


def _need_vec(t, dtype, count: int, name: str, H: "HMatrix"):
    _need_cuda(t, dtype, name, H)
    if t.numel() != count:
        raise QkdError(N.ERR_INVALID_ARG, f"{name} must hold {count} elements, got {t.numel()}")


class HMatrix:
    """The parity-check matrix (reference H_matrix, array_and_matrix_operations.hpp:16-27),
    uploaded once to one device and immutable afterwards."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)
        info = N.CodeInfo()
        N.check(N.lib().qkd_code_get_info(self._h, C.byref(info)))
        self.num_bit_nodes = info.n_bits
        self.num_check_nodes = info.n_checks
        self.n_edges = info.n_edges
        self.max_bit_nodes_weight = info.max_bit_degree
        self.max_check_nodes_weight = info.max_check_degree
        self.is_regular = bool(info.is_regular)
        self.device = info.device

    # --- constructors (reference readers) ----------------------------------
    @classmethod
    def _make(cls, fn, *args):
        st = C.c_int(0)
        h = fn(*args, C.byref(st))
        if not h:
            raise QkdError(st.value, N.last_error())
        return cls(h)

    @classmethod
    def from_alist(cls, path: str, device: int = 0, sort_rows: bool = False) -> "HMatrix":
        """read_sparse_alist_matrix. sort_rows: accept lines that are not ascending
        by sorting them (QKD_READ_SORT_ROWS) instead of rejecting the file."""
        return cls._make(N.lib().qkd_code_from_alist_ex, str(path).encode(), device,
                         N.READ_SORT_ROWS if sort_rows else 0)

    @classmethod
    def from_dense(cls, path: str, device: int = 0) -> "HMatrix":
        return cls._make(N.lib().qkd_code_from_dense, str(path).encode(), device)

    @classmethod
    def from_check_lists(cls, n_bits: int, check_ptr, check_idx, device: int = 0) -> "HMatrix":
        cp = np.ascontiguousarray(check_ptr, dtype=np.int32)
        ci = np.ascontiguousarray(check_idx, dtype=np.int32)
        return cls._make(N.lib().qkd_code_create, n_bits, cp.size - 1, cp.ctypes.data,
                         ci.ctypes.data, device)

    @classmethod
    def from_dense_array(cls, dense, device: int = 0) -> "HMatrix":
        d = np.asarray(dense)
        ptr, idx = [0], []
        for row in d:
            idx.extend(np.nonzero(row)[0].tolist())
            ptr.append(len(idx))
        return cls.from_check_lists(d.shape[1], ptr, idx, device)

    # --- adjacency ------------------------------------------------------------
    def adjacency(self):
        n, m, e = self.num_bit_nodes, self.num_check_nodes, self.n_edges
        cp = np.zeros(m + 1, np.int32)
        ci = np.zeros(e, np.int32)
        bp = np.zeros(n + 1, np.int32)
        bi = np.zeros(e, np.int32)
        N.check(N.lib().qkd_code_get_adjacency(self._h, cp.ctypes.data, ci.ctypes.data,
                                               bp.ctypes.data, bi.ctypes.data))
        return cp, ci, bp, bi

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            N.lib().qkd_code_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Workspace:
    """Device scratch for one stream (qkd_workspace)."""

    def __init__(self, H: HMatrix):
        st = C.c_int(0)
        h = N.lib().qkd_workspace_create(H.handle, C.byref(st))
        if not h:
            raise QkdError(st.value, N.last_error())
        self._h = C.c_void_p(h)

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            N.lib().qkd_workspace_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ws(ws):
    return ws.handle if ws is not None else None


def set_debug_option(name: str, value=None, workspace: "Workspace | None" = None) -> None:
    """qkd_debug_set_option: a debug / A-B option (include/qkd_ldpc.h lists
    them) for `workspace`, or process-wide when None; value None restores the
    default (the product behaviour). The library reads no environment variable."""
    v = None if value is None else str(value).encode()
    N.check(N.lib().qkd_debug_set_option(_ws(workspace), name.encode(), v))


def spec_replays(ws: Workspace, reset: bool = False) -> int:
    """Frames of the QKD path decoded on `ws` whose speculative interval
    iterations could not certify every hard decision and were decoded again
    exactly (qkd_debug_spec_replays); outputs never depend on it."""
    v = C.c_uint64(0)
    N.check(N.lib().qkd_debug_spec_replays(ws.handle, C.byref(v), int(reset)))
    return int(v.value)


def check_lanes(ws: Workspace):
    """(form, lane_tasks, edge_tasks) of the last split-decoder launch on `ws`
    (qkd_debug_check_lanes): QKD_CHECK_LANES as applied, the tasks run one check
    per lane and the tasks of the edge-lane plan; form -1 before any launch."""
    v = [C.c_int32(0) for _ in range(3)]
    N.check(N.lib().qkd_debug_check_lanes(ws.handle, *[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def calculate_syndrome(H: HMatrix, bits, stream=None):
    """calculate_syndrome_irregular/_regular: bits [F, N] uint8 -> [F, M] uint8."""
    _need_cuda(bits, torch.uint8, "bits", H)
    f = _frames(bits, H.num_bit_nodes, "bits")
    out = torch.empty((f, H.num_check_nodes), dtype=torch.uint8, device=bits.device)
    N.check(N.lib().qkd_syndrome_batch(H.handle, _ptr(bits), f, _ptr(out), _stream(stream, H.device)))
    return out


@dataclass
class SPResult:
    """SP_result (qkd_ldpc_algorithm.hpp:14-18), one entry per frame."""
    iterations: "torch.Tensor"
    syndromes_match: "torch.Tensor"
    bits: "torch.Tensor | None"


@dataclass
class LDPCResult:
    """LDPC_result (qkd_ldpc_algorithm.hpp:20-24), one entry per frame."""
    iterations: "torch.Tensor"
    syndromes_match: "torch.Tensor"
    keys_match: "torch.Tensor"
    bits: "torch.Tensor | None"


def sum_product_decoding(H: HMatrix, llr, syndrome, max_iterations: int = 50,
                         msg_threshold: float = 100.0, threshold_enabled: bool = True,
                         want_bits: bool = True, workspace=None, stream=None,
                         variant: str = "sp_f64", minsum_scale: float | None = None,
                         minsum_offset: float | None = None, minsum_self_correct: bool = False,
                         erasures: bool = False) -> SPResult:
    """sum_product_decoding_irregular/_regular (qkd_ldpc_algorithm.cpp:3-345), batched.
    llr [F, N] float64, syndrome [F, M] uint8 (0/1). erasures: the check rule defined
    at zero LLRs (QKD_FLAG_ERASURES; variant "sp_f64" only), for punctured bits."""
    _need_cuda(llr, torch.float64, "llr", H)
    _need_cuda(syndrome, torch.uint8, "syndrome", H)
    f = _frames(llr, H.num_bit_nodes, "llr")
    _frames(syndrome, H.num_check_nodes, "syndrome", f)
    dev = llr.device
    bits = torch.empty((f, H.num_bit_nodes), dtype=torch.uint8, device=dev) if want_bits else None
    iters = torch.empty(f, dtype=torch.int32, device=dev)
    ok = torch.empty(f, dtype=torch.uint8, device=dev)
    flags = decoder_flags(threshold_enabled, variant, minsum_scale, minsum_offset, minsum_self_correct,
                          erasures)
    N.check(N.lib().qkd_decode_batch(H.handle, _ws(workspace), _ptr(llr), _ptr(syndrome), f,
                                     max_iterations, msg_threshold, flags, _ptr(bits), _ptr(iters),
                                     _ptr(ok), _stream(stream, H.device)))
    return SPResult(iters, ok, bits)


# The reference has two twins that differ only in loop bounds; one kernel serves both.
sum_product_decoding_irregular = sum_product_decoding
sum_product_decoding_regular = sum_product_decoding


def qkd_ldpc(H: HMatrix, alice, bob, qber: float, max_iterations: int = 50,
             msg_threshold: float = 100.0, threshold_enabled: bool = True,
             want_bits: bool = False, workspace=None, stream=None,
             variant: str = "sp_f64", minsum_scale: float | None = None,
             minsum_offset: float | None = None, minsum_self_correct: bool = False) -> LDPCResult:
    """QKD_LDPC_irregular/_regular (qkd_ldpc_algorithm.cpp:347-447), batched.
    alice, bob [F, N] uint8 (0/1); one QBER for the batch."""
    _need_cuda(alice, torch.uint8, "alice", H)
    _need_cuda(bob, torch.uint8, "bob", H)
    f = _frames(alice, H.num_bit_nodes, "alice")
    _frames(bob, H.num_bit_nodes, "bob", f)
    dev = alice.device
    bits = torch.empty((f, H.num_bit_nodes), dtype=torch.uint8, device=dev) if want_bits else None
    iters = torch.empty(f, dtype=torch.int32, device=dev)
    ok = torch.empty(f, dtype=torch.uint8, device=dev)
    km = torch.empty(f, dtype=torch.uint8, device=dev)
    flags = decoder_flags(threshold_enabled, variant, minsum_scale, minsum_offset, minsum_self_correct)
    N.check(N.lib().qkd_qkd_ldpc_batch(H.handle, _ws(workspace), _ptr(alice), _ptr(bob), f, qber,
                                       max_iterations, msg_threshold, flags, _ptr(bits),
                                       _ptr(iters), _ptr(ok), _ptr(km), _stream(stream, H.device)))
    return LDPCResult(iters, ok, km, bits)


QKD_LDPC_irregular = qkd_ldpc
QKD_LDPC_regular = qkd_ldpc


@dataclass
class ReconcileResult:
    """Bob's view of one reconciliation, one entry per frame: SP_result
    (qkd_ldpc_algorithm.hpp:14-18) with the decoded key and the number of bits
    the decoder changed in Bob's key (None when not asked for)."""
    iterations: "torch.Tensor"
    syndromes_match: "torch.Tensor"
    bits: "torch.Tensor"
    corrected: "torch.Tensor | None"
    # key verification (reconcile with any of its hash arguments): the corrected keys'
    # tags (int64 bit patterns) and syndromes_match & (tag == Alice's tag)
    tags: "torch.Tensor | None" = None
    verified: "torch.Tensor | None" = None
    # reconcile_adaptive with want_frames: the whole N-bit decisions (bits is the payload)
    frames: "torch.Tensor | None" = None


def reconcile(H: HMatrix, bob, syndrome, qber: float, max_iterations: int = 50,
              msg_threshold: float = 100.0, threshold_enabled: bool = True,
              want_corrected: bool = True, workspace=None, stream=None,
              variant: str = "sp_f64", minsum_scale: float | None = None,
              minsum_offset: float | None = None, minsum_self_correct: bool = False,
              hash_seed: int | None = None, hash_words=None, tag_bits: int = 64, alice_tags=None,
              want_tags: bool = False) -> ReconcileResult:
    """Bob's side of one-way reconciliation (qkd_reconcile_batch): the decode step of
    QKD_LDPC_irregular/_regular (qkd_ldpc_algorithm.cpp:398-431) with the target syndrome
    received from Alice (her half is calculate_syndrome on her key) instead of computed
    from her key. bob [F, N] uint8 (0/1), syndrome [F, M] uint8 (nonzero = 1); one QBER
    for the batch. bits: the last hard decision; corrected: popcount(bits ^ bob).

    Key verification (qkd_reconcile_verify_batch), with any of hash_seed, hash_words,
    alice_tags, want_tags given: tags = verify_tags of the corrected keys, from the kernel
    that writes them; with alice_tags [F] (Alice's verify_tags under the same hash),
    verified = syndromes_match & (tag == alice_tags) over the low tag_bits bits. Every
    other field is what the call without them returns."""
    _need_cuda(bob, torch.uint8, "bob", H)
    _need_cuda(syndrome, torch.uint8, "syndrome", H)
    f = _frames(bob, H.num_bit_nodes, "bob")
    _frames(syndrome, H.num_check_nodes, "syndrome", f)
    dev = bob.device
    bits = torch.empty((f, H.num_bit_nodes), dtype=torch.uint8, device=dev)
    iters = torch.empty(f, dtype=torch.int32, device=dev)
    ok = torch.empty(f, dtype=torch.uint8, device=dev)
    corrected = torch.empty(f, dtype=torch.int32, device=dev) if want_corrected else None
    flags = decoder_flags(threshold_enabled, variant, minsum_scale, minsum_offset, minsum_self_correct)
    if hash_seed is not None or hash_words is not None or alice_tags is not None or want_tags:
        seed, words = _verify_key(H, hash_seed, hash_words)
        if alice_tags is not None:
            _need_tags(alice_tags, f, "alice_tags", H)
        # (the tags are returned whenever verification runs: 8 bytes a frame)
        tags = torch.empty(f, dtype=torch.int64, device=dev)
        verified = torch.empty(f, dtype=torch.uint8, device=dev) if alice_tags is not None else None
        N.check(N.lib().qkd_reconcile_verify_batch(
            H.handle, _ws(workspace), _ptr(bob), _ptr(syndrome), f, qber, max_iterations, msg_threshold, flags,
            _ptr(bits), _ptr(iters), _ptr(ok), _ptr(corrected), seed, _ptr(words), tag_bits, _ptr(alice_tags),
            _ptr(tags), _ptr(verified), _stream(stream, H.device)))
        return ReconcileResult(iters, ok, bits, corrected, tags, verified)
    N.check(N.lib().qkd_reconcile_batch(H.handle, _ws(workspace), _ptr(bob), _ptr(syndrome), f, qber,
                                        max_iterations, msg_threshold, flags, _ptr(bits), _ptr(iters),
                                        _ptr(ok), _ptr(corrected), _stream(stream, H.device)))
    return ReconcileResult(iters, ok, bits, corrected)


def verify_key_words(n_bits: int) -> int:
    """W = ceil((N + 63) / 64): the 64-bit words of the verification hash's key string
    for an N-bit key (qkd_verify_key_words)."""
    return int(N.lib().qkd_verify_key_words(n_bits))


def verify_expand_key(hash_seed: int, n_bits: int) -> np.ndarray:
    """The W words the seeded form of the hash uses (qkd_verify_expand_key; SplitMix64 in
    counter form), as a numpy uint64 array: to inspect, or to upload as hash_words."""
    out = np.zeros(max(verify_key_words(n_bits), 1), np.uint64)
    N.check(N.lib().qkd_verify_expand_key(hash_seed & (2**64 - 1), n_bits, out.ctypes.data))
    return out[:verify_key_words(n_bits)]


def _tag_dtypes():
    return tuple(d for d in (torch.int64, getattr(torch, "uint64", None)) if d is not None)


def _need_tags(t, count: int, name: str, H: HMatrix):
    """A contiguous device tensor of count 64-bit words (int64 bit patterns or uint64)."""
    if not (isinstance(t, torch.Tensor) and t.dtype in _tag_dtypes()):
        raise QkdError(N.ERR_INVALID_ARG, f"{name} must be a contiguous int64 or uint64 CUDA tensor")
    _need_vec(t, t.dtype, count, name, H)


def _verify_width(H) -> int:
    """The key width the verification hash runs over: N of an HMatrix, n_payload of an
    AdaptPlan."""
    return H.n_payload if hasattr(H, "n_payload") else H.num_bit_nodes


def _verify_key(H, hash_seed, hash_words):
    """(seed, words) of the hash's key string: the caller's device words, or the seed.
    H: an HMatrix, or an AdaptPlan (the string is then sized from n_payload)."""
    if hash_words is not None:
        _need_tags(hash_words, verify_key_words(_verify_width(H)), "hash_words", H)
    return (0 if hash_seed is None else int(hash_seed)) & (2**64 - 1), hash_words


def verify_tags(H, bits, hash_seed: int = 0, hash_words=None, tag_bits: int = 64, stream=None):
    """Key verification tags of byte keys (qkd_verify_tags_batch), Alice's half of the
    check that follows error correction: tags[f] = the Hankel-matrix universal hash of
    bits[f] ([F, N] uint8, a key bit is byte & 1), low tag_bits bits, as int64 bit
    patterns. The key string is hash_words (verify_key_words(N) 64-bit words on the
    device, truly random: the 2^-tag_bits universal form) or, without them, expanded from
    hash_seed (a computational stand-in). A tag discloses tag_bits bits of the key.

    With an AdaptPlan in H's place (qkd_adapt_verify_tags_batch): the tags of payloads
    [F, n_payload], positions being payload indices and N above n_payload; what
    reconcile_adaptive and reconcile_blind compare with as alice_tags."""
    width = _verify_width(H)
    _need_cuda(bits, torch.uint8, "bits", H)
    f = _frames(bits, width, "bits")
    seed, words = _verify_key(H, hash_seed, hash_words)
    tags = torch.empty(f, dtype=torch.int64, device=bits.device)
    entry = N.lib().qkd_adapt_verify_tags_batch if hasattr(H, "n_payload") else N.lib().qkd_verify_tags_batch
    N.check(entry(H.handle, _ptr(bits), f, seed, _ptr(words), tag_bits, _ptr(tags), _stream(stream, H.device)))
    return tags


def _csr(H):
    """(n, m, check_ptr, check_idx) of an HMatrix, or of a (n_bits, check_ptr, check_idx)
    tuple: the host helpers need no device."""
    if isinstance(H, HMatrix):
        cp, ci, _, _ = H.adjacency()
        return H.num_bit_nodes, H.num_check_nodes, cp, ci
    n, cp, ci = H
    cp = np.ascontiguousarray(cp, dtype=np.int32)
    ci = np.ascontiguousarray(ci, dtype=np.int32)
    return int(n), cp.size - 1, cp, ci


def adapt_positions(H, count: int, seed: int):
    """qkd_adapt_positions: a deterministic "untainted" choice of `count` positions that
    Alice and Bob both compute from a shared seed (a seeded Fisher-Yates order; first the
    candidates none of whose checks touches an earlier pick, then the rest). H: an HMatrix,
    or (n_bits, check_ptr, check_idx) on a machine without a device. Returns (positions
    int32 numpy array in the order taken, untainted count)."""
    n, m, cp, ci = _csr(H)
    out = np.zeros(max(int(count), 1), np.int32)
    unt = C.c_int32(0)
    N.check(N.lib().qkd_adapt_positions(n, m, cp.ctypes.data, ci.ctypes.data, int(count),
                                        int(seed) & (2**64 - 1), out.ctypes.data, C.byref(unt)))
    return out[:int(count)], int(unt.value)


class AdaptPlan:
    """A rate-adaptation plan of one code (qkd_adapt): `punctured` positions hold Alice's
    private random bits (Bob's LLR 0), `shortened` positions hold 0 on both sides (Bob's
    LLR +known_llr); payload bit k lives at the k-th other position, ascending. Uploaded
    once, immutable; close it before its HMatrix."""

    def __init__(self, H: HMatrix, punctured=(), shortened=()):
        pu = np.ascontiguousarray(punctured, dtype=np.int32).reshape(-1)
        sh = np.ascontiguousarray(shortened, dtype=np.int32).reshape(-1)
        st = C.c_int(0)
        h = N.lib().qkd_adapt_create(H.handle, pu.ctypes.data if pu.size else None, pu.size,
                                     sh.ctypes.data if sh.size else None, sh.size, C.byref(st))
        if not h:
            raise QkdError(st.value, N.last_error())
        self._h = C.c_void_p(h)
        self._H = H            # (the plan points into its code)
        info = N.AdaptInfo()
        N.check(N.lib().qkd_adapt_get_info(self._h, C.byref(info)))
        self.n_bits = info.n_bits
        self.n_payload = info.n_payload
        self.n_punctured = info.n_punctured
        self.n_shortened = info.n_shortened
        self.device = H.device
        self.punctured = pu.copy()
        self.shortened = sh.copy()

    @classmethod
    def choose(cls, H: HMatrix, count: int, p: int, seed: int) -> "AdaptPlan":
        """`count` positions from adapt_positions(H, count, seed): the first p punctured,
        the other count - p shortened."""
        if not 0 <= p <= count:
            raise QkdError(N.ERR_INVALID_ARG, f"p must be in 0..{count}")
        pos, _ = adapt_positions(H, count, seed)
        return cls(H, pos[:p], pos[p:])

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            N.lib().qkd_adapt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def adapt_embed(plan: AdaptPlan, payload, fill=None, stream=None):
    """qkd_adapt_embed_batch: payload [F, n_payload] uint8 (a bit is byte & 1) and, exactly
    when the plan punctures, fill [F, p] uint8 (Alice's private random bits, in the order
    of the plan's punctured list) -> frames [F, N] uint8; shortened positions are 0.
    Alice's half of the protocol is this followed by calculate_syndrome."""
    _need_cuda(payload, torch.uint8, "payload", plan)
    f = _frames(payload, plan.n_payload, "payload")
    if fill is not None:
        _need_cuda(fill, torch.uint8, "fill", plan)
        if plan.n_punctured == 0:
            raise QkdError(N.ERR_INVALID_ARG, "fill given for a plan without punctured positions")
        _frames(fill, plan.n_punctured, "fill", f)
    frames = torch.empty((f, plan.n_bits), dtype=torch.uint8, device=payload.device)
    N.check(N.lib().qkd_adapt_embed_batch(plan.handle, _ptr(payload), f, _ptr(fill), _ptr(frames),
                                          _stream(stream, plan.device)))
    return frames


def adapt_extract(plan: AdaptPlan, frames, stream=None):
    """qkd_adapt_extract_batch: frames [F, N] uint8 -> their payload [F, n_payload] (byte & 1)."""
    _need_cuda(frames, torch.uint8, "frames", plan)
    f = _frames(frames, plan.n_bits, "frames")
    out = torch.empty((f, plan.n_payload), dtype=torch.uint8, device=frames.device)
    N.check(N.lib().qkd_adapt_extract_batch(plan.handle, _ptr(frames), f, _ptr(out),
                                            _stream(stream, plan.device)))
    return out


def reconcile_adaptive(H: HMatrix, plan: AdaptPlan, bob_payload, syndrome, qber: float,
                       known_llr: float = 100.0, max_iterations: int = 50, msg_threshold: float = 100.0,
                       threshold_enabled: bool = True, want_corrected: bool = True,
                       want_frames: bool = False, workspace=None, stream=None,
                       hash_seed: int | None = None, hash_words=None, tag_bits: int = 64, alice_tags=None,
                       want_tags: bool = False) -> ReconcileResult:
    """Bob's side with punctured and shortened frames (qkd_reconcile_adaptive_batch):
    bob_payload [F, n_payload] uint8, syndrome [F, M] uint8 of Alice's embedded frames. The
    decision equals sum_product_decoding(erasures=True) on the LLRs +-log((1-q)/q) at the
    payload positions, +0.0 at the punctured and +known_llr at the shortened ones, without
    that array ever existing. bits: the payload of the decision; corrected:
    popcount(bits ^ bob_payload); frames (want_frames): the whole N-bit decisions. The
    default known_llr is the default clamp, so a shortened bit publishes t = 1.0 exactly.

    Key verification (qkd_reconcile_adaptive_verify_batch), with any of hash_seed,
    hash_words, alice_tags, want_tags given, exactly as on reconcile: tags =
    verify_tags(plan, bits), taken by the decoder kernel as it writes the payload; with
    alice_tags [F] (Alice's verify_tags(plan, payload) under the same hash), verified =
    syndromes_match & (tag == alice_tags) over the low tag_bits bits. Every other field is
    what the call without them returns."""
    _need_cuda(bob_payload, torch.uint8, "bob_payload", H)
    _need_cuda(syndrome, torch.uint8, "syndrome", H)
    f = _frames(bob_payload, plan.n_payload, "bob_payload")
    _frames(syndrome, H.num_check_nodes, "syndrome", f)
    dev = bob_payload.device
    bits = torch.empty((f, plan.n_payload), dtype=torch.uint8, device=dev)
    frames = torch.empty((f, H.num_bit_nodes), dtype=torch.uint8, device=dev) if want_frames else None
    iters = torch.empty(f, dtype=torch.int32, device=dev)
    ok = torch.empty(f, dtype=torch.uint8, device=dev)
    corrected = torch.empty(f, dtype=torch.int32, device=dev) if want_corrected else None
    flags = decoder_flags(threshold_enabled, "sp_f64")
    if hash_seed is not None or hash_words is not None or alice_tags is not None or want_tags:
        seed, words = _verify_key(plan, hash_seed, hash_words)
        if alice_tags is not None:
            _need_tags(alice_tags, f, "alice_tags", H)
        tags = torch.empty(f, dtype=torch.int64, device=dev)
        verified = torch.empty(f, dtype=torch.uint8, device=dev) if alice_tags is not None else None
        N.check(N.lib().qkd_reconcile_adaptive_verify_batch(
            H.handle, _ws(workspace), plan.handle, _ptr(bob_payload), _ptr(syndrome), f, qber, known_llr,
            max_iterations, msg_threshold, flags, _ptr(bits), _ptr(frames), _ptr(iters), _ptr(ok), _ptr(corrected),
            seed, _ptr(words), tag_bits, _ptr(alice_tags), _ptr(tags), _ptr(verified), _stream(stream, H.device)))
        return ReconcileResult(iters, ok, bits, corrected, tags, verified, frames=frames)
    N.check(N.lib().qkd_reconcile_adaptive_batch(
        H.handle, _ws(workspace), plan.handle, _ptr(bob_payload), _ptr(syndrome), f, qber, known_llr,
        max_iterations, msg_threshold, flags, _ptr(bits), _ptr(frames), _ptr(iters), _ptr(ok), _ptr(corrected),
        _stream(stream, H.device)))
    return ReconcileResult(iters, ok, bits, corrected, frames=frames)


@dataclass
class BlindResult(ReconcileResult):
    """reconcile_blind's view of its frames: ReconcileResult's fields (a skipped frame's
    entries are left as allocated, never written), rounds (how many rounds decoded the
    frame), n_revealed (the revealed-bit count its last decode used) and leak_bits =
    M - p + n_revealed, the key bits the exchange disclosed for that frame, which the
    caller takes off in privacy amplification (all int32, on the device). A verified link
    (alice_tags) additionally discloses tag_bits bits per frame, once; leak_bits does not
    include them."""
    rounds: "torch.Tensor | None" = None
    n_revealed: "torch.Tensor | None" = None
    leak_bits: "torch.Tensor | None" = None


def reconcile_blind(H: HMatrix, plan: AdaptPlan, bob_payload, syndrome, qber: float,
                    revealed=None, n_revealed=None, skip=None, step: int = 0, max_rounds: int = 1,
                    known_llr: float = 100.0, max_iterations: int = 50, msg_threshold: float = 100.0,
                    threshold_enabled: bool = True, want_corrected: bool = True,
                    want_frames: bool = False, workspace=None, stream=None,
                    hash_seed: int | None = None, hash_words=None, tag_bits: int = 64, alice_tags=None,
                    want_tags: bool = False) -> BlindResult:
    """Blind reconciliation, Bob's side (qkd_reconcile_blind_batch): reconcile_adaptive
    made interactive. revealed [F, p] uint8: the values (byte & 1) of the punctured bits in
    the order of the plan's punctured list, i.e. Alice's fill, of which frame f holds the
    first n_revealed[f] ([F] int32; missing: zeros; the caller's tensor is not modified);
    those positions are known bits (LLR -+known_llr) instead of erasures, and no later byte
    of `revealed` is read. skip [F] uint8: nonzero = the frame is left alone, outputs
    included. In each of max_rounds rounds every open frame is decoded; one that matched is
    closed, as is one with nothing left to reveal; any other gets `step` more bits for the
    next round. max_rounds = 1 is Bob's step on a link (he then asks Alice for more and
    calls again with skip set for the finished frames); max_rounds > 1 wants Alice's whole
    fill and runs the rounds on the device without a trip to the host. With no reveals, no
    skip and one round the result is reconcile_adaptive's.

    The counts are uint32 in the library and a count past p counts as p, so a negative
    int32 count means "everything revealed" (it cannot be rejected without a
    synchronisation). With stream= given, the copy of n_revealed and leak_bits are made on
    that stream too, after whatever it already holds: the inputs must be ready there, and
    the result is ready once that stream is.

    Key verification (qkd_reconcile_blind_verify_batch), with any of hash_seed, hash_words,
    alice_tags, want_tags given, exactly as on reconcile: tags and verified of each frame's
    last decode. With alice_tags (Alice's verify_tags(plan, payload), announced with the
    syndrome) "matched" above reads "verified": a frame whose syndrome matches under a
    wrong tag is treated like a failed one, revealed more bits and decoded again, and on a
    link Bob sets skip from verified. With want_tags alone, closing stays on
    syndromes_match."""
    _need_cuda(bob_payload, torch.uint8, "bob_payload", H)
    _need_cuda(syndrome, torch.uint8, "syndrome", H)
    f = _frames(bob_payload, plan.n_payload, "bob_payload")
    _frames(syndrome, H.num_check_nodes, "syndrome", f)
    p = plan.n_punctured
    if revealed is not None:
        _need_cuda(revealed, torch.uint8, "revealed", H)
        if p == 0:
            raise QkdError(N.ERR_INVALID_ARG, "revealed given for a plan without punctured positions")
        _frames(revealed, p, "revealed", f)
    elif p > 0:
        raise QkdError(N.ERR_INVALID_ARG, "revealed is required when the plan punctures")
    dev = bob_payload.device
    if n_revealed is not None:
        _need_vec(n_revealed, torch.int32, f, "n_revealed", H)
    if skip is not None:
        _need_vec(skip, torch.uint8, f, "skip", H)
    if not (isinstance(max_rounds, int) and 1 <= max_rounds < 2**32):
        raise QkdError(N.ERR_INVALID_ARG, "max_rounds must be >= 1")
    if not (isinstance(step, int) and 0 <= step < 2**32) or (max_rounds > 1 and step < 1):
        raise QkdError(N.ERR_INVALID_ARG, "step must be >= 1 when max_rounds > 1")
    bits = torch.empty((f, plan.n_payload), dtype=torch.uint8, device=dev)
    frames = torch.empty((f, H.num_bit_nodes), dtype=torch.uint8, device=dev) if want_frames else None
    iters = torch.empty(f, dtype=torch.int32, device=dev)
    ok = torch.empty(f, dtype=torch.uint8, device=dev)
    corrected = torch.empty(f, dtype=torch.int32, device=dev) if want_corrected else None
    rounds = torch.empty(f, dtype=torch.int32, device=dev)
    flags = decoder_flags(threshold_enabled, "sp_f64")
    verify = hash_seed is not None or hash_words is not None or alice_tags is not None or want_tags
    tags = verified = None
    if verify:
        seed, words = _verify_key(plan, hash_seed, hash_words)
        if alice_tags is not None:
            _need_tags(alice_tags, f, "alice_tags", H)
        tags = torch.empty(f, dtype=torch.int64, device=dev)
        verified = torch.empty(f, dtype=torch.uint8, device=dev) if alice_tags is not None else None
    # The copy of the counts before the call and leak_bits after it are torch work of this
    # wrapper: they go on the launch stream, where the kernels that read and advance the
    # counts run, not on whatever stream is current.
    with torch.cuda.stream(_torch_stream(stream, H.device)):
        nrev = torch.zeros(f, dtype=torch.int32, device=dev) if n_revealed is None else n_revealed.clone()
        if verify:
            N.check(N.lib().qkd_reconcile_blind_verify_batch(
                H.handle, _ws(workspace), plan.handle, _ptr(bob_payload), _ptr(syndrome), f, qber, known_llr,
                max_iterations, msg_threshold, flags, _ptr(revealed), _ptr(nrev), _ptr(skip), step, max_rounds,
                _ptr(bits), _ptr(frames), _ptr(iters), _ptr(ok), _ptr(corrected), _ptr(rounds),
                seed, _ptr(words), tag_bits, _ptr(alice_tags), _ptr(tags), _ptr(verified),
                _stream(stream, H.device)))
        else:
            N.check(N.lib().qkd_reconcile_blind_batch(
                H.handle, _ws(workspace), plan.handle, _ptr(bob_payload), _ptr(syndrome), f, qber, known_llr,
                max_iterations, msg_threshold, flags, _ptr(revealed), _ptr(nrev), _ptr(skip), step, max_rounds,
                _ptr(bits), _ptr(frames), _ptr(iters), _ptr(ok), _ptr(corrected), _ptr(rounds),
                _stream(stream, H.device)))
        leak = nrev + (H.num_check_nodes - p)
    return BlindResult(iters, ok, bits, corrected, tags, verified, frames=frames, rounds=rounds, n_revealed=nrev,
                       leak_bits=leak)


class _Device:
    """What _need_cuda asks of an HMatrix, for entries that take a device and no code."""

    def __init__(self, index: int):
        self.device = index


def privacy_key_words(n_in: int, out_bits: int) -> int:
    """Wp = ceil((n_in + out_bits - 1) / 64): the 64-bit words of the privacy amplification
    hash's key string (qkd_privacy_key_words); 0 unless 1 <= out_bits <= n_in <= 2^20."""
    if not (0 <= n_in < 2**32 and 0 <= out_bits < 2**32):
        return 0
    return int(N.lib().qkd_privacy_key_words(n_in, out_bits))


def privacy_expand_key(hash_seed: int, n_in: int, out_bits: int) -> np.ndarray:
    """The Wp words the seeded form of the hash uses (qkd_privacy_expand_key), as a numpy
    uint64 array: to inspect, or to upload as hash_words."""
    w = privacy_key_words(n_in, out_bits)
    if w == 0:
        raise QkdError(N.ERR_INVALID_ARG, "need 1 <= out_bits <= n_in <= 2^20")
    out = np.zeros(w, np.uint64)
    N.check(N.lib().qkd_privacy_expand_key(hash_seed & (2**64 - 1), n_in, out_bits, out.ctypes.data))
    return out


def privacy_amplify(keys, out_bits: int, hash_seed: int = 0, hash_words=None, keep=None, stream=None):
    """Privacy amplification (qkd_privacy_amplify_batch): keys [F, n_in] uint8 on the GPU
    (a key bit is byte & 1) hashed to out_bits bits each with the Hankel matrix of the key
    string, out_i = XOR_p r[p + i] x_p; returns [F, ceil(out_bits / 64)] int64 bit
    patterns, bit i of a frame in word i >> 6 at i & 63. The key string is hash_words
    (privacy_key_words(n_in, out_bits) 64-bit words on the device, truly random: the
    universal form) or, without them, expanded from hash_seed (a computational stand-in).
    It must be independent of the verification hash's string. keep ([F] uint8, typically
    ReconcileResult.verified): frames with 0 get all-zero words. To hash B corrected
    frames as one block, pass bits.view(F // B, B * N). Past n_in = 2^20 the call goes to
    privacy_amplify_long (the same bits by transforms; keep is then per block)."""
    _need_cuda(keys, torch.uint8, "keys")
    if keys.dim() != 2 or keys.shape[0] < 1 or keys.shape[1] < 1:
        raise QkdError(N.ERR_INVALID_ARG, f"keys must have shape [F, n_in], got {list(keys.shape)}")
    f, n_in = int(keys.shape[0]), int(keys.shape[1])
    if not isinstance(out_bits, int) or not 1 <= out_bits <= n_in:
        raise QkdError(N.ERR_INVALID_ARG, f"out_bits must be in 1..{n_in}")
    wp = privacy_key_words(n_in, out_bits)
    if wp == 0:            # n_in exceeds 2^20 bits: the long form's range
        return privacy_amplify_long(keys, out_bits, hash_seed, hash_words, keep, stream=stream)
    dev = _Device(keys.device.index)
    if hash_words is not None:
        _need_tags(hash_words, wp, "hash_words", dev)
    if keep is not None:
        _need_vec(keep, torch.uint8, f, "keep", dev)
    seed = (0 if hash_seed is None else int(hash_seed)) & (2**64 - 1)
    out = torch.empty(f, (out_bits + 63) // 64, dtype=torch.int64, device=keys.device)
    N.check(N.lib().qkd_privacy_amplify_batch(dev.device, _ptr(keys), f, n_in, out_bits, seed, _ptr(hash_words),
                                              _ptr(keep), _ptr(out), _stream(stream, dev.device)))
    return out


def privacy_long_key_words(n_in: int, out_bits: int) -> int:
    """Wp = ceil((n_in + out_bits - 1) / 64) over the long form's range
    (qkd_privacy_long_key_words); 0 unless 1 <= out_bits <= n_in and
    n_in + out_bits - 1 <= 2^27."""
    if not (0 <= n_in < 2**32 and 0 <= out_bits < 2**32):
        return 0
    return int(N.lib().qkd_privacy_long_key_words(n_in, out_bits))


def privacy_long_expand_key(hash_seed: int, n_in: int, out_bits: int) -> np.ndarray:
    """The Wp words the seeded form uses over the long form's range
    (qkd_privacy_long_expand_key), as a numpy uint64 array."""
    w = privacy_long_key_words(n_in, out_bits)
    if w == 0:
        raise QkdError(N.ERR_INVALID_ARG, "need 1 <= out_bits <= n_in and n_in + out_bits - 1 <= 2^27")
    out = np.zeros(w, np.uint64)
    N.check(N.lib().qkd_privacy_long_expand_key(hash_seed & (2**64 - 1), n_in, out_bits, out.ctypes.data))
    return out


def privacy_amplify_long(keys, out_bits: int, hash_seed: int = 0, hash_words=None, keep=None, scratch=None,
                         stream=None):
    """Long-block privacy amplification (qkd_privacy_amplify_long_batch): the hash of
    privacy_amplify, bit for bit, by number-theoretic transforms, for keys [B, n_in] uint8
    with 1 <= out_bits <= n_in and n_in + out_bits - 1 <= 2^27; returns
    [B, ceil(out_bits / 64)] int64 bit patterns. hash_words holds
    privacy_long_key_words(n_in, out_bits) words; the seeded string is a computational
    stand-in. keep ([B] uint8) is per block: a block with 0 gets all-zero words (to hash only
    the verified frames of a block, call privacy_amplify_kept, which compacts them on the
    device at the block's fixed length).
    scratch: a uint8 device tensor of at least privacy_long_scratch_bytes(n_in, out_bits)
    bytes (about 8 bytes per bit of the power of two at or above n_in + out_bits - 1), to
    reuse one allocation over calls; without it the wrapper allocates one for the call."""
    _need_cuda(keys, torch.uint8, "keys")
    if keys.dim() != 2 or keys.shape[0] < 1 or keys.shape[1] < 1:
        raise QkdError(N.ERR_INVALID_ARG, f"keys must have shape [B, n_in], got {list(keys.shape)}")
    f, n_in = int(keys.shape[0]), int(keys.shape[1])
    if not isinstance(out_bits, int) or not 1 <= out_bits <= n_in:
        raise QkdError(N.ERR_INVALID_ARG, f"out_bits must be in 1..{n_in}")
    wp = privacy_long_key_words(n_in, out_bits)
    if wp == 0:
        raise QkdError(N.ERR_INVALID_ARG, "n_in + out_bits - 1 exceeds 2^27 bits")
    dev = _Device(keys.device.index)
    if hash_words is not None:
        _need_tags(hash_words, wp, "hash_words", dev)
    if keep is not None:
        _need_vec(keep, torch.uint8, f, "keep", dev)
    need = privacy_long_scratch_bytes(n_in, out_bits)
    ts = _torch_stream(stream, dev.device)
    if scratch is None:
        # allocated under the launch stream, so that the allocator hands the memory on
        # only to work that stream orders after this call's kernels
        with torch.cuda.stream(ts):
            scratch = torch.empty(need, dtype=torch.uint8, device=keys.device)
    else:
        _need_cuda(scratch, torch.uint8, "scratch", dev)
    seed = (0 if hash_seed is None else int(hash_seed)) & (2**64 - 1)
    out = torch.empty(f, (out_bits + 63) // 64, dtype=torch.int64, device=keys.device)
    N.check(N.lib().qkd_privacy_amplify_long_batch(dev.device, _ptr(keys), f, n_in, out_bits, seed, _ptr(hash_words),
                                                   _ptr(keep), _ptr(out), _ptr(scratch), scratch.numel(),
                                                   int(ts.cuda_stream)))
    return out


def privacy_long_scratch_bytes(n_in: int, out_bits: int) -> int:
    """The bytes of scratch privacy_amplify_long needs (qkd_privacy_long_scratch_bytes);
    0 for sizes outside its range."""
    if not (0 <= n_in < 2**32 and 0 <= out_bits < 2**32):
        return 0
    return int(N.lib().qkd_privacy_long_scratch_bytes(n_in, out_bits))


def privacy_kept_scratch_bytes(frame_bits: int, frames_per_block: int, out_bits: int, n_blocks: int = 1) -> int:
    """The bytes of scratch privacy_amplify_kept needs (qkd_privacy_kept_scratch_bytes):
    privacy_long_scratch_bytes(frames_per_block * frame_bits, out_bits) plus a frame list of
    n_blocks * frames_per_block 32-bit entries, a byte per block and 16 bytes of slack, so
    that, unlike the long form's, it grows with n_blocks; 0 for sizes outside the range."""
    if not all(isinstance(v, int) and 0 <= v < 2**32 for v in (frame_bits, frames_per_block, out_bits)):
        return 0
    if not (isinstance(n_blocks, int) and 0 <= n_blocks < 2**64):
        return 0
    return int(N.lib().qkd_privacy_kept_scratch_bytes(frame_bits, frames_per_block, out_bits, n_blocks))


def privacy_amplify_kept(frames, keep, out_bits: int, frames_per_block: int | None = None, hash_seed: int = 0,
                         hash_words=None, scratch=None, stream=None):
    """Long-block privacy amplification of the kept frames of each block
    (qkd_privacy_amplify_kept_batch): frames [F, N] uint8 on the GPU (a key bit is
    byte & 1), keep [F] uint8 (a frame is kept when its byte is nonzero; typically
    ReconcileResult.verified), blocks of B = frames_per_block consecutive frames (default F:
    one block; F % B != 0 is an error). Returns (out, kept): out [F // B, ceil(out_bits / 64)]
    int64, the hash of privacy_amplify_long of each block's kept frames set end to end in
    frame order with zeros behind them, at the fixed length n_in = B * N; kept [F // B] int32,
    the kept frames of each block. A block that keeps nothing gets zero words, and a dropped
    frame's bytes change nothing. The flags are read on the device only: no host copy, no
    synchronisation, capturable in a graph.

    The prefix rule: out_i = XOR_p r[p + i] x_p depends neither on the zeros behind the input
    nor on out_bits, so for any l <= min(out_bits, kept * N) the first l bits of a block are
    privacy_amplify_long(frames[keep != 0] as one block of kept * N bits, l) under the first
    privacy_long_key_words(kept * N, l) words of the same string, or under the same seed. How
    many bits to take is the caller's decision from kept (the finite-key formula); Alice, who
    makes the same call on her frames with the same public flags, B and l, gets the same bits.

    hash_words holds privacy_long_key_words(B * N, out_bits) words; the seeded string is a
    computational stand-in. scratch: a uint8 device tensor of at least
    privacy_kept_scratch_bytes(N, B, out_bits, F // B) bytes; without it the wrapper allocates
    one for the call."""
    _need_cuda(frames, torch.uint8, "frames")
    if frames.dim() != 2 or frames.shape[0] < 1 or frames.shape[1] < 1:
        raise QkdError(N.ERR_INVALID_ARG, f"frames must have shape [F, N], got {list(frames.shape)}")
    f, n = int(frames.shape[0]), int(frames.shape[1])
    b = f if frames_per_block is None else frames_per_block
    if not isinstance(b, int) or b < 1 or f % b != 0:
        raise QkdError(N.ERR_INVALID_ARG, f"frames_per_block must divide the {f} frames, got {b}")
    n_in, blocks = b * n, f // b
    if not isinstance(out_bits, int) or not 1 <= out_bits <= n_in:
        raise QkdError(N.ERR_INVALID_ARG, f"out_bits must be in 1..{n_in}")
    wp = privacy_long_key_words(n_in, out_bits)
    if wp == 0:
        raise QkdError(N.ERR_INVALID_ARG, "frames_per_block * N + out_bits - 1 exceeds 2^27 bits")
    dev = _Device(frames.device.index)
    _need_vec(keep, torch.uint8, f, "keep", dev)
    if hash_words is not None:
        _need_tags(hash_words, wp, "hash_words", dev)
    need = privacy_kept_scratch_bytes(n, b, out_bits, blocks)
    ts = _torch_stream(stream, dev.device)
    if scratch is None:
        # allocated under the launch stream, as in privacy_amplify_long
        with torch.cuda.stream(ts):
            scratch = torch.empty(need, dtype=torch.uint8, device=frames.device)
    else:
        _need_cuda(scratch, torch.uint8, "scratch", dev)
    seed = (0 if hash_seed is None else int(hash_seed)) & (2**64 - 1)
    out = torch.empty(blocks, (out_bits + 63) // 64, dtype=torch.int64, device=frames.device)
    kept = torch.empty(blocks, dtype=torch.int32, device=frames.device)
    N.check(N.lib().qkd_privacy_amplify_kept_batch(dev.device, _ptr(frames), blocks, n, b, out_bits, seed,
                                                   _ptr(hash_words), _ptr(keep), _ptr(out), _ptr(kept), _ptr(scratch),
                                                   scratch.numel(), int(ts.cuda_stream)))
    return out, kept


def keygen(H: HMatrix, seeds, q_nominal: float, seed_offset: int = 0, workspace=None,
           stream=None):
    """generate_random_bit_array + introduce_errors for frames seeded seeds[k] + seed_offset.
    Returns (alice [F,N] u8, bob [F,N] u8, exact_qber [F] f64) on the device."""
    _need_cuda(seeds, torch.int64, "seeds", H)
    if seeds.dim() != 1:
        raise QkdError(N.ERR_INVALID_ARG, f"seeds must be 1-D, got {list(seeds.shape)}")
    f = seeds.numel()
    dev = seeds.device
    a = torch.empty((f, H.num_bit_nodes), dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    q = torch.empty(f, dtype=torch.float64, device=dev)
    N.check(N.lib().qkd_keygen_batch(H.handle, _ws(workspace), _ptr(seeds), seed_offset, f,
                                     q_nominal, _ptr(a), _ptr(b), _ptr(q), _stream(stream, H.device)))
    return a, b, q


@dataclass
class TrialResults:
    iterations: "torch.Tensor"
    syndromes_match: "torch.Tensor"
    keys_match: "torch.Tensor"
    exact_qber: "torch.Tensor"
    counters: "torch.Tensor"      # raw qkd_counters bytes (device)


def run_trials(H: HMatrix, seeds, q_nominal: float, seed_offset: int = 0,
               max_iterations: int = 50, msg_threshold: float = 100.0,
               threshold_enabled: bool = True, workspace=None, stream=None,
               out: TrialResults | None = None, variant: str = "sp_f64",
               minsum_scale: float | None = None, minsum_offset: float | None = None,
               minsum_self_correct: bool = False) -> TrialResults:
    """run_trial (simulation.cpp:161-189) for every frame, fused on the device, plus the
    per-QBER-point counters of simulation.cpp:252-312. seeds: int64 CUDA tensor holding
    the uint64 seed bits."""
    _need_cuda(seeds, torch.int64, "seeds", H)
    if seeds.dim() != 1:
        raise QkdError(N.ERR_INVALID_ARG, f"seeds must be 1-D, got {list(seeds.shape)}")
    f = seeds.numel()
    dev = seeds.device
    if out is not None:
        _need_vec(out.iterations, torch.int32, f, "out.iterations", H)
        _need_vec(out.syndromes_match, torch.uint8, f, "out.syndromes_match", H)
        _need_vec(out.keys_match, torch.uint8, f, "out.keys_match", H)
        _need_vec(out.exact_qber, torch.float64, f, "out.exact_qber", H)
        _need_vec(out.counters, torch.uint8, N.COUNTERS_BYTES, "out.counters", H)
    if out is None:
        out = TrialResults(torch.empty(f, dtype=torch.int32, device=dev),
                           torch.empty(f, dtype=torch.uint8, device=dev),
                           torch.empty(f, dtype=torch.uint8, device=dev),
                           torch.empty(f, dtype=torch.float64, device=dev),
                           torch.empty(N.COUNTERS_BYTES, dtype=torch.uint8, device=dev))
    flags = decoder_flags(threshold_enabled, variant, minsum_scale, minsum_offset, minsum_self_correct)
    N.check(N.lib().qkd_trials_batch(H.handle, _ws(workspace), _ptr(seeds), seed_offset, f,
                                     q_nominal, max_iterations, msg_threshold, flags,
                                     _ptr(out.iterations), _ptr(out.syndromes_match),
                                     _ptr(out.keys_match), _ptr(out.exact_qber),
                                     _ptr(out.counters), _stream(stream, H.device)))
    return out


def interactive_simulation(H: HMatrix, simulation_seed: int, qbers, max_iterations: int = 50,
                           msg_threshold: float = 100.0, threshold_enabled: bool = True,
                           workspace=None, variant: str = "sp_f64") -> dict:
    """QKD_LDPC_interactive_simulation (simulation.cpp:73-137): the QBER points share ONE
    xoshiro256++(simulation_seed) key stream, point after point. Returns host arrays per
    point: exact_qber ("Actual QBER"), errors, iterations, syndromes_match, keys_match,
    success (both flags, "Error reconciliation SUCCESSFUL"). A point whose exact QBER
    would be 0 raises QkdError like the reference's throw; the points before it ran."""
    q = np.ascontiguousarray(qbers, dtype=np.float64)
    p = q.size
    it = np.zeros(p, np.uint32)
    sp = np.zeros(p, np.uint8)
    ko = np.zeros(p, np.uint8)
    ex = np.zeros(p, np.float64)
    er = np.zeros(p, np.uint32)
    done = C.c_size_t(0)
    st = N.lib().qkd_interactive_batch(H.handle, _ws(workspace), simulation_seed, p, q.ctypes.data,
                                       max_iterations, msg_threshold,
                                       decoder_flags(threshold_enabled, variant), it.ctypes.data,
                                       sp.ctypes.data, ko.ctypes.data, ex.ctypes.data, er.ctypes.data,
                                       C.byref(done))
    k = done.value
    out = {"points_done": k, "exact_qber": ex[:k], "errors": er[:k], "iterations": it[:k],
           "syndromes_match": sp[:k].astype(bool), "keys_match": ko[:k].astype(bool),
           "success": (sp[:k] & ko[:k]).astype(bool)}
    if st != N.OK:
        err = QkdError(st, N.last_error())
        err.partial = out
        raise err
    return out


def trace_decode(H: HMatrix, llr, syndrome, max_iterations: int = 50, msg_threshold: float = 100.0,
                 threshold_enabled: bool = True) -> dict:
    """TRACE_SUM_PRODUCT / TRACE_SUM_PRODUCT_LLR of the reference decoder
    (qkd_ldpc_algorithm.cpp:212-330) for one frame, decoded on the device.
    llr [N] float64 and syndrome [M] 0/1 as host arrays. Returns per executed
    iteration t the arrays the reference prints:
      E[t]  check-to-bit messages after the clamp, bit by bit (each bit's checks
            ascending) - the reference's check_to_bit_msg rows
      L[t]  bit totals;  z[t] hard decision;  s[t] its syndrome
      M[t]  bit-to-check messages after the clamp, check by check (each check's
            bits ascending) - bit_to_check_msg; only for iterations that did not
            stop (the reference computes M after the syndrome test)
    and max_llr (MAX_LLR: the largest |E|, |M| over those iterations)."""
    llr = np.ascontiguousarray(llr, dtype=np.float64)
    syn = np.ascontiguousarray(np.asarray(syndrome) != 0, dtype=np.uint8)
    n, m = H.num_bit_nodes, H.num_check_nodes
    cptr, cidx, bptr, bidx = H.adjacency()
    e = len(cidx)
    E = np.zeros((max_iterations, e), np.float64)
    L = np.zeros((max_iterations, n), np.float64)
    it = C.c_uint32()
    ok = C.c_uint8()
    flags = decoder_flags(threshold_enabled, "sp_f64")
    N.check(N.lib().qkd_trace_decode(H.handle, llr.ctypes.data, syn.ctypes.data, max_iterations,
                                     msg_threshold, flags, E.ctypes.data, L.ctypes.data,
                                     C.byref(it), C.byref(ok)))
    t_n = it.value
    E, L = E[:t_n], L[:t_n]
    z = (L <= 0).astype(np.uint8)
    # s: calculate_syndrome of each hard decision
    chk_of = np.repeat(np.arange(m), np.diff(cptr))
    s = np.zeros((t_n, m), np.uint8)
    for t in range(t_n):
        np.bitwise_xor.at(s[t], chk_of, z[t][cidx])
    # M: b2c[j][pos] = clamp(L_i - E[i][k]) for the edge (bit i's k-th check j)
    bit_of_e = np.repeat(np.arange(n), np.diff(bptr))
    pos_in_check = {}
    for j in range(m):
        for p, b in enumerate(cidx[cptr[j]:cptr[j + 1]]):
            pos_in_check[(j, int(b))] = cptr[j] + p
    to_check_order = np.array([pos_in_check[(int(bidx[k]), int(bit_of_e[k]))] for k in range(e)])
    stopped = bool(ok.value)
    t_m = t_n - 1 if stopped else t_n
    M = np.zeros((t_m, e), np.float64)
    max_llr = 0.0
    for t in range(t_m):
        b2c = L[t][bit_of_e] - E[t]
        if threshold_enabled:
            b2c = np.where(b2c > msg_threshold, msg_threshold, np.where(b2c < -msg_threshold, -msg_threshold, b2c))
        M[t][to_check_order] = b2c
        for arr in (E[t], M[t]):
            a = np.abs(arr)
            a = a[~np.isnan(a)]
            if a.size:
                max_llr = max(max_llr, float(a.max()))
    return {"iterations": t_n, "syndromes_match": stopped, "E": E, "L": L, "z": z, "s": s, "M": M,
            "max_llr": max_llr}


def read_counters(counters) -> N.Counters:
    raw = counters.detach().cpu().numpy().tobytes()
    return N.Counters.from_buffer_copy(raw)


def counters_to_stats(c: N.Counters, trials: int, max_iterations: int,
                      initial_qber: float) -> dict:
    """sim_result fields (simulation.hpp:29-43) from exact integer counters. The mean
    and population std match the reference's two-pass double arithmetic to the
    6 significant digits its CSV prints (simulation.cpp:285-312)."""
    sp, ok = int(c.sp_ok), int(c.ldpc_ok)
    mean = std = 0.0
    mn, mx = max_iterations, 0
    if sp > 0:
        s1, s2 = int(c.sum_iters), int(c.sum_iters_sq)
        mean = s1 / sp
        std = ((sp * s2 - s1 * s1) / (sp * sp)) ** 0.5   # exact integer numerator
        mn, mx = int(c.min_iters), int(c.max_iters)
    return {
        "initial_QBER": initial_qber,
        "iterations_successful_sp_mean": mean,
        "iterations_successful_sp_std_dev": std,
        "iterations_successful_sp_min": 0 if mn == max_iterations else mn,
        "iterations_successful_sp_max": mx,
        "ratio_trials_successful_sp": sp / trials,
        "ratio_trials_successful_ldpc": ok / trials,
        "fer": 1.0 - ok / trials,
        "sum_iters_sp": int(c.sum_iters),
    }


def make_seeds(simulation_seed: int, count: int) -> np.ndarray:
    """seeds[k] = k-th raw xoshiro256++(simulation_seed) draw (simulation.cpp:222-228)."""
    out = np.zeros(count, np.uint64)
    N.check(N.lib().qkd_make_seeds(simulation_seed, count, out.ctypes.data))
    return out


def qber_range(begin: float, end: float, step: float) -> list[float]:
    """One row of get_rate_based_QBER_range (simulation.cpp:48-70)."""
    cnt = C.c_size_t(0)
    N.check(N.lib().qkd_qber_range(begin, end, step, None, 0, C.byref(cnt)))
    vals = np.zeros(max(cnt.value, 1), np.float64)
    N.check(N.lib().qkd_qber_range(begin, end, step, vals.ctypes.data, cnt.value, C.byref(cnt)))
    return vals[: cnt.value].tolist()
