// qkd_host.h — what one .hip file of the library defines and another calls
// (host side; not part of the ABI, and not for the stand-alone native checks,
// which include the plain-C++ headers only). Each item is declared under the
// file that defines it.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

#include "qkd_decode.h"
#include "qkd_internal.h"

namespace qkd {

// ---- launch.hip ---------------------------------------------------------------
// Workspace helpers.
qkd_status ws_reserve_decode(qkd_workspace* ws, size_t slots);
qkd_status ws_reserve_keys(qkd_workspace* ws, size_t frames, size_t low_words);
qkd_workspace* resolve_ws(const qkd_code* code, qkd_workspace* ws);

// Serialise users of one workspace across streams: wait for the previous
// user's completion event, record ours after our launches.
struct WsSession {
    qkd_workspace* ws;
    hipStream_t stream;
    std::unique_lock<std::mutex> lk;
    // a stream under capture: the workspace's event stays out of the graph (it
    // would tie later, uncaptured calls to the capture); the caller orders the
    // graph's replays against other users of the workspace
    bool capturing = false;
    WsSession(qkd_workspace* w, hipStream_t s) : ws(w), stream(s), lk(w->mu) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cs) == hipSuccess) capturing = cs != hipStreamCaptureStatusNone;
        else (void)hipGetLastError();
        if (capturing) return;
        if (ws->done) (void)hipStreamWaitEvent(stream, ws->done, 0);
    }
    ~WsSession() {
        if (capturing) return;
        if (!ws->done) (void)hipEventCreateWithFlags(&ws->done, hipEventDisableTiming);
        if (ws->done) (void)hipEventRecord(ws->done, stream);
    }
};

unsigned blocks_for(size_t n, unsigned bs);

// qkd_debug_decoder_timing (debug.hip): the finished event pairs into the totals
hipError_t decoder_events_fold(qkd_workspace* ws);

// What a decode launch writes besides the decoder's own outputs.
// corrected (qkd_reconcile_batch, or nullptr): popcount(bits_out ^ bob) per
// frame, from the kernel that follows the decoder. verify
// (qkd_reconcile_verify_batch, or nullptr): the frames' verification tags, from
// that kernel too.
// adapt (kModeClass, qkd_reconcile_adaptive_batch): the plan and Bob's payload;
// the class bytes are written by the launch, in the bit order of the kernel
// that runs.
struct DecodeIo {
    uint32_t* corrected = nullptr;
    const VerifyArgs* verify = nullptr;
    const ClassArgs* adapt = nullptr;
};

qkd_status launch_decode(const qkd_code* c, qkd_workspace* ws, DecodeArgs& a, int mode, uint32_t flags,
                         hipStream_t stream, const DecodeIo& io = DecodeIo());

// ---- decode.hip ---------------------------------------------------------------
// the classic kernels' lookup (qkd_decode.h: split_kernel, ilv_kernel)
DecodeFn classic_kernel(const KernelKey& k);

// ---- api.hip ------------------------------------------------------------------
qkd_status check_frames(size_t n_frames);
qkd_status check_decode_params(uint32_t max_it, double thr, uint32_t flags, bool erasures_ok = false);
qkd_status decode_keys(const qkd_code* c, qkd_workspace* ws, size_t n_frames, double q,
                       uint32_t max_it, double thr, uint32_t flags, uint8_t* bits_out,
                       uint32_t* iters, uint8_t* sp_ok, uint8_t* key_ok, hipStream_t stream,
                       const uint8_t* alice_b = nullptr, const uint8_t* bob_b = nullptr,
                       const uint8_t* syn = nullptr, uint32_t* corrected = nullptr,
                       const VerifyArgs* verify = nullptr);

// ---- keygen.hip ---------------------------------------------------------------
qkd_status keygen_into_ws(const qkd_code* c, qkd_workspace* ws, const uint64_t* seeds,
                          uint64_t offset, size_t n_frames, double q_nom, double* exact_q,
                          hipStream_t stream);

// ---- bits.hip -----------------------------------------------------------------
// (launched by qkd_keygen_batch, keygen.hip)
__global__ void unpack_kernel(const uint64_t* words_in, uint32_t n, uint32_t words, uint32_t n_frames,
                              uint8_t* out);

// ---- counters.hip -------------------------------------------------------------
hipError_t launch_counters(const uint32_t* iters, const uint8_t* sp, const uint8_t* ko, size_t n_frames,
                           qkd_counters* c, hipStream_t stream);

// ---- frame_out.hip ------------------------------------------------------------
VerifyArgs verify_args(const qkd_code* c, uint64_t hash_seed, const uint64_t* hash_words, uint32_t tag_bits,
                       const uint64_t* alice_tags, uint64_t* tags_out, uint8_t* verified, const uint8_t* sp_ok);

}  // namespace qkd

// keygen.hip, launched by qkd_interactive_batch (api.hip); the kernel keeps the
// unmangled name it has always had
extern "C" __global__ void keygen_stream_kernel(uint64_t sim_seed, uint32_t n, uint32_t words, uint32_t n_points,
                                                const uint32_t* ne, uint64_t* alice_w, uint64_t* bob_w,
                                                uint32_t* low);
