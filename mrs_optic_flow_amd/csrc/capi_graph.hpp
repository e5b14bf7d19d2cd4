// capi_graph.hpp -- what the C ABI's engines need to be safe next to HIP graphs (host side only).
//
// Two hazards, both seen on the GPU box in round 2 (gpurun_out/r02r_c5graph.err, r02s_c5graph.err):
//  1. A batch call captured into a graph bakes raw pointers to engine-owned device memory (twiddles, the estimator's
//     scratch) into the graph's kernel nodes. Freeing or re-allocating that memory under the graph makes every later
//     replay read and write freed memory. An engine therefore gets PINNED by a captured call: while pinned its scratch
//     never moves (growth fails with MOF_ERR_BUSY) and mof_*_destroy does not free -- the engine is parked on a
//     process-wide list until the owner says the graphs are gone (mof_*_release_graphs / mof_purge_deferred).
//  2. hipFree / hipMalloc on ANY thread while some stream captures in HIP's default global mode is answered by
//     invalidating that capture. The library's own allocation and release paths run under the relaxed mode of the
//     calling thread (RelaxedCapture), the documented way for a library to stay out of other people's captures.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>

namespace mof {

// Non-re-entrancy flag of the reference (`running`, FftMethod.cpp:1775-1777), made atomic.
struct BusyGuard {
  std::atomic<bool>& flag;
  bool owned;
  explicit BusyGuard(std::atomic<bool>& f) : flag(f), owned(!f.exchange(true)) {}
  ~BusyGuard() {
    if (owned) flag.store(false);
  }
};

struct RelaxedCapture {
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  RelaxedCapture() { (void)hipThreadExchangeStreamCaptureMode(&mode); }
  ~RelaxedCapture() { (void)hipThreadExchangeStreamCaptureMode(&mode); }
  RelaxedCapture(const RelaxedCapture&) = delete;
  RelaxedCapture& operator=(const RelaxedCapture&) = delete;
};

inline bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

// Synchronous copy / fill on a stream of the engine's own (non-blocking): hipMemcpy / hipMemset run on the legacy stream,
// which implicitly joins every blocking stream -- a capturing one included ("operation would make the legacy stream depend
// on a capturing blocking stream"), so they cannot be used by a library that may be called beside a capture.
inline hipError_t copy_on(hipStream_t s, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}
inline hipError_t fill_on(hipStream_t s, void* dst, int value, size_t bytes) {
  const hipError_t e = hipMemsetAsync(dst, value, bytes, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}

// Ordering of engine-owned scratch across streams: every call that touches the scratch records the event behind its last kernel
// (release); a later call on a DIFFERENT stream first makes its stream wait for it (acquire; same-stream calls are ordered by the
// stream itself). Called with the engine's busy flag held.
struct ScratchFence {
  hipEvent_t ev = nullptr;
  hipStream_t stream = nullptr;  // stream of the last user
  bool scratch_used = false;
  hipError_t create() { return hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
  void destroy() {
    if (ev) (void)hipEventDestroy(ev);
  }
  // before the first launch that reads or writes the scratch
  hipError_t acquire(hipStream_t s) {
    if (!scratch_used || stream == s) return hipSuccess;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const hipError_t err = hipStreamIsCapturing(s, &cap);
    if (err != hipSuccess) return err;
    // a capturing stream must not take a dependency on work outside its graph: the caller orders graph replays
    return cap == hipStreamCaptureStatusNone ? hipStreamWaitEvent(s, ev, 0) : hipSuccess;
  }
  // behind the last launch of the call
  hipError_t release(hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    hipError_t err = hipStreamIsCapturing(s, &cap);
    if (err != hipSuccess) return err;
    if (cap != hipStreamCaptureStatusNone) return hipSuccess;  // events recorded while capturing belong to the graph
    err = hipEventRecord(ev, s);
    if (err != hipSuccess) return err;
    stream = s;
    scratch_used = true;
    return hipSuccess;
  }
  // before the scratch is re-allocated or freed: a batch on a caller's stream may still use it
  void wait_idle() {
    if (ev && scratch_used) (void)hipEventSynchronize(ev);
  }
};

// engines whose destroy was deferred because a captured graph may still use their device memory
void park_engine(void (*destroy_now)(void*), void* engine);  // mof_capi.hip
int purge_parked();                                          // frees every parked engine, returns how many
int parked_count();

}  // namespace mof
