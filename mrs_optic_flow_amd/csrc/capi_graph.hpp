// capi_graph.hpp -- what the C ABI's engines share (host side only, not installed): the error macro, the device check, and what
// keeps them safe next to HIP graphs.
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
#include <initializer_list>

#include "dev_mem.hpp"
#include "mof.h"

namespace mof {

int capi_fail(int code, const char* fmt, ...);  // mof_capi.hip: records the calling thread's last error text, returns `code`

#define HIP_TRY(expr)                                                                                 \
  do {                                                                                                \
    hipError_t _e = (expr);                                                                           \
    if (_e != hipSuccess) return mof::capi_fail(MOF_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

// "is there a device" (*n_devices receives how many), and "... and is `device` one of them": then it is made the calling thread's
inline int require_device(int* n_devices) {
  if (hipGetDeviceCount(n_devices) != hipSuccess || *n_devices <= 0) {
    (void)hipGetLastError();
    return capi_fail(MOF_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
  }
  return MOF_OK;
}
inline int select_device(int device) {
  int n = 0;
  const int rc = require_device(&n);
  if (rc) return rc;
  if (device < 0 || device >= n) return capi_fail(MOF_ERR_BAD_ARG, "device %d out of range (0..%d)", device, n - 1);
  HIP_TRY(hipSetDevice(device));
  return MOF_OK;
}

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

// Ordering of engine-owned scratch across streams: every call that touches the scratch records the event behind its last kernel
// (release); a later call on a DIFFERENT stream first makes its stream wait for it (acquire; same-stream calls are ordered by the
// stream itself). Called with the engine's busy flag held.
struct ScratchFence {
  Event ev;
  hipStream_t stream = nullptr;  // stream of the last user
  bool scratch_used = false;
  hipError_t create() { return ev.create(); }
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

// The one way engine-owned scratch grows from `have` to `want` units (hazard 1 above): refused while a graph pins the engine
// (MOF_ERR_BUSY) and inside a capture of the call's stream (MOF_ERR_BAD_ARG); otherwise every earlier user of the scratch -- the
// fence, the engine's own streams `drain` -- has finished before realloc(want) -> hipError_t frees and allocates. When that fails
// realloc(fallback) restores the smallest scratch, so the stateful entry stays usable, and the failure is reported. `noun` names the
// scratch and its unit in the messages. Called with the engine's busy flag held and its device current.
template <class Realloc>
int grow_scratch(bool pinned, ScratchFence& fence, std::initializer_list<hipStream_t> drain, bool capturing, const char* noun, long have,
                 long want, long fallback, Realloc&& realloc) {
  if (want <= have) return MOF_OK;
  if (pinned)
    return capi_fail(MOF_ERR_BUSY, "%s would have to grow from %ld to %ld, but a captured HIP graph still points into it: run (or "
                                   "reserve) the largest batch before capturing, or call mof_*_release_graphs once the graphs are gone",
                     noun, have, want);
  if (capturing)
    return capi_fail(MOF_ERR_BAD_ARG, "%s must grow to %ld, which cannot happen inside a graph capture: run (or reserve) one batch of "
                                      "this size before capturing", noun, want);
  fence.wait_idle();
  for (hipStream_t s : drain) (void)hipStreamSynchronize(s);
  const hipError_t err = realloc(want);
  if (err == hipSuccess) return MOF_OK;
  (void)realloc(fallback);
  return capi_fail(err == hipErrorOutOfMemory ? MOF_ERR_NO_MEMORY : MOF_ERR_HIP, "%s, %ld: %s", noun, want, hipGetErrorString(err));
}

// engines whose destroy was deferred because a captured graph may still use their device memory
void park_engine(void (*destroy_now)(void*), void* engine);  // mof_capi.hip
int purge_parked();                                          // frees every parked engine, returns how many
int parked_count();

}  // namespace mof
