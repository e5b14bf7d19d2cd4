// dev_mem.hpp -- the owners of what an engine holds on the HIP runtime (host side only, not installed): device memory, pinned host
// memory, a non-blocking stream, a timing-disabled event. Move-only; alloc / create return the HIP error and leave the owner empty
// on failure; reset() and the destructor release and are no-ops on an empty owner; get() -- or the implicit conversion -- hands the raw
// handle to a launch. An engine struct declares them so that C++'s reverse destruction order IS the teardown order: streams first,
// then events, then buffers, the host pipes last (mof_capi.hip, mof_sr.hip). No allocator, no pool: one hipMalloc per alloc.
// Every call here is an allocation or a release: the caller holds a RelaxedCapture (capi_graph.hpp) around it.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>
#include <utility>
#include <vector>

namespace mof {

// device and pinned allocations alive in this process (streams and events are not counted): mof_live_buffers(), a test and diagnostic aid
inline std::atomic<int> g_live_buffers{0};

template <class H, class Release>
class Owner {
 public:
  Owner() = default;
  Owner(Owner&& o) noexcept : h_(std::exchange(o.h_, H{})) {}
  Owner& operator=(Owner&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, H{});
    }
    return *this;
  }
  Owner(const Owner&) = delete;
  Owner& operator=(const Owner&) = delete;
  ~Owner() { reset(); }
  void reset() {
    if (h_) Release{}(h_);
    h_ = H{};
  }
  H get() const { return h_; }
  operator H() const { return h_; }

 protected:
  hipError_t adopt(hipError_t e, H h) {  // of a fresh handle, after reset()
    if (e == hipSuccess) h_ = h;
    return e;
  }

 private:
  H h_{};
};

struct DevRelease {
  void operator()(void* p) const {
    (void)hipFree(p);
    --g_live_buffers;
  }
};
struct PinnedRelease {
  void operator()(void* p) const {
    (void)hipHostFree(p);
    --g_live_buffers;
  }
};
struct StreamRelease {
  void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};
struct EventRelease {
  void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};

// `count` elements of T; what the owner held before is released first
template <class T, class Release>
struct Mem : Owner<T*, Release> {
  hipError_t alloc(size_t count) {
    this->reset();
    void* p = nullptr;
    const hipError_t e = std::is_same<Release, DevRelease>::value ? hipMalloc(&p, count * sizeof(T))
                                                                  : hipHostMalloc(&p, count * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess && p) ++g_live_buffers;
    return this->adopt(e, static_cast<T*>(p));
  }
};
template <class T>
using DevMem = Mem<T, DevRelease>;
template <class T>
using PinnedMem = Mem<T, PinnedRelease>;

struct Stream : Owner<hipStream_t, StreamRelease> {
  hipError_t create() {
    reset();
    hipStream_t s = nullptr;
    return adopt(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), s);
  }
};
struct Event : Owner<hipEvent_t, EventRelease> {
  hipError_t create() {
    reset();
    hipEvent_t e = nullptr;
    return adopt(hipEventCreateWithFlags(&e, hipEventDisableTiming), e);
  }
};

// alloc_all(a, na, b, nb, ...): every owner released FIRST (a regrowth never holds the old and the new scratch at once), then
// allocated in order; ends at the first error
inline void reset_all() {}
template <class M, class... R>
void reset_all(M& m, size_t, R&&... rest) {
  m.reset();
  reset_all(rest...);
}
inline hipError_t alloc_each() { return hipSuccess; }
template <class M, class... R>
hipError_t alloc_each(M& m, size_t count, R&&... rest) {
  const hipError_t e = m.alloc(count);
  return e != hipSuccess ? e : alloc_each(rest...);
}
template <class... A>
hipError_t alloc_all(A&&... a) {
  reset_all(a...);
  return alloc_each(a...);
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

// a host table on the device: allocated to the vector's size and copied on `s`, synchronously
template <class T>
hipError_t upload(DevMem<T>& d, const std::vector<T>& v, hipStream_t s) {
  const hipError_t e = d.alloc(v.size());
  return e != hipSuccess ? e : copy_on(s, d.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

}  // namespace mof
