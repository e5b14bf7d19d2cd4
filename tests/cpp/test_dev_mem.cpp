// Host-only unit test of csrc/dev_mem.hpp and the scratch-growth guard of csrc/capi_graph.hpp: the owners' move-only contract and what they do
// when no device answers, the guard's four outcomes with stub callables. No library and no device code: the HIP runtime API only.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "capi_graph.hpp"

using namespace mof;

// the library's error sink (mof_capi.hip), restated: the guard reports through it
static char g_text[512];
int mof::capi_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_text, sizeof(g_text), fmt, ap);
  va_end(ap);
  return code;
}

static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

template <class O>
constexpr bool move_only = !std::is_copy_constructible<O>::value && !std::is_copy_assignable<O>::value &&
                           std::is_nothrow_move_constructible<O>::value && std::is_nothrow_move_assignable<O>::value;
static_assert(move_only<DevMem<float>> && move_only<PinnedMem<double>> && move_only<Stream> && move_only<Event>, "owners are move-only");

// release() counts instead of calling the runtime: move and reset semantics of the one base every owner shares
static int released = 0;
struct CountRelease {
  void operator()(int* p) const { released += *p; }
};
struct Fake : Owner<int*, CountRelease> {
  void hold(int* p) {
    reset();
    (void)adopt(hipSuccess, p);
  }
};

static void check_owner_contract() {
  int one = 1, ten = 10;
  {
    Fake a;
    a.reset();  // empty: nothing released, here and in the destructor
    CHECK(a.get() == nullptr && released == 0);
    a.hold(&one);
    Fake b(std::move(a));
    CHECK(a.get() == nullptr && b.get() == &one && static_cast<int*>(b) == &one && released == 0);
    Fake c;
    c.hold(&ten);
    c = std::move(b);  // releases what c held, leaves b empty
    CHECK(released == 10 && b.get() == nullptr && c.get() == &one);
    Fake& same = c;
    c = std::move(same);  // self-move: nothing happens
    CHECK(released == 10 && c.get() == &one);
    c.reset();
    c.reset();
    CHECK(released == 11 && c.get() == nullptr);
    Fake d;
    d.hold(&ten);
  }  // d releases once, a / b / c nothing
  CHECK(released == 21);
}

// where no device answers: the HIP error, an empty owner, the live count untouched
static void check_without_device() {
  int n = 0;
  if (hipGetDeviceCount(&n) == hipSuccess && n > 0) {
    std::printf("dev_mem: a device answers, the no-device checks are skipped\n");
    return;
  }
  (void)hipGetLastError();
  DevMem<float> d;
  PinnedMem<double> h;
  Stream s;
  Event e;
  CHECK(d.alloc(16) != hipSuccess && d.get() == nullptr);
  CHECK(h.alloc(16) != hipSuccess && h.get() == nullptr);
  CHECK(s.create() != hipSuccess && s.get() == nullptr);
  CHECK(e.create() != hipSuccess && e.get() == nullptr);
  DevMem<int> a, b;
  CHECK(alloc_all(a, 4, b, 8) != hipSuccess && !a && !b);
  CHECK(upload(d, std::vector<float>(8, 1.f), nullptr) != hipSuccess && !d);
  CHECK(g_live_buffers.load() == 0);
  CHECK(require_device(&n) == MOF_ERR_NO_DEVICE && select_device(0) == MOF_ERR_NO_DEVICE);
}

static void check_growth_guard() {
  ScratchFence fence;  // never created: wait_idle has nothing to wait for
  std::vector<long> asked;
  hipError_t answer = hipSuccess;
  auto realloc = [&](long n) {
    asked.push_back(n);
    return n == 1 ? hipSuccess : answer;
  };
  // the size already fits: the callable is not called
  CHECK(grow_scratch(true, fence, {}, true, "scratch", 8, 8, 1, realloc) == MOF_OK && asked.empty());
  CHECK(grow_scratch(false, fence, {}, false, "scratch", 8, 3, 1, realloc) == MOF_OK && asked.empty());
  // pinned by a graph, pinned AND capturing: busy; capturing: a bad argument; both texts name the graph; nothing is touched
  CHECK(grow_scratch(true, fence, {}, false, "scratch", 8, 9, 1, realloc) == MOF_ERR_BUSY && std::strstr(g_text, "graph") && asked.empty());
  CHECK(grow_scratch(true, fence, {}, true, "scratch", 8, 9, 1, realloc) == MOF_ERR_BUSY && asked.empty());
  CHECK(grow_scratch(false, fence, {}, true, "scratch", 8, 9, 1, realloc) == MOF_ERR_BAD_ARG && std::strstr(g_text, "graph") && asked.empty());
  // grows: one request of the wanted size
  CHECK(grow_scratch(false, fence, {}, false, "scratch", 8, 16, 1, realloc) == MOF_OK && asked == std::vector<long>({16}));
  // the realloc fails: the fallback size is requested, the failure's code comes back
  asked.clear();
  answer = hipErrorOutOfMemory;
  CHECK(grow_scratch(false, fence, {}, false, "scratch", 8, 16, 1, realloc) == MOF_ERR_NO_MEMORY && asked == std::vector<long>({16, 1}));
  CHECK(std::strstr(g_text, "scratch") != nullptr);
  asked.clear();
  answer = hipErrorInvalidValue;
  CHECK(grow_scratch(false, fence, {nullptr}, false, "scratch", 0, 4, 1, realloc) == MOF_ERR_HIP && asked == std::vector<long>({4, 1}));
}

int main() {
  check_owner_contract();
  check_without_device();
  check_growth_guard();
  std::printf("dev_mem: %d failures\n", failures);
  return failures ? 1 : 0;
}
