// Host-only unit test of csrc/pc_launch.hpp: the form dispatch and its enumeration, the 65535-pair split, the CU count's fall-back.
// No device code and no kernel: the callables record what they are handed.
#include <cstdio>
#include <set>
#include <tuple>
#include <vector>

#include "pc_launch.hpp"

using namespace mof;
using Form = std::tuple<int, int, int>;

static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

template <int SET>
static void check_set(const std::set<Form>& want) {
  // every triple around the valid values: dispatched to ITS constants when it is a form of SET, refused otherwise
  std::set<Form> got;
  for (int ds = -1; ds <= 5; ++ds)
    for (int ch = -1; ch <= 4; ++ch)
      for (int pk = -1; pk <= 2; ++pk) {
        Form seen{0, 0, 0};
        const hipError_t e = pc_dispatch_form<SET>(ds, ch, pk, [&](auto d, auto c, auto p) {
          seen = Form{decltype(d)::value, decltype(c)::value, decltype(p)::value};
          return hipSuccess;
        });
        if (want.count(Form{ds, ch, pk})) {
          CHECK(e == hipSuccess && seen == (Form{ds, ch, pk}));
          got.insert(seen);
        } else {
          CHECK(e == hipErrorInvalidValue && seen == (Form{0, 0, 0}));
        }
      }
  CHECK(got == want);
  // the enumeration visits exactly those forms, each once, and stops at the first error
  std::vector<Form> visited;
  CHECK(pc_each_form<SET>([&](auto d, auto c, auto p) {
          visited.push_back(Form{decltype(d)::value, decltype(c)::value, decltype(p)::value});
          return hipSuccess;
        }) == hipSuccess);
  CHECK(visited.size() == want.size() && std::set<Form>(visited.begin(), visited.end()) == want);
  int calls = 0;
  CHECK(pc_each_form<SET>([&](auto, auto, auto) { return ++calls == 2 ? hipErrorOutOfMemory : hipSuccess; }) == hipErrorOutOfMemory && calls == 2);
}

static void check_split(int n_pairs, bool with_quality) {
  // (addresses only: nothing is dereferenced)
  const uint8_t* frames = reinterpret_cast<const uint8_t*>(uintptr_t(1) << 40);
  double* results = reinterpret_cast<double*>(uintptr_t(1) << 41);
  PcArgs a{};
  a.cur = frames;
  a.prev = frames + 7;
  a.cur_stride = 1000;
  a.prev_stride = 3000;
  a.grid_x = 3;
  a.grid_y = 2;
  a.out = results;
  a.quality = with_quality ? results + 5 : nullptr;
  a.channels = 3;
  int next = 0, launches = 0;
  CHECK(pc_split_pairs(a, n_pairs, [&](const PcArgs& c, int nk) {
          CHECK(nk >= 1 && nk <= PC_MAX_GRID_PAIRS && (nk == PC_MAX_GRID_PAIRS || next + nk == n_pairs));
          CHECK(c.cur == a.cur + (size_t)next * 1000 && c.prev == a.prev + (size_t)next * 3000);
          CHECK(c.out == a.out + (size_t)next * 12 && c.quality == (with_quality ? a.quality + (size_t)next * 12 : nullptr));
          CHECK(c.total == nk * 6 && c.channels == 3 && c.grid_x == 3 && c.cur_stride == 1000);
          next += nk;
          ++launches;
          return hipSuccess;
        }) == hipSuccess);
  CHECK(next == (n_pairs > 0 ? n_pairs : 0) && launches == (n_pairs + PC_MAX_GRID_PAIRS - 1) / PC_MAX_GRID_PAIRS);
}

int main() {
  const std::set<Form> ch{{1, 1, 0}, {1, 3, 0}};
  std::set<Form> ch_pk = ch, ds_ch = ch, all;
  ch_pk.insert({{1, 1, 1}, {1, 3, 1}});
  ds_ch.insert({4, 1, 0});
  all = ch_pk;
  all.insert({{4, 1, 0}, {4, 1, 1}});
  check_set<PC_FORMS_CH>(ch);
  check_set<PC_FORMS_CH_PK>(ch_pk);
  check_set<PC_FORMS_DS_CH>(ds_ch);
  check_set<PC_FORMS_ALL>(all);
  PcArgs a{};
  a.downscale = 4, a.channels = 1, a.peak_model = 1;
  Form seen{0, 0, 0};
  CHECK(pc_dispatch_form(a, [&](auto d, auto c, auto p) { seen = Form{d, c, p}; return hipSuccess; }) == hipSuccess && seen == (Form{4, 1, 1}));
  a.channels = 3;
  CHECK(pc_dispatch_form(a, [&](auto, auto, auto) { return hipSuccess; }) == hipErrorInvalidValue);
  for (int n : {0, 1, 65534, 65535, 65536, 65540, 2 * 65535, 2 * 65535 + 1}) {
    check_split(n, false);
    check_split(n, true);
  }
  int calls = 0;  // the first error ends the walk
  PcArgs b{};
  b.grid_x = b.grid_y = 1;
  CHECK(pc_split_pairs(b, 3 * 65535, [&](const PcArgs&, int) { return ++calls == 2 ? hipErrorLaunchFailure : hipSuccess; }) == hipErrorLaunchFailure && calls == 2);
  CHECK(PC_MAX_GRID_PAIRS == 65535 && PC_MAX_GRID_IMAGES == 65534);
  const int cus = pc_cu_count();  // the current device's, or 256 where there is none
  CHECK(cus > 0);
  CHECK(pc_cu_count(1 << 20) == 256);  // no such device: the fall-back
  std::printf("pc_launch: %d failures (cu count here: %d)\n", failures, cus);
  return failures ? 1 : 0;
}
