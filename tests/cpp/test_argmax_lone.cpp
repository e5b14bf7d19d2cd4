// Host-only test of the short cut K1 at 64 takes behind its arg-max barrier (csrc/pc_argmax.hpp, the functions the kernel inlines): a lone
// lane. Where ONE lane of a wave holds the maximum gm, the wave reads that lane's own (m, mi) instead of folding 64 pairs. Held to the
// fold itself: wave_best's xor butterfly 32, 16 .. 1 with better(), every lane folding (own, partner), on entries made by argmax_entry --
// every lane as the holder, +0 / -0 / -inf / tiny and huge maxima, indices up to 0x7fffffff, NaN-free m (as the kernel's fmaxf chains leave
// it). Counts other than one (two lanes, +0 beside -0, all -inf) must NOT take the short cut.
// Stand-alone, built with -fsanitize=address,undefined (argmax_lone.mk). No device, no library.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "pc_argmax.hpp"

using namespace mof;

namespace {

constexpr int LANES = 64;
int failures = 0;

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
bool same(Best a, Best b) { return bits(a.v) == bits(b.v) && a.idx == b.idx; }

// wave_best (csrc/pc_common.hpp): lane l folds better(own, the pair of lane l ^ off), off = 32, 16, 8, 4, 2, 1; every lane's result is kept
std::vector<Best> butterfly(std::vector<Best> b) {
  for (int off = 32; off > 0; off >>= 1) {
    std::vector<Best> n(LANES);
    for (int l = 0; l < LANES; ++l) n[l] = better(b[l], b[l ^ off]);
    b = n;
  }
  return b;
}

unsigned long long ballot(const std::vector<float>& m, float gm) {
  unsigned long long mask = 0;
  for (int l = 0; l < LANES; ++l) mask |= (unsigned long long)(m[l] == gm) << l;
  return mask;
}

void lone_lane() {
  const float inf = std::numeric_limits<float>::infinity();
  const float maxima[] = {2.f, 0.f, -0.f, -3.e38f, 3.e38f, 1e-45f, -1e-45f, -1.f};
  const int indices[] = {0, 1, 2047, 4095, 0x7ffffffe, 0x7fffffff};
  int cases = 0;
  for (float gm_val : maxima)
    for (int holder = 0; holder < LANES; ++holder)
      for (int idx : indices)
        for (int low = 0; low < 3; ++low) {
          // the other lanes: strictly below the maximum -- a value just below, -inf, or a mix --, each with an index that would win a tie
          std::vector<float> m(LANES);
          std::vector<int> mi(LANES);
          for (int l = 0; l < LANES; ++l) {
            m[l] = low == 0 ? std::nextafter(gm_val, -inf) : (low == 1 ? -inf : ((l & 1) ? -inf : -2.f * std::fabs(gm_val) - 1.f - (float)l));
            mi[l] = (l * 67) % 4096;
          }
          m[holder] = gm_val, mi[holder] = idx;
          float gm = -inf;
          for (float x : m) gm = std::fmax(gm, x);
          const unsigned long long holders = ballot(m, gm);
          std::vector<Best> in(LANES);
          for (int l = 0; l < LANES; ++l) in[l] = argmax_entry(m[l], gm, mi[l]);
          const std::vector<Best> out = butterfly(in);
          ++cases;
          if (!argmax_lone_holder(holders) || argmax_lone_lane(holders) != holder) {
            std::printf("FAILED lone lane: holder %d, ballot %llx\n", holder, holders);
            ++failures;
            continue;
          }
          const int L = argmax_lone_lane(holders);
          const Best took{m[L], mi[L]};
          for (int l = 0; l < LANES; ++l)
            if (!same(out[l], took)) {
              std::printf("FAILED lone lane: holder %d max %a idx %d: lane %d folds to {%a, %d}\n", holder, gm_val, idx, l, out[l].v, out[l].idx);
              ++failures;
              break;
            }
        }
  // counts other than one keep the fold: two lanes, +0 beside -0 (they compare equal), every lane at -inf
  {
    std::vector<float> m(LANES, -1.f);
    m[5] = m[44] = 2.f;
    if (argmax_lone_holder(ballot(m, 2.f))) std::printf("FAILED: two holders taken for one\n"), ++failures;
    m[5] = 0.f, m[44] = -0.f;
    if (argmax_lone_holder(ballot(m, 0.f)) || argmax_lone_holder(ballot(m, -0.f))) std::printf("FAILED: +0 beside -0 taken for one holder\n"), ++failures;
    std::vector<float> flat(LANES, -inf);
    if (argmax_lone_holder(ballot(flat, -inf))) std::printf("FAILED: the all -inf wave taken for one holder\n"), ++failures;
    if (argmax_lone_holder(0ull)) std::printf("FAILED: the empty ballot taken for one holder\n"), ++failures;
  }
  std::printf("lone lane: %d waves\n", cases);
}

}  // namespace

int main() {
  lone_lane();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("argmax lone ok\n");
  return 0;
}
