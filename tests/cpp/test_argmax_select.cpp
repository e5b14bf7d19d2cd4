// Host-only test of K1's value-first arg-max (csrc/pc_argmax.hpp, the functions the kernel inlines; csrc/pc_kernel.hip for the flow).
// A workgroup is 4 waves x 64 lanes x 16 candidates. The parent flow folds every lane's (m, mi) with better(): a butterfly in each wave,
// then the four wave results in order. The value-first flow reduces m alone, lets only the lanes with m == gm into the butterfly (the
// others carry the neutral pair), and only the waves that hold such a lane; the rest store the neutral pair. Both are compared, value
// BITS and index, with each other and with the plain sequential better() fold over all 256 lanes, on arrays with planted ties (inside
// a lane, across lanes, across waves), +0 against -0, -inf and NaN. No device, no library.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "pc_argmax.hpp"

using namespace mof;

namespace {

constexpr int WAVES = 4, LANES = 64, CAND = 16, TOTAL = WAVES * LANES * CAND;
int failures = 0;

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
bool same(Best a, Best b) { return bits(a.v) == bits(b.v) && a.idx == b.idx; }

struct LaneBest {
  float m;
  int mi;
};
// what col_pass_inv leaves in a lane: the fmaxf chain seeded with -inf, then the smallest index that attains it
LaneBest lane_best(const float* v, const int* idx) {
  float m = -std::numeric_limits<float>::infinity();
  for (int c = 0; c < CAND; ++c) m = std::fmax(m, v[c]);  // (fmaxf: a NaN operand is dropped)
  int mi = 0x7fffffff;
  for (int c = 0; c < CAND; ++c) mi = argmax_first_index(mi, v[c], m, idx[c]);
  return {m, mi};
}
// wave_best: the xor butterfly 32, 16, .. 1, every lane folding (own, partner); lane 0's result is what is stored
Best butterfly(std::vector<Best> b) {
  for (int off = 32; off > 0; off >>= 1) {
    std::vector<Best> n(LANES);
    for (int l = 0; l < LANES; ++l) n[l] = better(b[l], b[l ^ off]);
    b = n;
  }
  for (int l = 1; l < LANES; ++l)
    if (!same(b[l], b[0])) {
      std::printf("FAILED: butterfly lanes disagree (lane %d)\n", l);
      ++failures;
    }
  return b[0];
}

void check(const char* name, const std::vector<float>& v, const std::vector<int>& idx) {
  std::vector<LaneBest> lb(WAVES * LANES);
  for (int t = 0; t < WAVES * LANES; ++t) lb[t] = lane_best(&v[(size_t)t * CAND], &idx[(size_t)t * CAND]);
  // sequential fold over all lanes
  Best seq = argmax_neutral();
  for (const LaneBest& l : lb) seq = better(seq, Best{l.m, l.mi});
  // parent: per-wave butterfly, then wave 0's result folded with red[1..3]
  Best red[WAVES];
  for (int w = 0; w < WAVES; ++w) {
    std::vector<Best> b(LANES);
    for (int l = 0; l < LANES; ++l) b[l] = Best{lb[w * LANES + l].m, lb[w * LANES + l].mi};
    red[w] = butterfly(b);
  }
  Best parent = red[0];
  for (int w = 1; w < WAVES; ++w) parent = better(parent, red[w]);
  // value first
  float wm[WAVES], gm;
  for (int w = 0; w < WAVES; ++w) {
    wm[w] = lb[w * LANES].m;
    for (int l = 1; l < LANES; ++l) wm[w] = std::fmax(wm[w], lb[w * LANES + l].m);
  }
  gm = wm[0];
  for (int w = 1; w < WAVES; ++w) gm = std::fmax(gm, wm[w]);
  int waves_in = 0;
  for (int w = 0; w < WAVES; ++w) {
    bool any = false;
    for (int l = 0; l < LANES; ++l) any |= lb[w * LANES + l].m == gm;
    red[w] = argmax_neutral();
    if (any) {
      ++waves_in;
      std::vector<Best> b(LANES);
      for (int l = 0; l < LANES; ++l) b[l] = argmax_entry(lb[w * LANES + l].m, gm, lb[w * LANES + l].mi);
      red[w] = butterfly(b);
    }
  }
  Best vf = red[0];
  for (int w = 1; w < WAVES; ++w) vf = better(vf, red[w]);
  if (!same(vf, parent) || !same(vf, seq) || waves_in < 1) {
    std::printf("FAILED %s: value first {%a, %d}, parent {%a, %d}, sequential {%a, %d}, waves in %d\n", name, vf.v, vf.idx, parent.v,
                parent.idx, seq.v, seq.idx, waves_in);
    ++failures;
  }
}

}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  std::mt19937 rng(20261020);
  std::vector<int> idx(TOTAL);
  int cases = 0;
  for (int rep = 0; rep < 400; ++rep) {
    // distinct shifted indices in a shuffled order: the smaller index is not always in the earlier lane or wave
    for (int i = 0; i < TOTAL; ++i) idx[i] = i;
    if (rep & 1) std::shuffle(idx.begin(), idx.end(), rng);
    std::vector<float> base(TOTAL);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    for (float& x : base) x = u(rng);
    auto at = [&](int w, int l, int c) { return ((size_t)w * LANES + l) * CAND + c; };
    auto rnd = [&](int n) { return (int)(rng() % (unsigned)n); };
    std::vector<float> v;
    // one maximum
    v = base;
    v[at(rnd(4), rnd(64), rnd(16))] = 2.f;
    check("one maximum", v, idx), ++cases;
    // a tie inside one lane, across lanes of a wave, across waves
    v = base;
    {
      const int w = rnd(4), l = rnd(64);
      v[at(w, l, 3)] = v[at(w, l, 11)] = 2.f;
    }
    check("tie in a lane", v, idx), ++cases;
    v = base;
    {
      const int w = rnd(4);
      v[at(w, rnd(32), rnd(16))] = v[at(w, 32 + rnd(32), rnd(16))] = 2.f;
    }
    check("tie across lanes", v, idx), ++cases;
    v = base;
    for (int w = 0; w < 4; ++w)
      if (w == rep % 4 || rnd(2)) v[at(w, rnd(64), rnd(16))] = 2.f;
    check("tie across waves", v, idx), ++cases;
    // +0 against -0 as the maximum of a non-positive surface: the index decides, the winner's own bits are kept
    for (float& x : (v = base)) x = -std::fabs(x) - 0.5f;
    v[at(rnd(4), rnd(64), rnd(16))] = 0.f;
    v[at(rnd(4), rnd(64), rnd(16))] = -0.f;
    v[at(rnd(4), rnd(64), rnd(16))] = rnd(2) ? 0.f : -0.f;
    check("+0 meets -0", v, idx), ++cases;
    // NaN scattered, whole NaN lanes, a NaN beside the maximum in its lane
    v = base;
    for (int i = 0; i < 200; ++i) v[(size_t)rnd(TOTAL)] = nan;
    {
      const int w = rnd(4), l = rnd(64), w2 = rnd(4), l2 = rnd(64);
      for (int c = 0; c < CAND; ++c) v[at(w, l, c)] = nan;
      v[at(w2, l2, 5)] = 2.f;
      v[at(w2, l2, 6)] = nan;
    }
    check("NaN candidates", v, idx), ++cases;
    // -inf everywhere but a few places; everywhere; all NaN; NaN and -inf only
    for (float& x : (v = base)) x = -inf;
    check("all -inf", v, idx), ++cases;
    v[at(rnd(4), rnd(64), rnd(16))] = -3.e38f;
    check("one finite value", v, idx), ++cases;
    for (float& x : v) x = nan;
    check("all NaN", v, idx), ++cases;
    for (int i = 0; i < 50; ++i) v[(size_t)rnd(TOTAL)] = -inf;
    check("NaN and -inf", v, idx), ++cases;
    // a flat surface (every candidate equal) and a two-level one (the masked zeros of the OpenCL peak model)
    for (float& x : (v = base)) x = 0.25f;
    check("flat", v, idx), ++cases;
    for (float& x : (v = base)) x = x > 0.9f ? 0.f : -std::fabs(x) - 1.f;
    check("many equal zeros", v, idx), ++cases;
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("argmax select ok: %d arrays of %d x %d x %d candidates\n", cases, WAVES, LANES, CAND);
  return 0;
}
