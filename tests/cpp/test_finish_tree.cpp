// Host test of csrc/pc_finish_tree.hpp: finish_tree must return, bit for bit, what lane 0 of a wave holds after wave_sum3 -- simulated
// here as it runs on the device: six levels OFF = 32, 16, 8, 4, 2, 1, every one of the 64 lanes adding the value of lane l ^ OFF to its own.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "pc_finish_tree.hpp"

using mof::Sum3;

static uint64_t bits(double x) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  return u;
}

static Sum3 simulate(const Sum3* leaf) {
  Sum3 a[64], b[64];
  for (int l = 0; l < 64; ++l) a[l] = leaf[l];
  for (int off = 32; off >= 1; off >>= 1) {
    for (int l = 0; l < 64; ++l) b[l] = Sum3{a[l].cx + a[l ^ off].cx, a[l].cy + a[l ^ off].cy, a[l].sum + a[l ^ off].sum};
    for (int l = 0; l < 64; ++l) a[l] = b[l];
  }
  return a[0];
}

static int check(const char* what, const Sum3* leaf) {
  const Sum3 want = simulate(leaf), got = mof::finish_tree([&](int l) { return leaf[l]; });
  if (bits(want.cx) == bits(got.cx) && bits(want.cy) == bits(got.cy) && bits(want.sum) == bits(got.sum)) return 0;
  std::printf("MISMATCH %s: got %a %a %a want %a %a %a\n", what, got.cx, got.cy, got.sum, want.cx, want.cy, want.sum);
  return 1;
}

int main() {
  std::mt19937_64 rng(20261022);
  std::uniform_real_distribution<double> wide(-1e6, 1e6), unit(0.0, 1.0);
  int bad = 0, cases = 0;
  Sum3 leaf[64];
  // every leaf is asked for exactly once
  {
    int seen[64] = {0};
    mof::finish_tree([&](int l) { ++seen[l]; return Sum3{0, 0, 0}; });
    for (int l = 0; l < 64; ++l) bad += seen[l] != 1;
    ++cases;
  }
  for (int rep = 0; rep < 2000; ++rep, ++cases) {  // random leaves of mixed magnitude: a different pairing rounds differently
    for (auto& s : leaf) s = Sum3{wide(rng) * unit(rng), wide(rng), unit(rng) * 1e-9 + wide(rng) * (rep & 1)};
    bad += check("random", leaf);
  }
  for (int rep = 0; rep < 500; ++rep, ++cases) {  // the kernel's shape: 25 values times small integers, zeros of either sign behind them
    for (int l = 0; l < 64; ++l) {
      const double v = l < 25 ? (double)(float)unit(rng) : 0.0;
      const int xs = (int)(rng() % 70) - 3, ys = (int)(rng() % 70) - 3;
      leaf[l] = Sum3{(double)xs * v, (double)ys * v, v};
    }
    bad += check("window", leaf);
  }
  for (int sign = 0; sign < 4; ++sign, ++cases) {  // leaves of +0.0 and -0.0 only: -0 + -0 = -0, anything else +0
    for (int l = 0; l < 64; ++l) {
      const bool neg = sign == 0 ? false : sign == 1 ? true : sign == 2 ? (l & 1) : (l >= 32);
      leaf[l] = Sum3{neg ? -0.0 : 0.0, (l % 3) ? -0.0 : 0.0, neg ? -0.0 : 0.0};
    }
    bad += check("zeros", leaf);
  }
  for (int one = 0; one < 64; ++one, ++cases) {  // a single leaf among signed zeros
    for (int l = 0; l < 64; ++l) leaf[l] = Sum3{(l & 2) ? -0.0 : 0.0, -0.0, 0.0};
    leaf[one] = Sum3{-3.25 * (one + 1), 0x1.fffffep-1 * one, 0x1.000002p-20};
    bad += check("single", leaf);
  }
  if (bad) {
    std::printf("finish tree: %d of %d cases FAILED\n", bad, cases);
    return 1;
  }
  std::printf("finish tree ok: %d cases\n", cases);
  return 0;
}
