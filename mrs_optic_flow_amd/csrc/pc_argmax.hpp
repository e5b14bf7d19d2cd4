// pc_argmax.hpp -- the selection rule of the peak search: (value, shifted index) pairs, their order, and what a lane contributes when the
// value is reduced before the index ("value first", pc_kernel.hip). Plain C++ with no HIP header, so that a host program can call the very
// functions the kernels inline (tests/cpp/test_argmax_select.cpp).
#pragma once

#if defined(__HIPCC__)
#define MOF_ARGMAX_FN __host__ __device__ __forceinline__
#else
#define MOF_ARGMAX_FN inline
#endif

namespace mof {
namespace {

struct Best {
  float v;
  int idx;
};
MOF_ARGMAX_FN Best better(Best a, Best b) {
  // first maximum in row-major order of the fft-shifted surface (cv::minMaxLoc)
  return (b.v > a.v || (b.v == a.v && b.idx < a.idx)) ? b : a;
}

// what a fold starts from and what a lane (or a wave) without a candidate carries: loses to every value, ties with nothing but itself
MOF_ARGMAX_FN Best argmax_neutral() { return Best{-__builtin_huge_valf(), 0x7fffffff}; }

// One candidate of a lane whose maximum is m (never NaN: an fmaxf chain seeded with -inf): the smallest shifted index among the
// candidates that attain m. A NaN candidate equals nothing and never enters.
MOF_ARGMAX_FN int argmax_first_index(int mi, float cand, float m, int idx) {
  const int c = cand == m ? idx : 0x7fffffff;
  return mi < c ? mi : c;
}

// Value first. gm = the maximum of every lane's m (fmaxf, so gm >= m for every lane and gm == m for one at least). A lane with m != gm
// lies strictly below the maximum and enters the fold as the neutral element; a lane with m == gm enters with ITS OWN m, not with gm:
// +0 and -0 compare equal, the index decides between them, and the value that is stored afterwards (the quality's peak) must be the
// winner's bits.
//   Same result as folding every lane's (m, mi) with better(), whatever the order of the fold:
//   * better() picks by value first, then by the smaller index; m is never NaN, so apart from the tie of two identical neutral pairs the
//     fold's result is the one pair that is largest in that order, W, and W.v == gm (as a comparison);
//   * a pair with v < gm loses to W and to every other pair with v == gm wherever it stands in the fold, so replacing it with the
//     neutral element -- which loses to them as well, gm > -inf in this case -- changes no comparison that W or its competitors win;
//   * gm == -inf: every lane has m == -inf == gm, none is replaced, the fold is the parent's own (all-NaN or all -inf surfaces end as
//     {-inf, 0x7fffffff} or as the first -inf, as before);
//   * ties at gm, inside a lane, across lanes and across waves, are all still in the fold with their own indices.
MOF_ARGMAX_FN Best argmax_entry(float m, float gm, int mi) { return m == gm ? Best{m, mi} : argmax_neutral(); }

// A lone lane. holders = the wave's ballot of m == gm, bit l for lane l. Where exactly ONE bit is set, the wave's fold of the entries above
// -- in any order, the xor butterfly of wave_best among them -- ends in every lane with that lane's own (m, mi), so the wave may read the
// pair out of lane argmax_lone_lane(holders) and skip the fold:
//   * one bit means gm > -inf: with gm == -inf every lane has m == -inf == gm (m >= -inf, never NaN) and all 64 bits are set;
//   * so the 63 other entries are the neutral pair {-inf, 0x7fffffff}, whose value lies strictly below m. better(H, neutral) and
//     better(neutral, H) both return H, the holder's pair, by the value alone: the index is not asked and +0 / -0 do not meet, since
//     a lane that held the other zero would compare equal to gm and set a second bit; better(neutral, neutral) is the neutral pair;
//   * every lane of a butterfly level therefore carries H or the neutral pair, and a lane carries H after the level exactly where it or
//     its partner did before: the set of lanes with H doubles at each of the six levels, from 1 to 64.
// The pair handed over is the lane's own m -- its bits, not gm's. Any other count (two lanes of the wave tie, a +0 beside a -0, the flat
// and the all-NaN surfaces) keeps the fold. tests/cpp/test_argmax_lone.cpp holds the rule to the butterfly.
MOF_ARGMAX_FN bool argmax_lone_holder(unsigned long long holders) { return __builtin_popcountll(holders) == 1; }
MOF_ARGMAX_FN int argmax_lone_lane(unsigned long long holders) { return __builtin_ctzll(holders); }  // (holders != 0)

}  // namespace
}  // namespace mof
