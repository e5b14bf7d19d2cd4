// pc_finish_tree.hpp -- the three fp64 sums of a peak tail as ONE lane forms them (pc_finish_kernel, pc_kernel.hip): what lane 0 of a
// wave holds after wave_sum3 (pc_common.hpp), whose levels 32, 16, 8, 4, 2, 1 each run a[l] += a[l ^ OFF] in all 64 lanes. Lane 0 only
// ever consumes lanes below OFF, and there l ^ OFF = l + OFF with the lane's own value as the left operand:
//   g(i, 64) = leaf(i);   g(i, L) = g(i, 2 L) + g(i + L, 2 L);   lane 0 ends with g(0, 1)
// -- the same additions on the same operands in the same order, so the same bits. Every leaf is asked for once, with a compile-time
// index. Plain C++ with no HIP header, so that a host program can call the very function the kernel inlines
// (tests/cpp/test_finish_tree.cpp).
#pragma once

#if defined(__HIPCC__)
#define MOF_FINISH_FN __host__ __device__ __forceinline__
#else
#define MOF_FINISH_FN inline
#endif

namespace mof {
namespace {

struct Sum3 {
  double cx, cy, sum;
};

// leaf(l) -> Sum3 of virtual lane l, 0 <= l < 64
template <int I = 0, int L = 1, class Leaf>
MOF_FINISH_FN Sum3 finish_tree(const Leaf& leaf) {
  if constexpr (L == 64) {
    return leaf(I);
  } else {
    const Sum3 a = finish_tree<I, 2 * L>(leaf), b = finish_tree<I + L, 2 * L>(leaf);
    return Sum3{a.cx + b.cx, a.cy + b.cy, a.sum + b.sum};
  }
}

}  // namespace
}  // namespace mof
