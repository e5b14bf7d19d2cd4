// Self-test of the cross-lane helpers of pc_common.hpp (lane_xor, wave_best, wave_max, wave_sum3): ONE launch of ONE wave that
// compares them with __shfl_xor and with serial scans, and counts the mismatches. Not part of the public interface
// (not in mof.h): tests/test_gpu_wave_ops.py calls it through ctypes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_mem.hpp"
#include "pc_common.hpp"

namespace mof {
namespace {

__device__ __forceinline__ bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }
__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

template <int OFF>
__device__ __forceinline__ int check_xor(int lane) {
  const uint32_t u = 0x9e3779b9u * (uint32_t)(lane + 1) ^ (uint32_t)lane << 24;
  const int i = (int)~u;
  const float f = (float)(lane - 31) * 1.25f;
  const double d = __longlong_as_double((long long)((uint64_t)(0x3ff00000u + (uint32_t)lane * 0x1357u) << 32 | u));
  int bad = 0;
  bad += lane_xor<OFF>(u) != (uint32_t)__shfl_xor((int)u, OFF, 64);
  bad += lane_xor<OFF>(i) != __shfl_xor(i, OFF, 64);
  bad += !same_bits(lane_xor<OFF>(f), __shfl_xor(f, OFF, 64));
  bad += !same_bits(lane_xor<OFF>(d), __shfl_xor(d, OFF, 64));
  return bad;
}

// wave_best (1) against better() folded serially over lanes 0 .. 63, every lane holding the result: on the lanes' values
// as the kernels' passes form them (seeded with {-inf, 0x7fffffff}, a value enters by better(): a NaN never does);
// (2) against the __shfl_xor butterfly it replaces, lane by lane, on the raw values -- a NaN operand makes better()
// asymmetric and the butterfly's result lane-dependent, and the same bits are wanted there too
__device__ __forceinline__ int check_best(float v, int lane, Best* lds) {
  const Best raw = {v, lane * 3 + 5};
  const Best mine = better(Best{-__builtin_huge_valf(), 0x7fffffff}, raw);
  lds[lane] = mine;
  wave_sync();
  Best ref = lds[0];
#pragma unroll 1
  for (int l = 1; l < 64; ++l) ref = better(ref, lds[l]);
  wave_sync();
  const Best got = wave_best(mine);
  int bad = (!same_bits(got.v, ref.v)) + (got.idx != ref.idx);
  Best old = raw;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const Best o = {__shfl_xor(old.v, off, 64), __shfl_xor(old.idx, off, 64)};
    old = better(old, o);
  }
  const Best neu = wave_best(raw);
  return bad + (!same_bits(neu.v, old.v)) + (neu.idx != old.idx);
}

// wave_max (the value-only fold of the value-first arg-max) against fmaxf folded serially over lanes 0 .. 63 and against the
// __shfl_xor butterfly, every lane holding the result. Values as the kernels feed it: never NaN. Compared as VALUES (==), which is
// how the kernel uses it: where +0 and -0 are both the maximum either may come out.
__device__ __forceinline__ int check_max(float v, int lane, Best* lds) {
  lds[lane] = Best{v, lane};
  wave_sync();
  float ref = lds[0].v;
#pragma unroll 1
  for (int l = 1; l < 64; ++l) ref = fmaxf(ref, lds[l].v);
  wave_sync();
  float old = v;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) old = fmaxf(old, __shfl_xor(old, off, 64));
  const float got = wave_max(v);
  return !(got == ref) + !(got == old);
}

// wave_sum3 against the __shfl_xor butterfly it replaces, bit for bit, on `n` non-zero lanes of mixed magnitude and sign
template <int TOP>
__device__ __forceinline__ int check_sum3(int n, int lane) {
  const double val = lane < n ? (double)((lane % 7 - 3) * 1.0e-3f + 1.0f / (float)(lane + 1)) * ((lane & 5) == 1 ? -4096.0 : 1.0) : 0.0;
  double cx = (double)(lane % 7 - 3) * val, cy = (double)(lane / 7 + 29) * val, sum = val;
  double rx = cx, ry = cy, rs = sum;
  wave_sum3<TOP>(cx, cy, sum);
#pragma unroll
  for (int off = TOP; off > 0; off >>= 1) {
    rx += __shfl_xor(rx, off, 64);
    ry += __shfl_xor(ry, off, 64);
    rs += __shfl_xor(rs, off, 64);
  }
  int bad = (!same_bits(cx, rx)) + (!same_bits(cy, ry)) + (!same_bits(sum, rs));
  bad += !same_bits(wave_sum<TOP>(val), rs);
  return bad;
}

__global__ __launch_bounds__(64) void wave_ops_selftest_kernel(int* mismatches) {
  __shared__ Best lds[64];
  const int lane = (int)threadIdx.x;
  const float ninf = -__builtin_huge_valf(), nan = __builtin_nanf("");
  int bad = 0;
  bad += check_xor<32>(lane) + check_xor<16>(lane) + check_xor<8>(lane) + check_xor<4>(lane) + check_xor<2>(lane) + check_xor<1>(lane);
  bad += check_best((float)((lane * 37) % 64) - 20.5f, lane, lds);             // distinct values
  bad += check_best(lane == 9 || lane == 13 ? 7.f : (float)(lane % 5), lane, lds);  // a tie on two lanes: the smaller index wins
  bad += check_best(lane == 40 || lane == 3 ? 7.f : (float)(lane % 5), lane, lds);  // a tie across the 32-lane halves
  bad += check_best(ninf, lane, lds);                                            // all -inf
  bad += check_best(lane == 21 ? nan : (float)(63 - lane), lane, lds);           // one NaN lane
  {                                                                              // all NaN: idx stays 0x7fffffff
    bad += check_best(nan, lane, lds);
    bad += wave_best(better(Best{ninf, 0x7fffffff}, Best{nan, lane})).idx != 0x7fffffff;
  }
  bad += check_max((float)((lane * 37) % 64) - 20.5f, lane, lds);                // distinct values, the maximum in each half in turn
  bad += check_max((float)(((lane + 32) * 37) % 64) - 20.5f, lane, lds);
  bad += check_max(lane == 40 || lane == 3 ? 7.f : (float)(lane % 5), lane, lds);  // a tie across the 32-lane halves
  bad += check_max(lane == 17 ? 0.f : (lane == 50 ? -0.f : -1.f - (float)lane), lane, lds);  // +0 and -0 are the maximum
  bad += check_max(ninf, lane, lds);                                             // all -inf
  bad += check_max(lane == 63 ? -3.e38f : ninf, lane, lds);                      // one finite value in the last lane
  bad += check_sum3<32>(25, lane) + check_sum3<32>(49, lane) + check_sum3<16>(25, lane);
  if (bad) atomicAdd(mismatches, bad);
}

}  // namespace
}  // namespace mof

// number of mismatches (0 = pass), or -1 when the device could not be used
extern "C" int mof_selftest_wave_ops(void) {
  mof::DevMem<int> d;
  int h = -1;
  if (d.alloc(1) != hipSuccess) return -1;
  bool ok = hipMemset(d, 0, sizeof(int)) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(mof::wave_ops_selftest_kernel, dim3(1), dim3(64), 0, 0, d.get());
    ok = hipGetLastError() == hipSuccess && hipMemcpy(&h, d, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
  }
  return ok ? h : -1;
}
