// pc_common.hpp -- device helpers shared by the phase-correlation kernels (pc_kernel.hip: power-of-two patch
// sizes; pc_kernel_mixed.hip: 120 = 15 x 8; sr_kernel.hip: whole frames of 240 / 256 / 480): complex arithmetic, radix butterflies, wave-local LDS ordering, the
// normalised cross-power spectrum of one bin and the centroid / gate tail. Reference citations as in pc_kernel.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mof_kernels.h"
#include "pc_argmax.hpp"

namespace mof {
namespace {

struct cf {
  float x, y;
};

__device__ __forceinline__ cf cmul(cf a, cf b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cf cadd(cf a, cf b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cf csub(cf a, cf b) { return {a.x - b.x, a.y - b.y}; }
// multiply by -i (a quarter turn of the forward kernel e^{-2 pi i k/N})
__device__ __forceinline__ cf mul_mi(cf a) { return {a.y, -a.x}; }

template <int R>
__device__ __forceinline__ void butterfly(cf* v);

template <>
__device__ __forceinline__ void butterfly<2>(cf* v) {
  cf a = v[0], b = v[1];
  v[0] = cadd(a, b);
  v[1] = csub(a, b);
}

template <>
__device__ __forceinline__ void butterfly<4>(cf* v) {
  cf a = cadd(v[0], v[2]), b = csub(v[0], v[2]);
  cf c = cadd(v[1], v[3]), d = mul_mi(csub(v[1], v[3]));
  v[0] = cadd(a, c);
  v[1] = cadd(b, d);
  v[2] = csub(a, c);
  v[3] = csub(b, d);
}

template <>
__device__ __forceinline__ void butterfly<8>(cf* v) {
  const float h = 0.70710678118654752440f;
  cf e[4] = {v[0], v[2], v[4], v[6]};
  cf o[4] = {v[1], v[3], v[5], v[7]};
  butterfly<4>(e);
  butterfly<4>(o);
  cf w1 = {h * (o[1].x + o[1].y), h * (o[1].y - o[1].x)};   // o1 * e^{-i pi/4}
  cf w2 = mul_mi(o[2]);                                     // o2 * e^{-i pi/2}
  cf w3 = {h * (o[3].y - o[3].x), -h * (o[3].x + o[3].y)};  // o3 * e^{-3 i pi/4}
  v[0] = cadd(e[0], o[0]);
  v[4] = csub(e[0], o[0]);
  v[1] = cadd(e[1], w1);
  v[5] = csub(e[1], w1);
  v[2] = cadd(e[2], w2);
  v[6] = csub(e[2], w2);
  v[3] = cadd(e[3], w3);
  v[7] = csub(e[3], w3);
}

// butterfly<8> of v_k = a_k t_k (t_0 = 1; tw[k-1] = t_k): the twiddle products ride the first radix-2 layer as FMAs
// (x + t y needs 4 FMAs, x - t y = 2 x - (x + t y) two more) -- 8 instructions fewer than 7 complex multiplies followed
// by butterfly<8>, the same value up to rounding.
__device__ __forceinline__ void butterfly8_tw(cf* v, const cf* tw) {
  auto fma_c = [](cf x, cf t, cf y) -> cf {  // x + t * y
    return {__builtin_fmaf(t.x, y.x, __builtin_fmaf(-t.y, y.y, x.x)), __builtin_fmaf(t.x, y.y, __builtin_fmaf(t.y, y.x, x.y))};
  };
  auto twice_minus = [](cf x, cf s) -> cf { return {__builtin_fmaf(2.f, x.x, -s.x), __builtin_fmaf(2.f, x.y, -s.y)}; };
  const float h = 0.70710678118654752440f;
  // even half: e = (a0, t2 a2, t4 a4, t6 a6)
  const cf A = fma_c(v[0], tw[3], v[4]), B = twice_minus(v[0], A);
  const cf u2 = cmul(v[2], tw[1]);
  const cf C = fma_c(u2, tw[5], v[6]), Dm = twice_minus(u2, C);
  const cf D = mul_mi(Dm);
  const cf e0 = cadd(A, C), e1 = cadd(B, D), e2 = csub(A, C), e3 = csub(B, D);
  // odd half: o = (t1 a1, t3 a3, t5 a5, t7 a7)
  const cf u1 = cmul(v[1], tw[0]);
  const cf A1 = fma_c(u1, tw[4], v[5]), B1 = twice_minus(u1, A1);
  const cf u3 = cmul(v[3], tw[2]);
  const cf C1 = fma_c(u3, tw[6], v[7]), Dm1 = twice_minus(u3, C1);
  const cf D1 = mul_mi(Dm1);
  const cf o0 = cadd(A1, C1), o1 = cadd(B1, D1), o2 = csub(A1, C1), o3 = csub(B1, D1);
  const cf w1 = {h * (o1.x + o1.y), h * (o1.y - o1.x)};
  const cf w2 = mul_mi(o2);
  const cf w3 = {h * (o3.y - o3.x), -h * (o3.x + o3.y)};
  v[0] = cadd(e0, o0);
  v[4] = csub(e0, o0);
  v[1] = cadd(e1, w1);
  v[5] = csub(e1, w1);
  v[2] = cadd(e2, w2);
  v[6] = csub(e2, w2);
  v[3] = cadd(e3, w3);
  v[7] = csub(e3, w3);
}

// (a raised or lowered issue priority, s_setprio, inside the radix-16 butterflies against the LDS phases around them: butterflies first
// -4 .. -5 % at c2 and -7 % at c4, LDS phases first +-0, profiles/r06_bfly_prio_ab.txt -- none is set)
template <>
__device__ __forceinline__ void butterfly<16>(cf* v) {
  // 16 = 4 x 4: four radix-4 over n1 (stride 4), twiddle W16^{n2 k1}, four radix-4 over n2
  const float c1 = 0.92387953251128675613f, s1 = 0.38268343236508977173f, h = 0.70710678118654752440f;
  cf t[4][4];
#pragma unroll
  for (int n2 = 0; n2 < 4; ++n2) {
    cf a[4] = {v[n2], v[n2 + 4], v[n2 + 8], v[n2 + 12]};
    butterfly<4>(a);
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) t[n2][k1] = a[k1];
  }
  // W16^m = (cos(pi m/8), -sin(pi m/8))
  const cf w[10] = {{1.f, 0.f}, {c1, -s1}, {h, -h}, {s1, -c1}, {0.f, -1.f}, {-s1, -c1}, {-h, -h}, {-c1, -s1}, {-1.f, 0.f},
                    {-c1, s1}};
#pragma unroll
  for (int k1 = 0; k1 < 4; ++k1) {
    cf a[4];
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2) a[n2] = (n2 * k1 == 0) ? t[n2][k1] : cmul(t[n2][k1], w[n2 * k1]);
    butterfly<4>(a);
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) v[k1 + 4 * k2] = a[k2];
  }
}

__device__ __forceinline__ void butterfly3(cf* a) {
  const float s3 = 0.86602540378443864676f;  // sin(2 pi / 3)
  const cf s = cadd(a[1], a[2]), d = csub(a[1], a[2]);
  const cf m = {a[0].x - 0.5f * s.x, a[0].y - 0.5f * s.y};
  a[0] = cadd(a[0], s);
  a[1] = {m.x + s3 * d.y, m.y - s3 * d.x};
  a[2] = {m.x - s3 * d.y, m.y + s3 * d.x};
}

__device__ __forceinline__ void butterfly5(cf* a) {
  const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;  // cos(2pi/5), cos(4pi/5)
  const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;   // sin(2pi/5), sin(4pi/5)
  const cf s14 = cadd(a[1], a[4]), d14 = csub(a[1], a[4]), s23 = cadd(a[2], a[3]), d23 = csub(a[2], a[3]);
  const cf p1 = {a[0].x + c1 * s14.x + c2 * s23.x, a[0].y + c1 * s14.y + c2 * s23.y};
  const cf p2 = {a[0].x + c2 * s14.x + c1 * s23.x, a[0].y + c2 * s14.y + c1 * s23.y};
  const cf q1 = {s1 * d14.x + s2 * d23.x, s1 * d14.y + s2 * d23.y};
  const cf q2 = {s2 * d14.x - s1 * d23.x, s2 * d14.y - s1 * d23.y};
  a[0] = {a[0].x + s14.x + s23.x, a[0].y + s14.y + s23.y};
  a[1] = {p1.x + q1.y, p1.y - q1.x};  // p1 - i q1
  a[4] = {p1.x - q1.y, p1.y + q1.x};  // p1 + i q1
  a[2] = {p2.x + q2.y, p2.y - q2.x};
  a[3] = {p2.x - q2.y, p2.y + q2.x};
}

// 15-point DFT: n = 5 n1 + n2, k = k1 + 3 k2 (radix 3, twiddle W15^{n2 k1}, radix 5)
__device__ __forceinline__ void butterfly15(cf* v) {
  // W15^m = (cos(2 pi m / 15), -sin(2 pi m / 15)), m = 0..8
  const cf w15[9] = {{1.f, 0.f},
                     {0.91354545764260089550f, -0.40673664307580020775f},
                     {0.66913060635885821383f, -0.74314482547739423501f},
                     {0.30901699437494742410f, -0.95105651629515357212f},
                     {-0.10452846326765347140f, -0.99452189536827333692f},
                     {-0.5f, -0.86602540378443864676f},
                     {-0.80901699437494742410f, -0.58778525229247312917f},
                     {-0.97814760073380563793f, -0.20791169081775933710f},
                     {-0.97814760073380563793f, 0.20791169081775933710f}};
  cf t[5][3];
#pragma unroll
  for (int n2 = 0; n2 < 5; ++n2) {
    cf a[3] = {v[n2], v[5 + n2], v[10 + n2]};
    butterfly3(a);
#pragma unroll
    for (int k1 = 0; k1 < 3; ++k1) t[n2][k1] = (n2 * k1 == 0) ? a[k1] : cmul(a[k1], w15[n2 * k1]);
  }
#pragma unroll
  for (int k1 = 0; k1 < 3; ++k1) {
    cf b[5] = {t[0][k1], t[1][k1], t[2][k1], t[3][k1], t[4][k1]};
    butterfly5(b);
#pragma unroll
    for (int k2 = 0; k2 < 5; ++k2) v[k1 + 3 * k2] = b[k2];
  }
}

// 32-point DFT: n = 8 n1 + n2, k = k1 + 4 k2 (eight radix-4 over n1, twiddle W32^{n2 k1}, four radix-8 over n2)
__device__ __forceinline__ void butterfly32(cf* v) {
  // W32^m = (cos(pi m / 16), -sin(pi m / 16)), m = 0..21
  const float c1 = 0.98078528040323044913f, s1 = 0.19509032201612826785f;  // pi/16
  const float c2 = 0.92387953251128675613f, s2 = 0.38268343236508977173f;  // pi/8
  const float c3 = 0.83146961230254523708f, s3 = 0.55557023301960222474f;  // 3 pi/16
  const float h = 0.70710678118654752440f;
  const cf w[22] = {{1.f, 0.f}, {c1, -s1}, {c2, -s2}, {c3, -s3}, {h, -h}, {s3, -c3}, {s2, -c2}, {s1, -c1}, {0.f, -1.f},
                    {-s1, -c1}, {-s2, -c2}, {-s3, -c3}, {-h, -h}, {-c3, -s3}, {-c2, -s2}, {-c1, -s1}, {-1.f, 0.f},
                    {-c1, s1}, {-c2, s2}, {-c3, s3}, {-h, h}, {-s3, c3}};
  cf t[8][4];
#pragma unroll
  for (int n2 = 0; n2 < 8; ++n2) {
    cf a[4] = {v[n2], v[8 + n2], v[16 + n2], v[24 + n2]};
    butterfly<4>(a);
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) t[n2][k1] = (n2 * k1 == 0) ? a[k1] : cmul(a[k1], w[n2 * k1]);
  }
#pragma unroll
  for (int k1 = 0; k1 < 4; ++k1) {
    cf b[8] = {t[0][k1], t[1][k1], t[2][k1], t[3][k1], t[4][k1], t[5][k1], t[6][k1], t[7][k1]};
    butterfly<8>(b);
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) v[k1 + 4 * k2] = b[k2];
  }
}

// Orders the LDS traffic of the lanes of ONE wave (a wave's DS instructions execute in order);
// emits no instruction, only stops the compiler from moving LDS accesses across it.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 8-byte LDS read kept as ONE ds_read_b64: hipcc otherwise fuses neighbouring reads into ds_read2_b64 /
// ds_read2st64_b64, which move half the bytes per LDS cycle on gfx950 (MI355X_MICROARCH.md, LDS table).
__device__ __forceinline__ cf lds_read(const cf* p) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef const volatile f2 __attribute__((address_space(3))) * lds_f2_ptr;
  const f2 t = *(lds_f2_ptr)(p);
  return {t.x, t.y};
}

// (Best, better() and the value-first selection rule: pc_argmax.hpp, host-callable)

// ---- cross-lane exchange on the VALU -------------------------------------------------------------------------------
// lane_xor<OFF>(x) = the x of lane (lane ^ OFF), OFF in {32, 16, 8, 4, 2, 1}: what __shfl_xor(x, OFF, 64) returns, without
// the trip through the wave's in-order LDS queue that ds_bpermute_b32 takes (the peak tails are chains of 12 - 14
// dependent exchanges at the end of every patch, on a CU whose LDS pipe is busy with the other workgroups' tiles):
//   32: v_permlane32_swap   16: v_permlane16_swap   8: DPP row_ror:8   4: DPP row_shl:4 | row_shr:4 under complementary
//   bank masks   2, 1: DPP quad_perm
// CONTRACT: ALL 64 LANES ACTIVE. DPP and the swaps keep the old value where the source lane is inactive, ds_bpermute
// returns 0 there: a call site inside lane-divergent control flow stays on __shfl_xor.
__device__ __forceinline__ int wave_lane() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

template <int OFF>
__device__ __forceinline__ uint32_t lane_xor(uint32_t x) {
  static_assert(OFF == 32 || OFF == 16 || OFF == 8 || OFF == 4 || OFF == 2 || OFF == 1, "one butterfly level");
  if constexpr (OFF == 32) {
    // (x, x) -> r[0] = {x[0..31], x[0..31]}, r[1] = {x[32..63], x[32..63]}: the partner is picked explicitly (better() is
    // not symmetric in its operands when one is NaN, so "op(r[0], r[1])" would not be the same butterfly)
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return (wave_lane() & 32) ? r[0] : r[1];
  } else if constexpr (OFF == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);  // the same, by bit 4 of the lane
    return (wave_lane() & 16) ? r[0] : r[1];
  } else if constexpr (OFF == 8) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x128, 0xf, 0xf, false);  // row_ror:8
  } else if constexpr (OFF == 4) {
    const int lo = __builtin_amdgcn_update_dpp((int)x, (int)x, 0x104, 0xf, 0x5, false);  // row_shl:4 -> lanes 0-3, 8-11 of a row
    return (uint32_t)__builtin_amdgcn_update_dpp(lo, (int)x, 0x114, 0xf, 0xa, false);    // row_shr:4 -> lanes 4-7, 12-15
  } else if constexpr (OFF == 2) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x4e, 0xf, 0xf, false);  // quad_perm:[2,3,0,1]
  } else {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0xb1, 0xf, 0xf, false);  // quad_perm:[1,0,3,2]
  }
}
template <int OFF>
__device__ __forceinline__ int lane_xor(int x) { return (int)lane_xor<OFF>((uint32_t)x); }
template <int OFF>
__device__ __forceinline__ float lane_xor(float x) { return __uint_as_float(lane_xor<OFF>(__float_as_uint(x))); }
template <int OFF>
__device__ __forceinline__ double lane_xor(double x) {
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  const uint32_t lo = lane_xor<OFF>((uint32_t)u), hi = lane_xor<OFF>((uint32_t)(u >> 32));
  return __longlong_as_double((long long)((uint64_t)hi << 32 | lo));
}

// The butterflies of the peak tails, levels TOP, TOP/2 .. 1 with the partners and the operand order of the __shfl_xor
// loops they replace (same bits). TOP < 32 where only the first 2 TOP lanes hold non-zero terms.
template <int TOP = 32, class T>
__device__ __forceinline__ T wave_sum(T v) {
  if constexpr (TOP >= 32) v += lane_xor<32>(v);
  if constexpr (TOP >= 16) v += lane_xor<16>(v);
  v += lane_xor<8>(v);
  v += lane_xor<4>(v);
  v += lane_xor<2>(v);
  v += lane_xor<1>(v);
  return v;
}
template <int OFF>
__device__ __forceinline__ void wave_sum3_level(double& a, double& b, double& c) {
  const double oa = lane_xor<OFF>(a), ob = lane_xor<OFF>(b), oc = lane_xor<OFF>(c);
  a += oa;
  b += ob;
  c += oc;
}
template <int TOP = 32>
__device__ __forceinline__ void wave_sum3(double& a, double& b, double& c) {
  if constexpr (TOP >= 32) wave_sum3_level<32>(a, b, c);
  if constexpr (TOP >= 16) wave_sum3_level<16>(a, b, c);
  wave_sum3_level<8>(a, b, c);
  wave_sum3_level<4>(a, b, c);
  wave_sum3_level<2>(a, b, c);
  wave_sum3_level<1>(a, b, c);
}
template <int OFF>
__device__ __forceinline__ Best wave_best_level(Best b) {
  const Best o = {lane_xor<OFF>(b.v), lane_xor<OFF>(b.idx)};
  return better(b, o);
}
// every lane ends with the wave's first maximum (better())
__device__ __forceinline__ Best wave_best(Best b) {
  b = wave_best_level<32>(b);
  b = wave_best_level<16>(b);
  b = wave_best_level<8>(b);
  b = wave_best_level<4>(b);
  b = wave_best_level<2>(b);
  return wave_best_level<1>(b);
}

// The value alone: every lane ends with the wave's maximum. One exchange and one v_max_f32 per level -- fmaxf is symmetric in its
// operands where neither is NaN (the callers' values never are: they come out of fmaxf chains seeded with -inf), so the two swap levels
// take the maximum of the swap's two results and need no select on the lane's half. +0 and -0 compare equal and either may come out:
// the result is for comparing, not for storing.
__device__ __forceinline__ float wave_max(float v) {
  {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  }
  {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  }
  v = fmaxf(v, lane_xor<8>(v));
  v = fmaxf(v, lane_xor<4>(v));
  v = fmaxf(v, lane_xor<2>(v));
  return fmaxf(v, lane_xor<1>(v));
}

// cv::cvtColor(.., CV_RGB2GRAY) on 8-bit data (fixed point, yuv_shift 14): gray = (c0*R2Y + c1*G2Y + c2*B2Y + 2^13) >> 14
// with R2Y 4899, G2Y 9617, B2Y 1868. The node feeds it BGR8 data (optic_flow.cpp:1465 toCvCopy(BGR8), :1622
// CV_RGB2GRAY), so the blue byte gets the red weight -- reproduced as is.
__device__ __forceinline__ uint32_t rgb2gray_fixed(uint32_t c0, uint32_t c1, uint32_t c2) {
  return (c0 * 4899u + c1 * 9617u + c2 * 1868u + 8192u) >> 14;
}

// byte i of a little-endian dword array; the gray value of the interleaved pixel that starts there; four of them (u8x4) from byte 12 q on
__device__ __forceinline__ uint32_t byte_at(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }
__device__ __forceinline__ uint32_t gray_at(const uint32_t* w, int i) { return rgb2gray_fixed(byte_at(w, i), byte_at(w, i + 1), byte_at(w, i + 2)); }
__device__ __forceinline__ uint32_t gray4_at(const uint32_t* w, int q) {
  uint32_t packed = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) packed |= gray_at(w, 3 * (4 * q + b)) << (8 * b);
  return packed;
}

// 4 / 16 / 8 gray pixels (packed u8x4) from 12 / 48 / 24 interleaved bytes, any alignment, ONE load of that width each
__device__ __forceinline__ uint32_t gray4_from_bgr12(const uint8_t* p) {
  uint32_t w[3];
  __builtin_memcpy(w, p, 12);
  return gray4_at(w, 0);
}
__device__ __forceinline__ void gray16_from_bgr48(const uint8_t* p, uint32_t* g /*[4]*/) {
  uint32_t w[12];
  __builtin_memcpy(w, p, 48);
#pragma unroll
  for (int q = 0; q < 4; ++q) g[q] = gray4_at(w, q);
}
__device__ __forceinline__ void gray8_from_bgr24(const uint8_t* p, uint32_t* g /*[2]*/) {
  uint32_t w[6];
  __builtin_memcpy(w, p, 24);
#pragma unroll
  for (int q = 0; q < 2; ++q) g[q] = gray4_at(w, q);
}

// one pixel (row y, column x of the patch whose top-left pixel is `base`): as it is, through the node's CV_RGB2GRAY on BGR8 data (CH = 3),
// or the quarter-resolution pixel of the long-range mode (DS = 4: cv::resize(.., 1/4, 1/4), FftMethod.cpp:1931-1932) -- pc_field_kernel's front ends
template <int DS, int CH>
__device__ __forceinline__ uint32_t fetch_px(const uint8_t* __restrict__ base, size_t pitch, int y, int x) {
  if constexpr (DS == 4) {
    const uint8_t* r1 = base + (size_t)(4 * y + 1) * pitch + 4 * x;
    const uint8_t* r2 = r1 + pitch;
    return ((uint32_t)r1[1] + r1[2] + r2[1] + r2[2] + 2u) >> 2;
  } else if constexpr (CH == 3) {
    const uint8_t* p = base + (size_t)y * pitch + 3 * x;
    return rgb2gray_fixed(p[0], p[1], p[2]);
  } else {
    return base[(size_t)y * pitch + x];
  }
}

// four consecutive pixels x0 .. x0 + 3 of row y, one byte each (x0 + 3 inside the patch): ONE unaligned dword of a gray frame, three dwords
// of a BGR8 frame, or -- the long-range mode -- the 2 x 2 taps of four quarter-resolution pixels from two 16-byte runs of the frame rows
// 4 y + 1 and 4 y + 2 (cv::resize(1/4, INTER_LINEAR): columns 4 x + 1 and 4 x + 2)
template <int DS, int CH>
__device__ __forceinline__ uint32_t fetch_px4(const uint8_t* __restrict__ base, size_t pitch, int y, int x0) {
  if constexpr (DS == 4) {
    const uint8_t* r1 = base + (size_t)(4 * y + 1) * pitch + 4 * (size_t)x0;
    uint32_t w1[4], w2[4];
    __builtin_memcpy(w1, r1, 16);
    __builtin_memcpy(w2, r1 + pitch, 16);
    uint32_t g = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      g |= ((((w1[b] >> 8) & 0xffu) + ((w1[b] >> 16) & 0xffu) + ((w2[b] >> 8) & 0xffu) + ((w2[b] >> 16) & 0xffu) + 2u) >> 2) << (8 * b);
    return g;
  } else if constexpr (CH == 3) {
    return gray4_from_bgr12(base + (size_t)y * pitch + 3 * (size_t)x0);
  } else {
    uint32_t w;
    __builtin_memcpy(&w, base + (size_t)y * pitch + x0, 4);
    return w;
  }
}

// One bin of the normalised cross-power spectrum from the packed transform Z = FFT(cur + i prev):
//   A[k] = (Z[k] + conj(Z[-k]))/2 ; B[k] = (Z[k] - conj(Z[-k]))/(2i) ; P = A conj(B)        (mulSpectrums :1494)
//   C = P |P| / (|P|^2 + eps)                                   (magSpectrums :70-168, divSpectrums :1086-1251)
//   real-only CCS slots: C = P / (P^2 + eps)                                   (:107-109 / :1127-1129)
// ONE hardware sqrt and ONE hardware reciprocal (1 ulp each): the IEEE divide/sqrt expansions were a fifth of the
// kernel's VALU work for no effect at 1e-4 px.
//
// PK = 1 is the useOCL=true normalisation (cl/FftMethod.cl:971-982, :1024-1031): C = P rsqrt(|P|^2 + eps)
// for every pair and 1 / (a b) in the four real-only slots.
// cross_power_ab takes the two spectra already separated (and doubled): A2 = 2A, B2 = 2B.
template <int PK = 0>
__device__ __forceinline__ cf cross_power_ab(cf A, cf B, bool real_only) {
  // Worked on 2A = Z[k] + conj(Z[-k]) and 2B = -i (Z[k] - conj(Z[-k])): P' = 2A conj(2B) = 4P, and
  //   P |P| / (|P|^2 + eps)  ==  P' |P'| / (|P'|^2 + 16 eps)   exactly (powers of two), four multiplies fewer per bin.
  const float eps16 = 16.f * 1.1920928955078125e-07f;  // 16 * FLT_EPSILON, :1117
  if (real_only) {
    // P = A.x B.x / 4 ; C = P / (P^2 + eps) = 4 P' / (P'^2 + 16 eps)
    const float p4 = A.x * B.x;
    if constexpr (PK == 1) return {4.f * __builtin_amdgcn_rcpf(p4), 0.f};  // 1 / (a b), cl:1029
    return {4.f * p4 * __builtin_amdgcn_rcpf(p4 * p4 + eps16), 0.f};
  }
  const float pr = A.x * B.x + A.y * B.y;
  const float pim = A.y * B.x - A.x * B.y;
  const float q = pr * pr + pim * pim;
  if constexpr (PK == 1) {
    // P rsqrt(|P|^2 + eps) == P' rsqrt(|P'|^2 + 16 eps)
    const float s = __builtin_amdgcn_rsqf(q + eps16);
    return {pr * s, pim * s};
  }
  // |P'|^2 >= 2^10: 16 eps / q < 2^-30 is below half an ulp of the unit-magnitude result, so C = P' rsq(q); the general
  // form is only needed for (numerically) empty bins such as constant patches. What the compiler makes of the test
  // below is NOT a branch (profiles/xpow_batch_static.txt): it if-converts it, and every bin executes v_rsq_f32,
  // v_sqrt_f32 and v_rcp_f32 (quarter rate each) plus the compare and two selects. That is accepted at the sites that
  // keep this scalar form -- single bins, the real-only slots, lanes that repeat a bin -- and is what
  // cross_power_ab_batch (below) removes where a lane holds several bins in registers.
  float s = __builtin_amdgcn_rsqf(q);
  if (__builtin_amdgcn_ballot_w64(!(q >= 1024.f)) != 0)
    s = (q >= 1024.f) ? s : __builtin_amdgcn_sqrtf(q) * __builtin_amdgcn_rcpf(q + eps16);
  return {pr * s, pim * s};
}

// The two real images ride one complex transform (z = cur + i prev): untangle bin k from Z[k] and Z[-k], doubled
__device__ __forceinline__ void untangle2(cf zk, cf zm, cf* A2, cf* B2) {
  *A2 = {zk.x + zm.x, zk.y - zm.y};
  *B2 = {zk.y + zm.y, zm.x - zk.x};
}

template <int PK = 0>
__device__ __forceinline__ cf cross_power(cf zk, cf zm, bool real_only) {
  cf A, B;
  untangle2(zk, zm, &A, &B);
  return cross_power_ab<PK>(A, B, real_only);
}

// R bins of one lane at once (none of them a real-only slot), bin by bin the arithmetic of cross_power_ab: P', q and
// s = rsq(q) for every bin, the per-bin tests !(q >= 1024) OR-ed into ONE flag and ONE ballot per batch, and the general
// form for all R bins behind one branch that a textured patch never takes. The empty asm keeps that branch a branch (as
// for the constant-patch codes of pc_kernel.hip): the main path then carries R v_rsq_f32 and no v_sqrt_f32 / v_rcp_f32,
// and -- one basic block for the whole batch -- the loads that feed it can all be in flight before the first bin is
// worked on (ISA evidence: profiles/xpow_batch_static.txt). PK = 1 has no rare path.
//
// The sums of two products are spelled as the fused multiply-adds the compiler made of cross_power_ab's expressions at the
// site the batch replaces -- it contracted them differently in the pair kernels (operands fresh from untangle2) and in the
// sequence kernel (spectra in registers) --, so that every bin keeps the bits it had: XPOW_PAIR / XPOW_SEQ.
enum { XPOW_PAIR = 0, XPOW_SEQ = 1 };
template <int PK, int R, int FORM>
__device__ __forceinline__ void cross_power_ab_batch(const cf* A, const cf* B, cf* C) {
  const float eps16 = 16.f * 1.1920928955078125e-07f;  // 16 * FLT_EPSILON, as cross_power_ab
  float pr[R], pim[R], q[R], s[R];
  bool rare = false;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    if constexpr (FORM == XPOW_PAIR) {
      pr[k] = __builtin_fmaf(A[k].y, B[k].y, A[k].x * B[k].x);
      pim[k] = __builtin_fmaf(-A[k].x, B[k].y, A[k].y * B[k].x);
      q[k] = __builtin_fmaf(pim[k], pim[k], pr[k] * pr[k]);
    } else {
      pr[k] = __builtin_fmaf(A[k].x, B[k].x, A[k].y * B[k].y);
      pim[k] = __builtin_fmaf(A[k].y, B[k].x, -(A[k].x * B[k].y));
      q[k] = __builtin_fmaf(pr[k], pr[k], pim[k] * pim[k]);
    }
    if constexpr (PK == 1) {
      s[k] = __builtin_amdgcn_rsqf(q[k] + eps16);
    } else {
      s[k] = __builtin_amdgcn_rsqf(q[k]);
      rare |= !(q[k] >= 1024.f);
    }
  }
  if constexpr (PK != 1) {
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(rare) != 0, 0)) {
      asm volatile("");
#pragma unroll
      for (int k = 0; k < R; ++k) s[k] = (q[k] >= 1024.f) ? s[k] : __builtin_amdgcn_sqrtf(q[k]) * __builtin_amdgcn_rcpf(q[k] + eps16);
    }
  }
#pragma unroll
  for (int k = 0; k < R; ++k) C[k] = {pr[k] * s[k], pim[k] * s[k]};
}

// ... from the packed transform's bins zk[k] = Z[k], zm[k] = Z[-k], conjugated for the Hermitian inverse
template <int PK, int R>
__device__ __forceinline__ void cross_power_batch(const cf* zk, const cf* zm, cf* out_conj) {
  cf A[R], B[R];
#pragma unroll
  for (int k = 0; k < R; ++k) untangle2(zk[k], zm[k], &A[k], &B[k]);
  cross_power_ab_batch<PK, R, XPOW_PAIR>(A, B, out_conj);
#pragma unroll
  for (int k = 0; k < R; ++k) out_conj[k].y = -out_conj[k].y;
}

// ---- degenerate pairs: a CONSTANT patch ----------------------------------------------------------------------------
// cv::phaseCorrelate transforms the two patches separately (FftMethod.cpp:1491-1493): a constant patch has an EXACTLY zero
// AC spectrum, the cross-power spectrum keeps its DC bin (a real-only slot: C = P / (P^2 + eps)) and nothing else, and the
// surface is flat = C_dc: first maximum at shifted (0, 0), centroid of the clamped 3 x 3 window of equal values =
// (1, 1) 9c / (9c + DBL_EPSILON) -- or (0, 0) when C_dc = 0 (an all-zero patch). The pair kernels pack cur + i prev into one
// complex transform, which leaks ~1e-7 of the textured patch's spectrum into those zeros; the normalisation blows that up
// to unit magnitude and the result is noise (found by tools/fft_sr_fuzz.py, r03). So constant patches are detected where
// the pixels are loaded (exact: integer compares) and the exact answer is substituted in the tail.
// A constant n x n patch that cv::phaseCorrelate pads to m x m is a BOX, and its spectrum -- level D[v] D[u], D the transform of n ones in a
// line of m -- is EXACTLY zero on every line k != 0 with k n = 0 (mod m), i.e. on the multiples of q = m / gcd(n, m): the Nyquist line
// alone when n and m share one factor of two only (158 in 160), but 40, 80, 120 for 156 in 160 and every multiple of 20 for 152 in 160.
// There P = 0 and C = 0; any transform that leaves rounding noise in those bins has it normalised to unit magnitude (0.03 - 0.09 px off on
// 156 / 152-pixel constant-against-texture pairs, tools/fft_sr_fuzz.py seeds 606 / 608, r05). The kernels know a constant patch exactly
// (integer compares where the pixels are loaded), so they zero exactly those bins. q = m when there is no such line.
__device__ __forceinline__ int box_zero_period(int n, int m) {
  int a = m, b = n;
  while (b != 0) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return m / a;
}
__device__ __forceinline__ bool box_zero_line(int k, int q) { return k != 0 && k % q == 0; }

// (1) per lane: `first` = its first pixel, `diff` != 0 iff one of its packed pixels differs from it
__device__ __forceinline__ void const_track(const uint32_t* words, int n_words, bool reset, uint32_t& first, uint32_t& diff) {
  if (reset) {
    first = words[0] & 0xffu;
    diff = 0u;
  }
  const uint32_t pat = first * 0x01010101u;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < n_words) diff |= words[i] ^ pat;
}
// (2) per wave: the pixel value if every `on` lane holds nothing else, or 256 (lane 0 must be `on`)
__device__ __forceinline__ int wave_const_code(bool on, uint32_t first, uint32_t diff) {
  const uint32_t f0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)first);
  const bool bad = on && (diff != 0u || first != f0);
  return __builtin_amdgcn_ballot_w64(bad) == 0ull ? (int)f0 : 256;
}
// (3) the per-wave codes live in LDS as int codes[16]: cur code | prev code << 16, 256 = "not constant", written by lane 0
// of every wave for every patch (a textured patch fails a two-compare pre-test and writes 256 | 256 << 16); one wave reads
// them in the tail (the LDS read `my = codes[lane & 15]` is issued ahead of its other tail reads: the latencies overlap)
template <int WAVES>
__device__ __forceinline__ bool const_codes_degenerate(int my, int lane) {
  static_assert(WAVES <= 16, "16 codes");
  const int c = my & 0xffff, p = (int)((unsigned)my >> 16);
  const int c0 = __builtin_amdgcn_readfirstlane(c), p0 = __builtin_amdgcn_readfirstlane(p);
  const bool cur_const = c0 < 256 && __builtin_amdgcn_ballot_w64(lane < WAVES && c != c0) == 0ull;
  const bool prev_const = p0 < 256 && __builtin_amdgcn_ballot_w64(lane < WAVES && p != p0) == 0ull;
  return cur_const || prev_const;
}

// Weighted centroid in double + validity gate, executed by ONE wave in two steps so that the tile can be recycled in
// between: (1) (2 RAD + 1)^2 lanes fetch one window element each (`surface(ys, xs)` returns the fft-shifted correlation
// value; 0 outside the clamped window), (2) three fp64 sums are reduced by shuffles and lane 0 stores (x, y) or
// (NaN, NaN).
//   PK = 0: cv::phaseCorrelate's weightedCentroid, 5x5, every value, sum + DBL_EPSILON      (:1337-1383, :1838-1856)
//   PK = 1: the OpenCL kernel's refine(), 7x7, values > 0 only, sum seeded with FLT_EPSILON     (cl:1315-1379, :1478)
//           (the kernel sums floats over absolute frame coordinates; here patch-local doubles -- same value, without
//           the ~1e-4 px of rounding noise that representation adds)
template <int PK>
struct PeakModel {
  static constexpr int RAD = PK == 1 ? 3 : 2;
  static constexpr int W = 2 * RAD + 1;
};

// Lane -> its element of the W x W window around the first maximum of an m x m surface: (*ys, *xs) in fft-SHIFTED coordinates; returns `in` = the
// surface held a maximum (best.idx != 0x7fffffff: some value compared equal to it, i.e. not every value is NaN), lane < W^2 and the
// element lies on the surface (the window is clamped to the -- padded -- patch). peak_unshift: shifted -> un-shifted coordinate, the
// inverse of fftShift's i -> (i + (m >> 1)) mod m for even and odd m alike (:1257-1323).
template <int PK>
__device__ __forceinline__ bool peak_window(Best best, int lane, int m, int* ys, int* xs) {
  constexpr int RAD = PeakModel<PK>::RAD, W = PeakModel<PK>::W;
  const int py = best.idx / m, px = best.idx % m;  // (no maximum: a row far below the surface)
  *ys = py - RAD + lane / W;
  *xs = px - RAD + lane % W;
  return best.idx != 0x7fffffff && lane < W * W && *ys >= 0 && *ys <= m - 1 && *xs >= 0 && *xs <= m - 1;
}
__device__ __forceinline__ int peak_unshift(int s, int m) {
  const int H = m >> 1;
  return s - H < 0 ? s - H + m : s - H;
}

template <int N, int PK = 0, class Surface>
__device__ __forceinline__ float centroid_window_value(Best best, int lane, Surface surface) {
  int ys, xs;
  if (peak_window<PK>(best, lane, N, &ys, &xs)) {
    const float v = surface(ys, xs);
    if constexpr (PK == 1) return v > 0.f ? v : 0.f;
    return v;
  }
  return 0.f;
}

// The correlation quality of one patch, stored by lane 0 of a tail beside the shift when the launch asked for it (`q` non-null: a
// wave-uniform test of a kernarg pointer, no second instantiation). It does not depend on the gate.
//   PK = 0: q[0] = cv::phaseCorrelate's `response` = window sum (before DBL_EPSILON) / M^2, q[1] = the first maximum / M^2   (:1337-1383)
//   PK = 1: q[0] = refine()'s sum (seeded with FLT_EPSILON), q[1] = the first maximum, of the surface the kernel has scaled  (cl:1315-1379)
// `have` = the surface held a maximum (else NaN, NaN). A constant patch (`degenerate`): the flat surface c_dc of
// PK = 0 -- peak c_dc / M^2, nine of them in the clamped 3 x 3 window -- and NaN, NaN under PK = 1, as for the shift.
template <int PK>
__device__ __forceinline__ void quality_store(double* q, double window_sum, float peak, double mm, bool have, bool degenerate, float c_dc) {
  double response = window_sum, pk = (double)peak;
  if constexpr (PK == 0) {
    response /= mm;
    pk /= mm;
  }
  if (!have) response = pk = __builtin_nan("");
  if (degenerate) {
    if constexpr (PK == 1) {
      response = pk = __builtin_nan("");
    } else {
      pk = (double)c_dc / mm;
      response = 9.0 * pk;
    }
  }
  q[0] = response;
  q[1] = pk;
}

// The finish of every peak tail, by lane 0 after wave_sum3: (cx, cy, window_sum) = sums of xs v, ys v, v over the window of an m x m
// surface whose patch is n x n (m > n: zero-padded). degenerate: one of the two patches is constant (each caller decides that from its own
// flags); c_dc = the DC bin of the cross-power spectrum (see above), read only then; quality: nullable (quality_store).
template <int PK>
__device__ __forceinline__ void peak_finish(double cx, double cy, double window_sum, Best best, int m, int n, bool degenerate, float c_dc,
                                            double max_px_speed_sq, double* out, double* quality) {
  const bool have = best.idx != 0x7fffffff;
  const double sum = window_sum + (PK == 1 ? 1.1920928955078125e-07 : 2.220446049250313e-16);  // FLT_EPSILON cl:1342 / DBL_EPSILON :1378
  if (quality) quality_store<PK>(quality, PK == 1 ? sum : window_sum, best.v, (double)m * (double)m, have, degenerate, c_dc);
  // shift = -(center - t) = t - M / 2.0 (:1836): cv::phaseCorrelate's centre is that of the PADDED image; the OpenCL branch returns
  // centroid - N/2 un-negated (cl:1370, :1833) -- the same number
  const double half_m = (double)m / 2.0, half_n = (double)n / 2.0;
  double sx = cx / sum - half_m, sy = cy / sum - half_m;
  if (degenerate) {
    if constexpr (PK == 1) {
      sx = sy = __builtin_nan("");  // 1 / (a b) with b = 0 in the three other real-only slots (cl:1029): no finite surface
    } else {
      const double c9 = 9.0 * (double)c_dc;
      sx = sy = (c9 > 0.0 ? c9 / (c9 + 2.220446049250313e-16) : 0.0) - half_m;
    }
  }
  // the gate compares with samplePointSize / 2 -- the UNPADDED size (:1841-1842). !have: the whole surface is NaN (a spectrum with
  // infinities, e.g. 1/0 in a real-only slot under the OpenCL model) -> invalid, as a NaN centroid is
  const bool bad = (sx * sx + sy * sy > max_px_speed_sq) || (fabs(sx) > half_n) || (fabs(sy) > half_n) || (sx != sx) || (sy != sy) ||
                   (!have && !degenerate);
  if (bad) sx = sy = __builtin_nan("");
  out[0] = sx;
  out[1] = sy;
}

// the compile-time N = M = n form: `wval` = the lane's centroid_window_value
template <int N, int PK = 0>
__device__ __forceinline__ void centroid_gate_store(Best best, float wval, int lane, double max_px_speed_sq, double* out, double* quality,
                                                    bool degenerate = false, float c_dc = 0.f) {
  int ys, xs;
  peak_window<PK>(best, lane, N, &ys, &xs);
  const double val = (double)wval;  // 0 for lanes outside the window
  double cx = (double)xs * val, cy = (double)ys * val, sum = val;
  wave_sum3(cx, cy, sum);
  if (lane == 0) peak_finish<PK>(cx, cy, sum, best, N, N, degenerate, c_dc, max_px_speed_sq, out, quality);
}

// The estimator's finish, by lane 0: pt = cv::phaseCorrelate(cur_lp, prev_lp) = center - t, NOT negated (scaleRotationEstimator.cpp:117);
// |pt.x| > resolution / 2 (int division) -> (1, 0) (:119-121); scale = exp(pt.x / M), rot = (pt.y / Ky) pi/180, Ky = resolution / 360
// (:123-124). An all-zero log-polar image has an exactly zero spectrum -- flat zero surface: first index, centroid 0 / (0 + eps), pt = (m / 2, m / 2),
// quality (0, 0) -- and needs no special case here. out4 = scale, rot, pt.x, pt.y
// The quality of that surface (quality_store<0>: response, peak; `best` = its first maximum) goes to `quality` when that is non-null, whatever
// the gates decide. min_response > 0 arms the response gate, which acts as the reference's: !(response >= min_response) -> (1, 0), pt still
// reported. It reads the very double that is stored, so a host that reads `quality` back decides as this code did.
__device__ __forceinline__ void sr_finish(double cx, double cy, double sum, Best best, int m, int n, double M_log, double* out4, double* quality,
                                          double min_response) {
  double q[2] = {0.0, 0.0};
  if (quality || min_response > 0.0) quality_store<0>(q, sum, best.v, (double)m * (double)m, best.idx != 0x7fffffff, false, 0.f);
  if (quality) {
    quality[0] = q[0];
    quality[1] = q[1];
  }
  sum += 2.220446049250313e-16;
  const double half_m = (double)m / 2.0;
  const double ptx = half_m - cx / sum, pty = half_m - cy / sum;
  double scale = 1.0, rot = 0.0;
  if (!(fabs(ptx) > (double)(n / 2)) && !(min_response > 0.0 && !(q[0] >= min_response))) {
    scale = exp(ptx / M_log);
    rot = (pty / ((double)n / 360.0)) * (3.14159265358979323846 / 180.0);
  }
  out4[0] = scale;
  out4[1] = rot;
  out4[2] = ptx;
  out4[3] = pty;
}

// The W x W window of a surface that exists only as the half spectrum of its rows (Dt[u][y], u <= m / 2: K8 and L8 keep no surface),
// re-evaluated in double: S[y][x] = Re G[y][0] + [m even: (-1)^x Re G[y][m/2]] + 2 sum_{u=1}^{(m-1)/2} Re(G[y][u] W^{ux}), what the
// inverse row transform computes for that point. One wave: the first maximum of `cand` (*best_out, in every lane), the sums split over
// the lanes by u (lane, lane + 64, ..), W^2 partial sums each, handed over through the kernel's part[W^2][65], lane k < W^2 adds the 64
// of its window point in a fixed order. Returns the lane's window value (the surface is CV_32F), 0 outside the clamped window.
// NS > 0: the compile-time transform size; NS = 0: m_rt.
template <int W, int NS>
__device__ __forceinline__ float spectrum_window(const float2* __restrict__ cand, int n_cand, const cf* __restrict__ Dt,
                                                 const float* __restrict__ twiddles, int m_rt, int lane, double (*part)[65], Best* best_out) {
  constexpr int PK = W == PeakModel<1>::W ? 1 : 0, WW = W * W;
  static_assert(W == PeakModel<PK>::W, "a peak model's window");
  const int m = NS > 0 ? NS : m_rt, H = m >> 1;
  const bool even = (m & 1) == 0;
  const int umax = even ? H - 1 : H;
  Best best = {-__builtin_huge_valf(), 0x7fffffff};
  for (int i = lane; i < n_cand; i += 64) {
    const float2 c = cand[i];
    best = better(best, Best{c.x, __float_as_int(c.y)});
  }
  best = wave_best(best);
  *best_out = best;
  int ys, xs;
  peak_window<PK>(best, 0, m, &ys, &xs);  // the window's first row and column; un-shifted and wrapped (entries outside the clamped window are skipped below;
                                          // no maximum: ys is far below the surface, the double modulo still leaves every wy / wx in [0, m))
  int wy[W], wx[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    wy[k] = ((((ys + k) % m) + m) % m - H + m) % m;
    wx[k] = ((((xs + k) % m) + m) % m - H + m) % m;
  }
  double acc[WW];
#pragma unroll
  for (int k = 0; k < WW; ++k) acc[k] = 0.0;
  for (int u = 1 + lane; u <= umax; u += 64) {
    cf f[W];
#pragma unroll
    for (int r = 0; r < W; ++r) f[r] = Dt[(size_t)u * m + wy[r]];
#pragma unroll
    for (int c = 0; c < W; ++c) {
      const float2 t = *reinterpret_cast<const float2*>(twiddles + 2 * (int)(((long)u * wx[c]) % m));  // (cos, -sin)
#pragma unroll
      for (int r = 0; r < W; ++r) acc[r * W + c] += (double)f[r].x * (double)t.x - (double)f[r].y * (double)t.y;
    }
  }
#pragma unroll
  for (int k = 0; k < WW; ++k) part[k][lane] = acc[k];
  __syncthreads();
  if (!peak_window<PK>(best, lane, m, &ys, &xs)) return 0.f;
  const int y = wy[lane / W], x = wx[lane % W];
  double s2 = 0.0;
  for (int l = 0; l < 64; ++l) s2 += part[lane][l];
  double s0 = (double)Dt[y].x;
  if (even) s0 += ((x & 1) ? -1.0 : 1.0) * (double)Dt[(size_t)H * m + y].x;
  return (float)(s0 + 2.0 * s2);
}

// PK = 1 only: value (y, x) of the UN-shifted m x m surface after the kernel's scaling and +-search_radius mask
// (cl:733, :737-746, :823-826): rows / columns with search_radius < index < m - search_radius read as 0.
// scale = 1.0f / (float)(m * m), hoisted by the caller
__device__ __forceinline__ float ocl_scale_mask(float v, int y, int x, int sr, int m, float scale) {
  const bool masked = (y > sr && y < m - sr) || (x > sr && x < m - sr);
  return masked ? 0.f : v * scale;
}
template <int N>
__device__ __forceinline__ float ocl_scale_mask(float v, int y, int x, int sr) {
  return ocl_scale_mask(v, y, x, sr, N, 1.0f / (float)(N * N));
}

}  // namespace
}  // namespace mof
