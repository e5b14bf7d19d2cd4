// pc_kernel.hip -- K1: fused per-patch FFT phase correlation for gfx950 (CDNA4).
//
// One workgroup owns one patch pair and never leaves the CU: the two u8 patches are read once
// from HBM (16 B per lane, any byte alignment), packed as z = cur + i*prev into ONE complex N x N
// tile in LDS ("two-for-one" real transform), transformed, untangled into the two real spectra,
// turned into the normalised cross-power spectrum, inverse-transformed exploiting its Hermitian
// symmetry (half the work of a complex inverse), and reduced to (arg-max, 5x5 centroid): 16 B leave
// the CU per patch. Nothing but the frames and the results touches HBM. (N = 64 under cv::phaseCorrelate's peak model: 128 B leave the
// CU, a record of the peak and its window, and pc_finish_kernel -- one lane per patch, at the end of this file's kernels -- runs the fp64
// centroid and the gate for the whole launch.)
//
// Replaces, per patch, the reference's
//   -cv::phaseCorrelate(cur(roi), prev(roi))              src/FftMethod.cpp:1836
// whose stages the reference spells out at src/FftMethod.cpp:1487-1498, with the helper semantics of
// :70-168 (magSpectrums), :1086-1251 (divSpectrums), :1257-1323 (fftShift), :1329-1385
// (weightedCentroid), followed by the validity gate of :1838-1856.
//
// CDNA4 mapping
//   * N*N/16 threads; each 1-D transform is two Stockham stages N = R1*R2 with 16 points per lane in
//     registers (64 = 8*8, 128 = 16*8, 32 = 8*4), twiddles in registers (host-computed in double);
//   * wave w owns rows (then columns) [w*L, (w+1)*L) through a whole 1-D pass, so the stages of a
//     pass are ordered by the wave's in-order LDS queue and need no workgroup barrier: 5 barriers
//     per patch in total;
//   * LDS tile is skewed (element c of a row sits at c + (c >> SK), row pitch = 8 mod 16 complex) so
//     that the stride-R accesses of the Stockham stages and the column walks are bank-conflict free;
//   * LDS writes cost 3x reads on this chip (MI355X_MICROARCH.md, LDS table): the Hermitian inverse
//     writes half a tile per stage and the arg-max is taken from registers.
//
// Arithmetic: fp32 transforms (as OpenCV for CV_32F), fp64 centroid and gate.
// Algorithmic HBM bytes per patch: 2*N*N in + 16 out.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <stdint.h>
#include <stdlib.h>

#include "mof_kernels.h"
#include "pc_common.hpp"
#include "pc_finish_tree.hpp"
#include "pc_launch.hpp"

#include "pc_passes.hpp"
#include "pc_passes3.hpp"

namespace mof {

// DS = 1: patches are read from the frames as they are. DS = 4: long-range mode -- every patch pixel is the
// quarter-resolution pixel cv::resize(.., 1/4, 1/4, INTER_LINEAR) would produce (FftMethod.cpp:1931-1932), i.e.
// the rounded mean of the 2x2 centre of a 4x4 cell, formed on the fly from the full-resolution frame.
// CH = 3: the frames are interleaved BGR8 and the CV_RGB2GRAY conversion of the node's front end
// (optic_flow.cpp:1622) is fused into the load, so raw camera frames are read from HBM exactly once.
// PK = 1: the peak model of the reference's useOCL=true branch (cl/FftMethod.cl) instead of cv::phaseCorrelate's.
// OFF: the fused window-offset form (include/mof.h, "Predicted-shift window offsets"; full resolution, PK = 0 only) -- the previous
// patch of linear index q is read at (x0 - a_x, y0 - a_y), (a_x, a_y) = a.prev_off[2 q], [2 q + 1]: a change of its base address, which
// depends on the workgroup's patch index alone -- two scalar loads and scalar arithmetic, no VGPR, no LDS
// (profiles/fft_pred_fused_static.txt). Everything else is the form it was made from, so are its bits on the same pixels.
// A: PcArgs, or PcArgsRecord for the forms that end a patch with a record (RECORD below: N = 64 under cv::phaseCorrelate's peak model). The
// record buffer rides behind the PcArgs those forms take: PcArgs keeps its size, and with it every other kernel that takes one its code.
struct PcArgsRecord : PcArgs {
  uint32_t* finish;  // device, engine-owned: PC_FINISH_DWORDS dwords per patch of the launch (mof_kernels.h)
};
// One patch's record (mof_kernels.h, PC_FINISH_DWORDS), by the wave that ends the patch, every lane with the same `b` and `deg`:
// wv = the lane's centroid_window_value; const_code + 16 = C_dc, read for a constant patch only, as the finish read it in K1
__device__ __forceinline__ void pc_store_record(uint32_t* finish, int p, int lane, Best b, float wv, bool deg, const int* const_code) {
  const float c_dc = deg ? *reinterpret_cast<const float*>(const_code + 16) : 0.f;
  uint32_t v = __float_as_uint(wv);  // (0 in lanes 25 .. 63: outside the 5 x 5 window)
  v = lane == 25 ? __float_as_uint(b.v) : v;
  v = lane == 26 ? (uint32_t)b.idx : v;
  v = lane == 27 ? (deg ? 1u : 0u) : v;
  v = lane == 28 ? __float_as_uint(c_dc) : v;
  if (lane < PC_FINISH_DWORDS) finish[(size_t)PC_FINISH_DWORDS * (size_t)p + lane] = v;
}
// The pair of a wave that holds the workgroup's maximum gm, record forms (N = 64): `holders` = the wave's ballot of m == gm, not zero; sv, m
// as col_pass_inv<N, PK, false> left them. Every lane walks the index chain, all 64 lanes active.
// Where ONE lane of the wave holds the maximum -- every textured patch -- that lane's own (m, mi) is read with two v_readlane behind one
// s_ff1 of the ballot: wave_best's six levels would end with that pair in every lane (argmax_lone_holder, pc_argmax.hpp). Any other count
// folds as before. The branch is wave-uniform, and the fold, now the rare side, is kept behind it.
template <int N>
__device__ __forceinline__ Best holder_pair(const cf* sv, float m, float gm, int col0, int lane, unsigned long long holders) {
  const int mi = col_pass_inv_index<N>(sv, m, col0, lane);
  if (__builtin_expect(!argmax_lone_holder(holders), 0)) {
    asm volatile("");
    return wave_best(argmax_entry(m, gm, mi));
  }
  const int l = argmax_lone_lane(holders);
  return Best{__int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), l)), __builtin_amdgcn_readlane(mi, l)};
}
template <int N, int PK>
using PcFieldArgs = std::conditional_t<pc_field_records(N, PK), PcArgsRecord, PcArgs>;
template <int N, int DS, int CH, int PK, bool OFF = false, class A = PcFieldArgs<N, PK>>
__global__ void __launch_bounds__(PcTraits<N>::T) pc_field_kernel(A a) {
  static_assert(CH == 1 || (CH == 3 && DS == 1), "BGR front end only for the full-resolution path");
  static_assert(!OFF || (DS == 1 && PK == 0), "window offsets: full resolution, cv::phaseCorrelate's peak model");
  using P = PcTraits<N>;
  constexpr int T = P::T, H = N / 2, R1 = P::R1, R2 = P::R2, LPW = P::LPW;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* z = reinterpret_cast<cf*>(smem);
  Best* red = reinterpret_cast<Best*>(z + P::TILE);
  int* const_code = reinterpret_cast<int*>(red + 32);  // [16] per-wave constant-patch codes (cur | prev << 16), then C_dc (pc_common.hpp)

  const int tid0 = threadIdx.x, lane0 = tid0 & 63, wave0 = tid0 >> 6;
  const int patches = a.grid_x * a.grid_y;
  constexpr int CPR = N / 16;  // 16-pixel chunks per row
  const int lrow = wave0 * LPW + ord1<N>(lane0 / CPR), lcol = (lane0 % CPR) * 16;  // this lane's 16 pixels of the patch (ord1: pc_passes.hpp)
  const bool ld_on = lane0 < LPW * CPR;  // (all lanes unless the workgroup has more than N*N/16 threads)

  // N >= 128: persistent workgroups (one per CU) walking a linear patch index. Smaller tiles: one workgroup per
  // patch on a 3-D grid (patch column, patch row, pair) -- the hardware dispatcher balances 4 workgroups per CU better
  // than a static stride does, and the patch coordinates come from blockIdx without the integer divisions that
  // otherwise cost ~5 % of the kernel's VALU instructions.
  constexpr bool PERSIST = P::PERSIST;
  // N = 32 (one wave per workgroup) keeps the parent's prologue with the persistent form: with the straight-line one it measured 3 % slower
  // (profiles/k1_prologue_ab.txt). OLD_PROLOGUE: the loop, the laundering, the p < total guard, 64-bit lane addresses, const_track as it was.
  constexpr bool OLD_PROLOGUE = PERSIST || N == 32;
  constexpr bool FWD3 = N == 64 && DS == 1;                  // the three-stage forward transform (pc_passes3.hpp)
  constexpr bool RAW = (N == 128 || N == 64) && DS == 1;     // raw pixel staging (pc_passes.hpp)
  // arg-max by value first (below). One patch per workgroup and more than one wave: a single wave (N = 32) always holds the maximum,
  // so nothing would leave its path; the persistent form's second barrier already has a job (it protects the tile)
  constexpr bool VALUE_FIRST = !PERSIST && P::WAVES > 1;
  (void)patches;
  // (x0, y0) of a patch are in the units of the correlated image: full-res pixels, or quarter-res when DS = 4
  auto patch_base = [&](int p, const uint8_t* frames, size_t frame_stride) -> const uint8_t* {
    int pr, bx, by;
    if constexpr (PERSIST) {
      const int pt = p % patches;
      pr = p / patches;
      bx = pt % a.grid_x;
      by = pt / a.grid_x;
    } else {
      pr = blockIdx.z;
      bx = blockIdx.x;
      by = blockIdx.y;
    }
    const int px0 = a.origin_x + bx * a.stride_x, py0 = a.origin_y + by * a.stride_y;
    return frames + (size_t)pr * frame_stride + (size_t)(DS * py0) * a.pitch + (size_t)(CH * DS * px0);
  };
  // the previous patch's base: OFF moves it by the applied prediction of patch q -- signed, 64-bit: either component may be negative.
  // The clamp kernel wrote a.prev_off (pc_offset_kernel.hip), so the window stays inside the frame.
  auto prev_base = [&](int q) -> const uint8_t* {
    const uint8_t* base = patch_base(q, a.prev, a.prev_stride);
    if constexpr (OFF) {
      // (through the constant address space: nothing writes the applied predictions while the kernel runs, and saying so keeps the
      // persistent loop's re-reads scalar loads -- behind the loop's own stores the compiler otherwise takes a vector load)
      typedef const int32_t __attribute__((address_space(4))) * const_i32_ptr;
      const const_i32_ptr off = (const_i32_ptr)a.prev_off;
      const int64_t ax = off[2 * (size_t)q], ay = off[2 * (size_t)q + 1];
      base -= ay * (int64_t)a.pitch + (int64_t)CH * ax;
    }
    return base;
  };

  // twiddles of the second Stockham stage, W_N^{k x}: x = lane % R1 in row passes, lane / (64/R1) in column passes
  // (the persistent form gathers them here, first; the one-patch forms -- the ones with packed rows -- ask for theirs behind the two pixel
  // loads, which are what they wait for)
  static_assert(TwRows<N>::USE == !P::PERSIST, "packed twiddle rows: the one-patch forms");
  cf tw_row[R2 - 1], tw_col[R2 - 1];
  Fwd3Tw tw3;
  auto load_twiddle_rows = [&] {  // one packed row each (TwRows, pc_passes.hpp)
    const int xr = lane0 % R1, xc = lane0 / (64 / R1);
    tw_row_load<R2, N == 32>(a.twiddles + TwRows<N>::ROWS_AT + 2 * R2 * xr, tw_row);
    tw_row_load<R2, N == 32>(a.twiddles + TwRows<N>::ROWS_AT + 2 * R2 * xc, tw_col);
    if constexpr (FWD3) tw3.load(a.twiddles, wave0, lane0);
  };
  if constexpr (TwRows<N>::USE && OLD_PROLOGUE) load_twiddle_rows();
  if constexpr (!TwRows<N>::USE) {
    const int xr = lane0 % R1, xc = lane0 / (64 / R1);
#pragma unroll
    for (int k = 1; k < R2; ++k) {
      tw_row[k - 1] = {a.twiddles[2 * (k * xr)], a.twiddles[2 * (k * xr) + 1]};
      tw_col[k - 1] = {a.twiddles[2 * (k * xc)], a.twiddles[2 * (k * xc) + 1]};
    }
  }
  // ---- persistent workgroup: patches p = blockIdx.x, + gridDim.x, ...; the 2 x 16 B of the NEXT patch are
  //      requested from HBM before the current one is transformed, so the ~2 us load latency is off the critical path
  uint32_t cw[4] = {0u, 0u, 0u, 0u}, pw[4] = {0u, 0u, 0u, 0u};
  int p = PERSIST ? (int)blockIdx.x : (int)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
  auto fetch16 = [&](int pp, uint32_t* c, uint32_t* q) {
    const uint8_t *cs, *ps;
    if constexpr (OLD_PROLOGUE) {
      cs = patch_base(pp, a.cur, a.cur_stride) + (size_t)lrow * a.pitch + CH * lcol;
      ps = prev_base(pp) + (size_t)lrow * a.pitch + CH * lcol;
    } else {
      // The patch bases depend on the workgroup alone (scalar, 64-bit, signed under OFF); the lane's part lrow * pitch + CH * lcol is ONE
      // 32-bit value for both images: lrow < 64 and pitch < 2^24 (PC_MAX_PITCH, refused by launch_pc_field beyond it) keep the 24-bit
      // multiply exact and the sum below 2^30 + 144. Scalar base + 32-bit lane offset is an addressing mode of global_load.
      const uint32_t lane_off = __umul24((uint32_t)lrow, (uint32_t)a.pitch) + (uint32_t)(CH * lcol);
      cs = patch_base(pp, a.cur, a.cur_stride) + lane_off;
      ps = prev_base(pp) + lane_off;
    }
    if constexpr (CH == 1) {
      __builtin_memcpy(c, cs, 16);
      __builtin_memcpy(q, ps, 16);
    } else {
      gray16_from_bgr48(cs, c);
      gray16_from_bgr48(ps, q);
    }
  };
  // (one-patch forms: launch_n launches exactly grid_x x grid_y x nk workgroups with total = nk x patches -- pc_split_pairs --, so p < total
  // holds for every workgroup and is not asked: the pixel loads do not wait for a kernel-argument round trip and a branch)
  if (DS == 1 && (!OLD_PROLOGUE || p < a.total) && ld_on) fetch16(p, cw, pw);
  if constexpr (TwRows<N>::USE && !OLD_PROLOGUE) load_twiddle_rows();
  // Co-resident workgroups would otherwise run the same phase at the same time (all of them LDS-bound, then all
  // VALU-bound): delay the k-th workgroup of a CU by k quarter-patches so their phases interleave.
  if constexpr (PERSIST) {
    const int slot = (blockIdx.x / a.stagger_div) & 3;
    for (int i = 0; i < slot * a.stagger_units; ++i) __builtin_amdgcn_s_sleep(100);
  }
  // The persistent form walks its patches. A one-patch form runs the body once, as straight-line code: p < total holds (above) and the
  // body ends with a break -- no loop header, no test of a.total, no wait for the twiddle loads in front of it.
  if constexpr (!OLD_PROLOGUE) __builtin_assume(p < a.total);
  for (; p < a.total; p += PERSIST ? (int)gridDim.x : a.total) {
  // The lane / wave indices are laundered once per patch: otherwise LICM hoists every LDS address of the body out
  // of the persistent loop (+70 VGPRs), which costs a whole workgroup of occupancy per CU. (No loop, nothing to hoist out of.)
  int lane = lane0, wave = wave0;
  if constexpr (OLD_PROLOGUE) asm volatile("" : "+v"(lane), "+v"(wave));
  lane &= 63;             // give the value ranges back to the optimiser (they fold the skew and the
  wave &= P::WAVES - 1;   // Hermitian row cases at compile time)
  const int tid = wave * 64 + lane;
  // ---- the wave's own LPW rows: u8 -> f32 (exact), z = cur + i*prev  (convertTo, :1805-1806)
  {
    const int row = wave * LPW + ord1<N>(lane / CPR), col = (lane % CPR) * 16;
    int cc = 256, cp = 256;  // constant-patch codes of this wave (pc_common.hpp)
    if constexpr (DS == 1) {
      // pre-test: a textured patch has a lane whose first two dwords differ -- two compares and it is out
      const bool maybe_c = __builtin_amdgcn_ballot_w64(ld_on && cw[0] != cw[1]) == 0ull;
      const bool maybe_p = __builtin_amdgcn_ballot_w64(ld_on && pw[0] != pw[1]) == 0ull;
      // (the empty asm keeps the compiler from if-converting the rare branch into unconditional instructions. That alone does not pin
      // const_track's compare chain, whose inputs are pure: the one-patch forms hand it the words through an asm inside the branch, so
      // the chain depends on something that exists only there. The persistent form is spelled as it was.)
      auto track = [&](const uint32_t* w, uint32_t& f, uint32_t& d) {
        uint32_t t[4] = {w[0], w[1], w[2], w[3]};
        asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));
        const_track(t, 4, true, f, d);
      };
      if (__builtin_expect(maybe_c, 0)) {
        asm volatile("");
        uint32_t f, d;
        if constexpr (OLD_PROLOGUE) const_track(cw, 4, true, f, d);
        else track(cw, f, d);
        cc = wave_const_code(ld_on, f, d);
      }
      if (__builtin_expect(maybe_p, 0)) {
        asm volatile("");
        uint32_t f, d;
        if constexpr (OLD_PROLOGUE) const_track(pw, 4, true, f, d);
        else track(pw, f, d);
        cp = wave_const_code(ld_on, f, d);
      }
    }
    uint32_t fc = 0, dc = 0, fp = 0, dp = 0;  // (long-range mode forms its pixels one by one: tracked in its loop)
    if constexpr (RAW) {
      // raw bytes into the wave's staging area; the first row stage converts them (pc_passes.hpp, raw_store)
      raw_store<N>(z, wave * LPW, lane, cw, pw);
      if constexpr (PERSIST) {
        const int pn = p + gridDim.x;
        if (pn < a.total) fetch16(pn, cw, pw);
      }
    } else if constexpr (DS == 1) {
      if (ld_on) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            z[zaddr<N>(row, col + q * 4 + b)] = {(float)((cw[q] >> (8 * b)) & 0xffu), (float)((pw[q] >> (8 * b)) & 0xffu)};
          }
        if constexpr (PERSIST) {
          const int pn = p + gridDim.x;
          if (pn < a.total) fetch16(pn, cw, pw);
        }
      }
    } else if (ld_on) {
      // pixel (row, col+i) <- (s(4r+1,4c+1) + s(4r+1,4c+2) + s(4r+2,4c+1) + s(4r+2,4c+2) + 2) >> 2 of the full-res frame
      const uint8_t* c1 = patch_base(p, a.cur, a.cur_stride) + (size_t)(4 * row + 1) * a.pitch + 4 * col;
      const uint8_t* p1 = patch_base(p, a.prev, a.prev_stride) + (size_t)(4 * row + 1) * a.pitch + 4 * col;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t ca[4], cb[4], pa[4], pb[4];
        __builtin_memcpy(ca, c1 + 16 * q, 16);
        __builtin_memcpy(cb, c1 + a.pitch + 16 * q, 16);
        __builtin_memcpy(pa, p1 + 16 * q, 16);
        __builtin_memcpy(pb, p1 + a.pitch + 16 * q, 16);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const uint32_t cs = ((ca[b] >> 8) & 0xffu) + ((ca[b] >> 16) & 0xffu) + ((cb[b] >> 8) & 0xffu) + ((cb[b] >> 16) & 0xffu);
          const uint32_t ps = ((pa[b] >> 8) & 0xffu) + ((pa[b] >> 16) & 0xffu) + ((pb[b] >> 8) & 0xffu) + ((pb[b] >> 16) & 0xffu);
          const uint32_t cv = (cs + 2u) >> 2, pv = (ps + 2u) >> 2;
          if (q == 0 && b == 0) fc = cv, fp = pv, dc = 0u, dp = 0u;
          dc |= cv ^ fc;
          dp |= pv ^ fp;
          z[zaddr<N>(row, col + q * 4 + b)] = {(float)cv, (float)pv};
        }
      }
    }
    if constexpr (DS != 1) {
      cc = wave_const_code(ld_on, fc, dc);
      cp = wave_const_code(ld_on, fp, dp);
    }
    if (lane == 0) const_code[wave] = cc | (cp << 16);
    wave_sync();
  }

  // ---- forward 2-D transform of z: rows (wave-local), barrier, columns (wave-local)  (dft x2, :1491-1493)
  if constexpr (FWD3) {
    fwd3_rows(z, wave, lane);
    __syncthreads();
    fwd3_mid(z, wave, lane, tw3);
    wave_sync();
    fwd3_cols(z, wave, lane);
  } else {
    row_pass<N, LPW, RAW>(z, wave * LPW, lane, tw_row);
    __syncthreads();
    col_pass_fwd<N>(z, wave * LPW, lane, tw_col);
  }
  __syncthreads();

  // ---- untangle A = FFT(cur), B = FFT(prev); P = A conj(B); C = P|P| / (|P|^2 + eps)
  //      (mulSpectrums :1494, magSpectrums :70-168, divSpectrums :1086-1251, incl. the real-only-slot
  //      behaviour of :107-109 / :1127-1129). Only the half spectrum v < N/2 (+ row N/2 packed into the
  //      imaginary part of row 0) is kept, conjugated, for the Hermitian inverse.
  if constexpr (P::FUSE_XPOW) {
  // rows 0 and H share row 0: G'[u] = conj(C[0][u]) + i conj(C[H][u]) (partner of u is N-u in the same rows), packed
  // by wave 0, which owns row 0 in the pass below; rows 1..H-1 get their cross-power inside row_pass_xpow
  if (wave == 0) {
    for (int u = lane; u <= H; u += 64) {
      const int um = (N - u) % N;
      const bool self = (u == um);
      const cf C0 = cross_power<PK>(z[zaddr<N>(0, u)], z[zaddr<N>(0, um)], self);
      const cf Ch = cross_power<PK>(z[zaddr<N>(H, u)], z[zaddr<N>(H, um)], self);
      if (u == 0) *reinterpret_cast<float*>(const_code + 16) = C0.x;  // C_dc: all that is left of a degenerate pair's spectrum
      z[zaddr<N>(0, u)] = {C0.x + Ch.y, Ch.x - C0.y};
      if (!self) z[zaddr<N>(0, um)] = {C0.x - Ch.y, Ch.x + C0.y};
    }
    wave_sync();
  }
  // ---- inverse (unscaled) of the Hermitian spectrum: forward transforms of conj(C); rows 0..H-1 only,
  //      then column pairs  (idft :1497)
  if (wave == 0) row_pass_xpow<N, PK, true>(z, 0, lane, tw_row);
  else if (wave < P::WI) row_pass_xpow<N, PK, false>(z, wave * P::LI, lane, tw_row);
  } else {
  {
    // rows 1..H-1: every u; partner (N-v, N-u) lies in the untouched lower half. Fixed trip count, so every
    // address is a base plus a compile-time offset.
    {
      constexpr int UPW = (N < 64) ? N : 64;          // columns covered by one wave
      constexpr int RPI = T / UPW;                     // rows covered per iteration
      const int u = tid % UPW, vr = tid / UPW;
      const int um = (N - u) % N;
#pragma unroll
      for (int i = 0; i < (H - 1 + RPI - 1) / RPI; ++i) {
#pragma unroll
        for (int uu = 0; uu < N / UPW; ++uu) {
          const int v = 1 + vr + i * RPI;
          if (v < H) {
            const int uc = u + uu * UPW, umc = (N - uc) % N;
            (void)um;
            const cf zk = z[zaddr<N>(v, uc)], zm = z[zaddr<N>(N - v, umc)];
            const cf C = cross_power<PK>(zk, zm, false);
            z[zaddr<N>(v, uc)] = {C.x, -C.y};  // conj(C[v][u])
          }
        }
      }
    }
    // rows 0 and H share row 0: G'[u] = conj(C[0][u]) + i conj(C[H][u]); partner of u is N-u in the same rows
    for (int u = tid; u <= H; u += T) {
      const int um = (N - u) % N;
      const bool self = (u == um);
      const cf C0 = cross_power<PK>(z[zaddr<N>(0, u)], z[zaddr<N>(0, um)], self);
      const cf Ch = cross_power<PK>(z[zaddr<N>(H, u)], z[zaddr<N>(H, um)], self);
      if (u == 0) *reinterpret_cast<float*>(const_code + 16) = C0.x;  // C_dc (see the fused form above)
      z[zaddr<N>(0, u)] = {C0.x + Ch.y, Ch.x - C0.y};
      if (!self) z[zaddr<N>(0, um)] = {C0.x - Ch.y, Ch.x + C0.y};
    }
  }
  __syncthreads();

  // ---- inverse (unscaled) of the Hermitian spectrum: forward transforms of conj(C); rows 0..H-1 only,
  //      then column pairs  (idft :1497)
  if (wave < P::WI) row_pass<N, P::LI>(z, wave * P::LI, lane, tw_row);
  }  // FUSE_XPOW
  __syncthreads();
  Best best = argmax_neutral();
  // RECORD (N = 64 under cv::phaseCorrelate's peak model): the wave that ends the patch does not run the fp64 finish -- three 64-lane
  // sums, two divisions, the gate: a third of the one-wave section that holds the workgroup's LDS. It stores what the finish needs, 128
  // bytes in one store (pc_store_record), and pc_finish_kernel below, one lane per patch, does the rest for the whole piece.
  constexpr bool RECORD = pc_field_records(N, PK);
  static_assert(RECORD == std::is_same_v<A, PcArgsRecord> && (!RECORD || VALUE_FIRST), "the record forms take PcArgsRecord and reduce the value first");
  if constexpr (VALUE_FIRST) {
    // The value first, the index only where the value matched (the rule and why it gives the parent fold's Best: pc_argmax.hpp). Each
    // lane keeps its 16 surface values; the wave's maximum goes to a float slot in the free part of `red`; behind the barrier every wave
    // forms the workgroup's maximum gm from the WAVES slots. Only a wave that holds a lane with m == gm -- one wave, unless the maximum is
    // attained in several -- walks the index chain and folds (value, index) pairs, all 64 lanes active (lane_xor's contract); the others
    // store the neutral pair. The second barrier, which a one-patch workgroup did not need before, now orders red[] for wave 0.
    static_assert(P::WI == P::WAVES, "every wave runs the inverse column pass");
    float* red_max = reinterpret_cast<float*>(red + 16);  // red[0 .. WAVES-1] pairs; [16, 32) free; the constant-patch codes from 32
    cf sv[InvPlan<N>::PER * R2];
    const float m = col_pass_inv<N, PK, false>(z, wave * P::LI, lane, tw_col, a.search_radius, sv).v;
    const float wm = wave_max(m);
    if (lane == 0) red_max[wave] = wm;
    __syncthreads();
    float gm = red_max[0];
#pragma unroll
    for (int w = 1; w < P::WAVES; ++w) gm = fmaxf(gm, red_max[w]);
    if constexpr (PK == 0) {
      // The wave that holds the maximum ends the patch. A slot equals gm exactly where its wave has a lane with m == gm (m <= the wave's
      // slot <= gm), so every wave counts the same holders. ONE holder -- every surface but a flat, a periodic or an all-NaN one -- : its
      // wave_best is already the workgroup's pair (the other waves would hand in the neutral pair, which loses to it: gm > -inf, or all four
      // slots were equal), so it reads the codes and its window element and ends the patch itself, all 64 lanes active, and the other waves
      // leave: no red[] store, no second barrier, and the one-wave tail falls on whichever SIMD holds the peak. The window read is ordered:
      // every wave stored its part of the surface before the barrier above. Any other count takes the path below: wave 0 behind a second barrier.
      int holders = 0;
#pragma unroll
      for (int w = 0; w < P::WAVES; ++w) holders += red_max[w] == gm ? 1 : 0;
      if (__builtin_amdgcn_readfirstlane(holders) == 1) {
        const unsigned long long mine = __builtin_amdgcn_ballot_w64(m == gm);  // this wave's lanes that hold it
        if (mine == 0ull) return;
        const int my_code = const_code[lane & 15];
        best = holder_pair<N>(sv, m, gm, wave * P::LI, lane, mine);
        const float wv = centroid_window_value<N, PK>(best, lane, [&](int ys, int xs) {
          const int y = (ys + H) % N, x = (xs + H) % N;  // un-shifted position
          const cf s = z[zaddr<N>(y, x % H)];
          return x < H ? s.x : s.y;
        });
        pc_store_record(a.finish, p, lane, best, wv, const_codes_degenerate<P::WAVES>(my_code, lane), const_code);
        return;
      }
    }
    if (const unsigned long long mine = __builtin_amdgcn_ballot_w64(m == gm); mine != 0ull) {
      asm volatile("");  // (keeps the rare branch a branch, as for the constant-patch codes above)
      if constexpr (RECORD) best = holder_pair<N>(sv, m, gm, wave * P::LI, lane, mine);
      else best = wave_best(argmax_entry(m, gm, col_pass_inv_index<N>(sv, m, wave * P::LI, lane)));
    }
    if (lane == 0) red[wave] = best;
  } else {
  if (wave < P::WI) best = col_pass_inv<N, PK>(z, wave * P::LI, lane, tw_col, a.search_radius);
  best = wave_best(best);
  if (lane == 0) red[wave] = best;
  }
  __syncthreads();

  // ---- 5x5 weighted centroid in double + validity gate  (:1337-1383, :1838-1856), wave 0. The window is read
  //      before a second barrier releases the other waves to overwrite the tile with the next patch.
  float wval = 0.f;
  bool degenerate = false;
  if (wave == 0) {
    const int my_code = const_code[lane & 15];
    for (int w = 1; w < P::WAVES; ++w) best = better(best, red[w]);
    wval = centroid_window_value<N, PK>(best, lane, [&](int ys, int xs) {
      const int y = (ys + H) % N, x = (xs + H) % N;  // un-shifted position
      const cf s = z[zaddr<N>(y, x % H)];
      return x < H ? s.x : s.y;
    });
    degenerate = const_codes_degenerate<P::WAVES>(my_code, lane);
  }
  // (only the persistent form needs it: the value-first forms have spent their second barrier above and nothing follows that it could
  // protect; N = 32 keeps it, never measured without: docs/history/retired_switches.md)
  if constexpr (!VALUE_FIRST) __syncthreads();
  if constexpr (RECORD) {
    if (wave == 0) pc_store_record(a.finish, p, lane, best, wval, degenerate, const_code);
  } else if (wave == 0)
    centroid_gate_store<N, PK>(best, wval, lane, a.max_px_speed_sq, a.out + 2 * (size_t)p, a.quality ? a.quality + 2 * (size_t)p : nullptr, degenerate,
                               degenerate ? *reinterpret_cast<const float*>(const_code + 16) : 0.f);
  if constexpr (!OLD_PROLOGUE) break;  // one patch
  }  // persistent loop
}

// the kernel of form (N, ds, ch, pk, OFF) as configure_n and launch_n name it: f(kernel, takes_records)
template <int N, bool OFF, class DS, class CH, class PK, class F>
static hipError_t pc_field_form(DS, CH, PK, F&& f) {
  return f(&pc_field_kernel<N, DS::value, CH::value, PK::value, OFF>, std::is_same<PcFieldArgs<N, PK::value>, PcArgsRecord>{});
}

// The fp64 finish of K1 at 64 (RECORD above), on the same stream behind the field kernel: ONE LANE PER PATCH (a wave per patch would keep
// 65536 waves of c2 busy with one lane's work each). A lane reads its patch's record, forms the three leaves of the 64 lanes of the tail it
// replaces exactly as centroid_gate_store does -- (double)xs * val, (double)ys * val, val, val = 0 beyond lane 24 --, adds them in
// wave_sum3's pairing (pc_finish_tree.hpp: the products are a 24-bit value times a small integer, exact in fp64, so a contraction into a
// fused multiply-add changes nothing) and runs peak_finish<0>, the function K1 ran: same operands, same bits.
constexpr int PC_FINISH_T = 256;
__global__ void __launch_bounds__(PC_FINISH_T) pc_finish_kernel(const uint32_t* __restrict__ records, int total, double max_px_speed_sq,
                                                                double* __restrict__ out, double* __restrict__ quality) {
  const int p = (int)blockIdx.x * PC_FINISH_T + (int)threadIdx.x;
  if (p >= total) return;
  uint32_t w[PC_FINISH_DWORDS];
  const uint4* r = reinterpret_cast<const uint4*>(records + (size_t)PC_FINISH_DWORDS * (size_t)p);
#pragma unroll
  for (int q = 0; q < PC_FINISH_DWORDS / 4; ++q) {
    const uint4 v = r[q];
    w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
  }
  const Best best{__uint_as_float(w[25]), (int)w[26]};
  const bool degenerate = w[27] != 0u;
  const Sum3 s = finish_tree([&](int l) {
    int ys, xs;
    peak_window<0>(best, l, 64, &ys, &xs);
    const double val = (double)(l < 25 ? __uint_as_float(w[l]) : 0.f);
    return Sum3{(double)xs * val, (double)ys * val, val};
  });
  peak_finish<0>(s.cx, s.cy, s.sum, best, 64, 64, degenerate, __uint_as_float(w[28]), max_px_speed_sq, out + 2 * (size_t)p,
                 quality ? quality + 2 * (size_t)p : nullptr);
}

int pc_finish_records(int patch_size, int peak_model, int patches) {
  if (!pc_field_records(patch_size, peak_model)) return 0;
  return patches > 65536 ? patches : 65536;
}

template <int N>
static hipError_t configure_n() {
  const size_t lds = PcTraits<N>::LDS_BYTES + pc_extra_lds();
  const hipError_t e = pc_each_form([&](auto ds, auto ch, auto pk) {
    return pc_field_form<N, false>(ds, ch, pk, [&](auto* kernel, auto) { return pc_raise_lds(kernel, lds); });
  });
  if (e != hipSuccess) return e;
  // the fused window-offset forms: gray and BGR8, the enumeration launch_n dispatches them by
  return pc_each_form<PC_FORMS_CH>([&](auto ds, auto ch, auto pk) {
    return pc_field_form<N, true>(ds, ch, pk, [&](auto* kernel, auto) { return pc_raise_lds(kernel, lds); });
  });
}

template <int N>
static hipError_t launch_n(const PcArgs& a_in, int n_pairs, hipStream_t stream, uint32_t* finish, int finish_records) {
  using Tr = PcTraits<N>;
  PcArgs a = a_in;
  a.total = n_pairs * a.grid_x * a.grid_y;
  const int cus = pc_cu_count();
  a.stagger_div = cus;
  {
    static const int units = [] { const char* e = getenv("MOF_PC_STAGGER"); return e ? atoi(e) : 0; }();
    a.stagger_units = units;
  }
  const dim3 b(Tr::T);
  const size_t lds = Tr::LDS_BYTES + pc_extra_lds();
  auto go = [&](const PcArgs& aa, dim3 g) {
    return [&, g](auto* kernel, auto takes_records) {
      if constexpr (decltype(takes_records)::value) {
        PcArgsRecord ar;
        static_cast<PcArgs&>(ar) = aa;
        ar.finish = finish;
        hipLaunchKernelGGL(kernel, g, b, lds, stream, ar);
      } else {
        hipLaunchKernelGGL(kernel, g, b, lds, stream, aa);
      }
      return hipGetLastError();
    };
  };
  auto launch = [&](const PcArgs& aa, dim3 g) {
    if (aa.prev_off)  // the fused window-offset form; hipErrorInvalidValue for the long-range mode and the OpenCL peak model
      return pc_dispatch_form<PC_FORMS_CH>(aa, [&](auto ds, auto ch, auto pk) { return pc_field_form<N, true>(ds, ch, pk, go(aa, g)); });
    return pc_dispatch_form(aa, [&](auto ds, auto ch, auto pk) { return pc_field_form<N, false>(ds, ch, pk, go(aa, g)); });
  };
  if constexpr (Tr::PERSIST) {
    // as many workgroups as are resident at once (LDS-limited), each loops over patches (c4: +9 % over one per patch)
    const int per_cu = (int)((160u * 1024u) / lds);
    const int resident = cus * (per_cu < 1 ? 1 : (per_cu > 16 ? 16 : per_cu));
    return launch(a, dim3((unsigned)(a.total < resident ? a.total : resident)));
  } else {
    // one workgroup per patch; the pair index rides gridDim.z
    const int patches = a.grid_x * a.grid_y;
    // K1 at 64 under cv::phaseCorrelate's peak model: every piece is the field kernel and then the finish kernel over the piece's records, its
    // own out / quality offsets and the record buffer from its start again -- a piece holds no more patches than the buffer holds records
    const bool record = pc_finish_records(N, a.peak_model, patches) > 0;
    int piece = PC_MAX_GRID_PAIRS;
    if (record) {
      if (!finish || finish_records < patches) return hipErrorInvalidValue;
      if (finish_records / patches < piece) piece = finish_records / patches;
    }
    return pc_split_pairs(a, n_pairs, [&](const PcArgs& c, int nk) {
      const hipError_t e = launch(c, dim3((unsigned)a.grid_x, (unsigned)a.grid_y, (unsigned)nk));
      if (e != hipSuccess || !record) return e;
      hipLaunchKernelGGL(pc_finish_kernel, dim3((unsigned)((c.total + PC_FINISH_T - 1) / PC_FINISH_T)), dim3(PC_FINISH_T), 0, stream, finish,
                         c.total, c.max_px_speed_sq, c.out, c.quality);
      return hipGetLastError();
    }, piece);
  }
}

hipError_t pc_configure(int patch_size) {
  switch (patch_size) {
    case 32: return configure_n<32>();
    case 64: return configure_n<64>();
    case 128: return configure_n<128>();
    case 120: return pc_configure_120();
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_pc_field(const PcArgs& a, int patch_size, int n_pairs, hipStream_t stream, uint32_t* finish, int finish_records) {
  if (a.pitch >= PC_MAX_PITCH) return hipErrorInvalidValue;  // (the 32-bit lane offsets of fetch16; mof_kernels.h)
  switch (patch_size) {
    case 32: return launch_n<32>(a, n_pairs, stream, finish, finish_records);
    case 64: return launch_n<64>(a, n_pairs, stream, finish, finish_records);
    case 128: return launch_n<128>(a, n_pairs, stream, finish, finish_records);
    case 120: return a.prev_off ? hipErrorInvalidValue : launch_pc_field_120(a, n_pairs, stream);  // (the 15 x 8 kernel has no fused form)
    default: return hipErrorInvalidValue;
  }
}

bool pc_patch_size_supported(int n) { return n == 32 || n == 64 || n == 128 || n == 120; }

template <int N>
static void append_rows_n(std::vector<float>& t) {
  using R = TwRows<N>;
  t.resize(R::FLOATS);
  auto copy = [&](size_t at, int k) {  // entry `at` of the appended part <- W_N^k of the classic table, the very floats
    t[at] = t[2 * (size_t)k];
    t[at + 1] = t[2 * (size_t)k + 1];
  };
  for (int x = 0; x < R::R1; ++x)
    for (int k = 0; k < R::R2; ++k) copy(R::ROWS_AT + 2 * (size_t)(x * R::R2 + k), k * x);
  if constexpr (N == 64)
    for (int i = 0; i < 16; ++i)
      for (int k = 0; k < 4; ++k) copy(R::FWD3_AT + 2 * (size_t)(i * 4 + k), k * i);
}

void pc_append_twiddle_rows(std::vector<float>& table, int n) {
  if (table.size() != 2 * (size_t)n) return;  // (not a classic table of that size)
  if (n == 32) append_rows_n<32>(table);
  else if (n == 64) append_rows_n<64>(table);
}

}  // namespace mof
