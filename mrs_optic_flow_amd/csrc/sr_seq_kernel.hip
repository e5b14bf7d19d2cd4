// sr_seq_kernel.hip -- the scale/rotation estimator's transforms for FRAME SEQUENCES (K5s, K6s) on gfx950.
//
// scaleRotationEstimator::processImage (/root/reference/src/scaleRotationEstimator.cpp:34-148) is a stream processor: from
// the second call on, every frame's log-polar image is `cur` once (:112-117) and -- unless the gate of :119-121 fires --
// `prev` once (:128). Packing (cur, prev) into one complex transform (the retired pair kernels K5 / K6,
// docs/history/retired_switches.md) transforms every frame of a video twice. Here the unit is the frame:
//   K5s sr_rows_real : one log-polar image -> its row half-spectra, two real rows per complex transform, untangled and
//                      written transposed and DOUBLED: Zh[u][v] = 2 * rowDFT(v)[u], u = 0..N/2 (925 KB per 480^2 frame
//                      instead of 1.84 MB of packed Zt per pair)
//   K6s sr_cols_seq  : ONE WAVE owns four columns u and walks a run of consecutive pairs in time: the column spectra of
//                      the previous frame stay in its registers (60 VGPRs), per new frame it reads four lines of Zh,
//                      transforms them in LDS, forms the normalised cross-power spectrum against the registers (same
//                      rules as K1, pc_common.hpp), transforms back and writes the Dt that K7 / K8 of sr_kernel.hip
//                      consume. No workgroup barrier; per pair and column group 8 line transforms, and each Zh line is
//                      read (1 + 1/run) times.
// The stateful single-frame entry (mof_sr_process) runs the SAME kernels with one pair per launch, so a sequence processed
// in one call and the same frames fed one at a time produce identical bits.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mof_kernels.h"
#include "pc_common.hpp"
#include "pc_launch.hpp"
#include "sr_common.hpp"

namespace mof {

namespace {

// ---- K5s: row half-spectra of one real image -------------------------------------------------------------------------
// ROWS image rows per workgroup = ROWS / 2 packed lines, four lines per wave. The transposed store writes ROWS * 8
// contiguous bytes per u.
// 32 image rows per workgroup where N allows (256-byte segments of the transposed store; kept in the A/B against 16 rows = more workgroups per CU).
template <int N>
struct RowsReal {
  static constexpr int ROWS = N > 512 ? 8 : (N % 32 == 0 ? 32 : (N % 16 == 0 ? 16 : 8));  // (200: 25 one-wave workgroups of 8 rows per image; beyond 512: one wave = four lines = up to 31 KB of LDS per workgroup)
  static constexpr bool TAIL = N % ROWS != 0;  // (270, 300, 450: the last one-wave workgroup holds 3, 2 or 1 row pairs; the rest of its lines are zeros and are not stored)
  static_assert((N % ROWS == 0 || ROWS == 8) && ROWS % 8 == 0, "whole workgroups of four-line waves, a tail only behind one-wave workgroups");  // (odd N: the last row shares its line with zeros)
  static constexpr int GROUPS = (N + ROWS - 1) / ROWS;
  static constexpr int LINES = ROWS / 2;
  // lines per wave: four. (r06 A/B: two lines per wave at the long lines, N >= 540 -- twice the waves for the same LDS, as K7 took
  // it -- LOSES here: 576 +9 %, 640 +17 % time, profiles/r06_lpw2_ab.txt)
  static constexpr int LPW = 4;
  static constexpr int T = LINES / LPW * 64;
};

template <int N>
__global__ void __launch_bounds__(RowsReal<N>::T) sr_rows_real_kernel(const uint8_t* __restrict__ lp, size_t lp_stride,
                                                                       const float* __restrict__ twiddles,
                                                                       float* __restrict__ zh, size_t zh_stride) {
  using P = SrPlan<N>;
  using R = RowsReal<N>;
  constexpr int H = N / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char rr_lds[];
  cf* z = reinterpret_cast<cf*>(rr_lds);  // [LINES][LINE]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, frame = blockIdx.y, row0 = blockIdx.x * R::ROWS;
  SrTw<N> tw;
  tw.load(twiddles, lane);
  // wave w owns rows row0 + 8w .. +7 = lines 4w .. 4w+3: line l = rows (2l, 2l+1) as real and imaginary part
  const uint8_t* img = lp + (size_t)frame * lp_stride + (size_t)(row0 + 8 * wave) * N;
  cf* mine = z + 4 * wave * P::LINE;
  {
    constexpr int ND = N / 4, NL = (4 * ND + 63) / 64;  // dwords per row; (even, odd) dword pairs per lane
    uint32_t c[NL], p[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) {  // all loads first, then the conversion (convertTo CV_32FC1, :115)
      const int i = lane + 64 * k;
      if (i < 4 * ND) {
        const int l = i / ND, d = i % ND;
        c[k] = stream_load(reinterpret_cast<const uint32_t*>(img + (size_t)(2 * l) * N + 4 * d));
        p[k] = stream_load(reinterpret_cast<const uint32_t*>(img + (size_t)(2 * l + 1) * N + 4 * d));
      }
    }
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const int i = lane + 64 * k;
      if (i < 4 * ND) {
        const int l = i / ND, d = i % ND;
        // (a lane's four pixels go out in the order rotated by d / 4: lanes 4 apart -- 32 B x 4 = one bank wrap -- would otherwise
        //  hit the same bank with every one of their four stores: 38 % of this kernel's LDS cycles were conflicts, r04 counters)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = (q + (d >> 2)) & 3;
          mine[l * P::LINE + 4 * d + r] = {(float)((c[k] >> (8 * r)) & 0xffu), (float)((p[k] >> (8 * r)) & 0xffu)};
        }
      }
    }
  }
  wave_sync();
  wave_fft<N>(mine, 4, lane, tw, StoreNatural<N>{});
  __syncthreads();
  // untangle the two rows of every line and store transposed: Zh[u][row0 + 2j], Zh[u][row0 + 2j + 1] are neighbours
  cf* out = reinterpret_cast<cf*>(zh + (size_t)frame * zh_stride) + row0;
  for (int i = tid; i < R::LINES * (H + 1); i += R::T) {
    const int u = i / R::LINES, j = i % R::LINES;
    const cf zk = z[j * P::LINE + u], zm = z[j * P::LINE + (N - u) % N];
    cf a2, b2;
    untangle2(zk, zm, &a2, &b2);  // 2 * DFT(row 2j)[u], 2 * DFT(row 2j + 1)[u]
    stream_store(reinterpret_cast<float4*>(out + (size_t)u * sr_zh_pitch<N>() + 2 * j), make_float4(a2.x, a2.y, b2.x, b2.y));
  }
}

// ---- K5s on PATCHES OF FRAMES (r04): FftMethod patches of 240 / 256 / 480 pixels -- the reference's whole-frame fallback
// (FftMethod.cpp:1709-1716) among them -- are exactly this estimator's transform sizes, so the large-patch pipeline of the FFT
// engine (pc_large_kernel.hip) hands them to the tuned K5s / K6s / K7 instead of its planned L5 / L6 / L7. The only difference
// to sr_rows_real_kernel is where the pixels come from (image f = 2 (pair * patches + patch) + (0 cur | 1 prev), any row pitch,
// gray or BGR8 through the node's CV_RGB2GRAY) and the constant-image flags the FFT tail wants (as pcl_rows_kernel sets them).
template <int N, int CH, bool PAD>  // PAD: n < N, the patch is zero-padded to the transform size (the unpadded form pays nothing for it)
__global__ void __launch_bounds__(RowsReal<N>::T) sr_rows_real_src_kernel(PclSrc src, const float* __restrict__ twiddles,
                                                                           float* __restrict__ zh, size_t zh_stride, int* __restrict__ flags, int n,
                                                                           int* __restrict__ sums) {
  using P = SrPlan<N>;
  using R = RowsReal<N>;
  constexpr int H = N / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char rr_lds[];
  cf* z = reinterpret_cast<cf*>(rr_lds);  // [LINES][LINE]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, img = blockIdx.y, row0 = blockIdx.x * R::ROWS;
  const int patches = src.grid_x * src.grid_y;
  const int which = src.paired == 2 ? 0 : (img & 1), q = src.paired == 2 ? img : (img >> 1);  // (a video: image = frame * patches + patch, `pair` = the frame)
  const int pair = q / patches, pt = q - pair * patches, by = pt / src.grid_x, bx = pt - by * src.grid_x;
  const uint8_t* base = src.base[which] + (size_t)pair * src.stride[which] + (size_t)(src.origin_y + by * src.stride_y) * src.pitch +
                        (size_t)(CH * (src.origin_x + bx * src.stride_x));
  SrTw<N> tw;
  tw.load(twiddles, lane);
  // r06: n < N -- a patch that cv::phaseCorrelate zero-pads to this transform size (copyMakeBorder): rows and columns beyond n are zeros
  // and take no part in the constant-image test (`inside`)
  // EDGE: some chunk of some line may lie (partly) outside the pixels to read -- a padded patch, a row length that is not a multiple of
  // four (270, 450: the last chunk of a row holds two pixels), or the zero lines behind the image in the last workgroup (RowsReal::TAIL)
  constexpr bool EDGE = PAD || (N % 4 != 0) || R::TAIL;
  const int ne = PAD ? n : N;
  auto px4 = [&](int y, int d) -> uint32_t {  // pixels 4d .. 4d+3 of patch row y, one byte each
    // EDGE, branch-free (r06): the load itself is unconditional -- row min(y, ne - 1), the four pixels that END no later than the row does --
    // and what lies outside the patch is shifted / masked away afterwards. With a branch per chunk (rows past the patch, the half-full last
    // chunk in a byte loop) every chunk's load waited for the previous one's: the sizes with a tail (250, 270, 300, 450) ran 1.7 x slower per
    // pixel than their neighbours (tools/size_probe.py).
    const int yc = EDGE ? (y < ne ? y : ne - 1) : y;
    const int xc = EDGE ? (4 * d < ne - 4 ? 4 * d : ne - 4) : 4 * d;
    const uint8_t* r = base + (size_t)yc * src.pitch + (size_t)CH * xc;
    uint32_t v;
    if constexpr (CH == 1) {
      __builtin_memcpy(&v, r, 4);  // (any alignment: the patch origin and the pitch are the caller's)
    } else {
      v = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) v |= rgb2gray_fixed(r[3 * b], r[3 * b + 1], r[3 * b + 2]) << (8 * b);
    }
    if constexpr (EDGE) {
      const int sh = 4 * d - xc;  // 0: a whole chunk; 1 .. 3: the last chunk of a row whose length is not a multiple of four; >= 4: past the row
      v = sh >= 4 ? 0u : v >> (8 * (sh & 3));
      v = y < ne ? v : 0u;
    }
    return v;
  };
  auto inside = [&](int y, int d) -> uint32_t {  // byte mask of the chunk's pixels that lie inside the n x n patch
    if (!EDGE) return 0xffffffffu;
    if (y >= ne || 4 * d >= ne) return 0u;
    return 4 * d + 3 < ne ? 0xffffffffu : (1u << (8 * (ne - 4 * d))) - 1u;
  };
  const uint32_t p00 = px4(0, 0) & 0xffu, pat = p00 * 0x01010101u;
  uint32_t diff = 0u;
  int s00 = 0, s01 = 0, s10 = 0, s11 = 0;
  constexpr int LPW = R::LPW;  // lines of this wave
  cf* mine = z + LPW * wave * P::LINE;
  {
    constexpr int ND = (N + 3) / 4, NL = (LPW * ND + 63) / 64;  // (N = 270, 450: the last chunk of a row is half full)
    uint32_t c[NL], p[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const int i = lane + 64 * k;
      if (i < LPW * ND) {
        const int l = i / ND, d = i % ND, y = row0 + 2 * LPW * wave + 2 * l;
        c[k] = px4(y, d);
        p[k] = px4(y + 1, d);
      }
    }
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const int i = lane + 64 * k;
      if (i < LPW * ND) {
        const int l = i / ND, d = i % ND, y = row0 + 2 * LPW * wave + 2 * l;
        diff |= ((c[k] ^ pat) & inside(y, d)) | ((p[k] ^ pat) & inside(y + 1, d));
        if constexpr (!SrNyqExact<P>::value) {
          // the four exact integer sums of the image (pixels outside the patch were loaded as zeros): row y is even, y + 1 odd; byte b of a chunk
          // is column 4 d + b, so the byte parity is the column parity
          const int ce = (int)((c[k] & 0xffu) + ((c[k] >> 16) & 0xffu)), co = (int)(((c[k] >> 8) & 0xffu) + (c[k] >> 24));
          const int pe = (int)((p[k] & 0xffu) + ((p[k] >> 16) & 0xffu)), po = (int)(((p[k] >> 8) & 0xffu) + (p[k] >> 24));
          s00 += ce + co + pe + po;
          s01 += ce - co + pe - po;  // (-1)^x
          s10 += ce + co - pe - po;  // (-1)^y
          s11 += ce - co - pe + po;  // (-1)^(x + y)
        }
#pragma unroll
        for (int b = 0; b < 4; ++b)
          mine[l * P::LINE + 4 * d + b] = {(float)((c[k] >> (8 * b)) & 0xffu), (float)((p[k] >> (8 * b)) & 0xffu)};
      }
    }
  }
  if constexpr (!SrNyqExact<P>::value) {
    s00 = wave_sum(s00);
    s01 = wave_sum(s01);
    s10 = wave_sum(s10);
    s11 = wave_sum(s11);
    if (lane == 0 && sums) {  // (zeroed by the caller; 255 * 432^2 < 2^31)
      int* q = sums + (size_t)(src.sums_stride ? src.sums_stride : 4) * img;
      atomicAdd(&q[0], s00);
      atomicAdd(&q[1], s01);
      atomicAdd(&q[2], s10);
      atomicAdd(&q[3], s11);
    }
  }
  if (flags) {  // bit 0: some pixel differs from pixel (0, 0); bit 1: pixel (0, 0) is not zero (zeroed by the caller)
    if (__builtin_amdgcn_ballot_w64(diff != 0u) != 0ull && lane == 0) atomicOr(&flags[img], 1);
    if (blockIdx.x == 0 && tid == 0 && p00 != 0u) atomicOr(&flags[img], 2);
  }
  wave_sync();
  wave_fft<N>(mine, LPW, lane, tw, StoreNatural<N>{});
  __syncthreads();
  cf* out = reinterpret_cast<cf*>(zh + (size_t)img * zh_stride) + row0;
  for (int i = tid; i < R::LINES * (H + 1); i += R::T) {
    const int u = i / R::LINES, j = i % R::LINES;
    if (R::TAIL && row0 + 2 * j >= N) continue;
    const cf zk = z[j * P::LINE + u], zm = z[j * P::LINE + (N - u) % N];
    cf a2, b2;
    untangle2(zk, zm, &a2, &b2);
    stream_store(reinterpret_cast<float4*>(out + (size_t)u * sr_zh_pitch<N>() + 2 * j), make_float4(a2.x, a2.y, b2.x, b2.y));
  }
}

// ---- K6s: column transforms + cross-power + inverse columns, one wave walking a run of pairs -------------------------
constexpr int SEQ_CW = 4;  // columns per wave
// (r06) the long lines: two columns per wave -- half the LDS, half of the previous-image spectra in registers (from 640 on four columns put
// those in AGPRs at one wave per SIMD: VALU 22 % / LDS 23 % at 720, profiles/r06_l720_sq_pmc.csv), and with a first radix above 16 the second
// stage takes two lines per pass anyway. SEQ_CW_BIG_FROM: first N of the two-column form
constexpr int SEQ_CW_BIG_FROM = 540;
template <int N>
constexpr int seq_cw() {
  // (two columns wherever the first radix is above 16 -- every N >= 540, and 324 / 486 / 500: 324 +10 %, 500 +5 %, 486 -1 %)
  return (SrPlan<N>::R1 > 16 || N >= SEQ_CW_BIG_FROM) ? 2 : SEQ_CW;
}

template <int N, bool BOX = false>  // BOX: patches zero-padded to N -- the box-zero rule of padded CONSTANT patches (the plain form pays nothing for it)
__global__ void __launch_bounds__(64) sr_cols_seq_kernel(const float* __restrict__ zh_prev, const float* __restrict__ zh_cur,
                                                         size_t zh_stride, const float* __restrict__ twiddles,
                                                         float* __restrict__ Dt, int n_pairs, int run, const int* __restrict__ flags, int n,
                                                         const int* __restrict__ sums_prev, const int* __restrict__ sums_cur, int sums_stride) {
  using P = SrPlan<N>;
  constexpr int H = N / 2, CW = seq_cw<N>();
  constexpr int MV = (N + 63) / 64;       // bins per lane and line (v = lane + 64 m)
  constexpr bool ODD = (N & 1) != 0;      // (r06) no Nyquist bin: only bin (0, 0) is real-only; Dt rows are not 16-byte aligned
  constexpr int NQ = (N + 1) / 2;         // 16-byte pieces of a line (odd N: the last one carries an element past the line)
  constexpr int MQ = (NQ + 63) / 64;      // 16-byte pieces per lane and line
  __shared__ cf z[CW * P::LINE];
  const int lane = threadIdx.x, u0 = blockIdx.x * CW, p0 = blockIdx.y * run;
  const int np = n_pairs - p0 < run ? n_pairs - p0 : run;
  SrTw<N> tw;
  tw.load(twiddles, lane);

  // four lines of one frame's Zh (columns u0 .. u0+3, clamped in the tail group) -> LDS -> column transforms in place
  auto load_cols = [&](const float* frame) {
    const cf* Zf = reinterpret_cast<const cf*>(frame);
    float4 t[CW][MQ];
#pragma unroll
    for (int s = 0; s < CW; ++s) {
      const int u = u0 + s > H ? H : u0 + s;
#pragma unroll
      for (int m = 0; m < MQ; ++m) {
        const int q = lane + 64 * m;
        if (q < NQ) t[s][m] = stream_load(reinterpret_cast<const float4*>(Zf + (size_t)u * sr_zh_pitch<N>() + 2 * q));
      }
    }
#pragma unroll
    for (int s = 0; s < CW; ++s)
#pragma unroll
      for (int m = 0; m < MQ; ++m) {
        const int q = lane + 64 * m;
        if (q < NQ) {
          z[s * P::LINE + 2 * q] = {t[s][m].x, t[s][m].y};
          z[s * P::LINE + 2 * q + 1] = {t[s][m].z, t[s][m].w};
        }
      }
    wave_sync();
    wave_fft<N>(z, CW, lane, tw, StoreNatural<N>{});
  };

  cf ap[CW][MV];  // column spectra of the previous frame (doubled): 2 B[v][u]
  load_cols(zh_prev + (size_t)p0 * zh_stride);
#pragma unroll
  for (int s = 0; s < CW; ++s)
#pragma unroll
    for (int m = 0; m < MV; ++m) {
      const int v = lane + 64 * m;
      ap[s][m] = v < N ? lds_read(&z[s * P::LINE + v]) : cf{0.f, 0.f};
    }
  wave_sync();
  // r06, FftMethod patches zero-padded to this transform size (n < N; `flags` as pcl_rows_kernel sets them, image 2 p = cur, 2 p + 1 = prev): a
  // CONSTANT patch became an n x n box whose spectrum is exactly zero on the multiples of box_zero_period(n, N) -- the rows were transformed
  // in pairs, their alternating sums carry rounding, and the normalisation would blow those bins up to unit magnitude: C = 0 there, the
  // rule of pcl_cols_kernel (pc_large_kernel.hip) and of the in-LDS kernels (pc_common.hpp)
  const int zq = BOX ? box_zero_period(n, N) : N + 1;
  for (int j = 0; j < np; ++j) {
    load_cols(zh_cur + (size_t)(p0 + j) * zh_stride);
    bool box_zeros = false;
    if constexpr (BOX) box_zeros = __builtin_amdgcn_readfirstlane((int)(((flags[2 * (p0 + j)] & 1) == 0) || ((flags[2 * (p0 + j) + 1] & 1) == 0))) != 0;
    // normalised cross-power spectrum of bins (v, u), conjugated in place; the current spectra move into the registers
#pragma unroll
    for (int s = 0; s < CW; ++s) {
      const int u = u0 + s > H ? H : u0 + s;
      const bool u_edge = u == 0 || (!ODD && u == H);
#pragma unroll
      for (int m = 0; m < MV; ++m) {
        const int v = lane + 64 * m;
        const int vv = v < N ? v : N - 1;  // (lanes past the line repeat its last bin: the wave-uniform branch inside
        const cf a = lds_read(&z[s * P::LINE + vv]);  //  cross_power_ab wants every lane to take part)
        cf av = a, bv = ap[s][m];
        if constexpr (!SrNyqExact<P>::value) {
          // the four real-only CCS slots from the images' exact integer sums (doubled as the spectra are: Zh = 2 x the row transform): bins
          // (v, u) in {0, N/2}^2 -> sums[(v ? 2 : 0) + (u ? 1 : 0)] = sum (+-1)^y (+-1)^x p  (run = 1: one pair per wave walk)
          if (u_edge && (vv == 0 || (!ODD && vv == H))) {
            const int slot = (vv == H ? 2 : 0) + (u == H ? 1 : 0);
            av = {2.f * (float)sums_cur[(size_t)(p0 + j) * sums_stride + slot], 0.f};
            bv = {2.f * (float)sums_prev[(size_t)(p0 + j) * sums_stride + slot], 0.f};
          }
        }
        cf C = cross_power_ab(av, bv, u_edge && (vv == 0 || (!ODD && vv == H)));
        if constexpr (BOX) {
          if (box_zeros && (box_zero_line(u, zq) || box_zero_line(vv, zq))) C = {0.f, 0.f};
        }
        ap[s][m] = a;
        if (v < N) z[s * P::LINE + v] = {C.x, -C.y};
      }
    }
    wave_sync();
    wave_fft<N>(z, CW, lane, tw, StoreNatural<N>{});
    cf* D = reinterpret_cast<cf*>(Dt) + (size_t)(p0 + j) * (H + 1) * N;
    if constexpr (ODD) {  // rows of N complex start on odd multiples of 8 bytes: element stores
#pragma unroll
      for (int s = 0; s < CW; ++s) {
        const int u = u0 + s;
#pragma unroll
        for (int m = 0; m < MV; ++m) {
          const int v = lane + 64 * m;
          if (v < N && u <= H) D[(size_t)u * N + v] = z[s * P::LINE + v];
        }
      }
    } else {
#pragma unroll
      for (int s = 0; s < CW; ++s) {
        const int u = u0 + s;
  #pragma unroll
        for (int m = 0; m < MQ; ++m) {
          const int q = lane + 64 * m;
          if (q < N / 2 && u <= H) {
            const cf a0 = z[s * P::LINE + 2 * q], a1 = z[s * P::LINE + 2 * q + 1];
            stream_store(reinterpret_cast<float4*>(D + (size_t)u * N + 2 * q), make_float4(a0.x, a0.y, a1.x, a1.y));
          }
        }
      }
    }
    wave_sync();
  }
}

// what processImage returns for the very first frame of a sequence (scaleRotationEstimator.cpp:74): (1, 0), no pt -- and, where the call
// asked for quality, (NaN, NaN): no correlation ran
__global__ void sr_identity_kernel(double* __restrict__ out, double* __restrict__ quality) {
  if (threadIdx.x < 4) out[threadIdx.x] = threadIdx.x == 0 ? 1.0 : 0.0;
  else if (threadIdx.x < 6 && quality) quality[threadIdx.x - 4] = __builtin_nan("");
}

template <int N>
hipError_t launch_rows_real_n(const uint8_t* lp, size_t lp_stride, const float* tw, float* zh, size_t zh_stride, int n_frames,
                              hipStream_t stream) {
  using R = RowsReal<N>;
  static_assert(N % R::ROWS == 0, "rows divide evenly over the workgroups");
  constexpr size_t lds = sizeof(cf) * R::LINES * SrPlan<N>::LINE;
  const hipError_t e = pc_raise_lds_beyond_default(&sr_rows_real_kernel<N>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sr_rows_real_kernel<N>, dim3(N / R::ROWS, (unsigned)n_frames), dim3(R::T), lds, stream, lp, lp_stride, tw, zh,
                     zh_stride);
  return hipGetLastError();
}

template <int N>
hipError_t launch_rows_real_src_n(const PclSrc& src, const float* tw, float* zh, size_t zh_stride, int* flags, int n_images, int channels,
                                  int n, int* sums, hipStream_t stream) {
  using R = RowsReal<N>;
  constexpr size_t lds = sizeof(cf) * R::LINES * SrPlan<N>::LINE;
  const bool pad = n < N;
  auto kernel = channels == 3 ? (pad ? &sr_rows_real_src_kernel<N, 3, true> : &sr_rows_real_src_kernel<N, 3, false>)
                              : (pad ? &sr_rows_real_src_kernel<N, 1, true> : &sr_rows_real_src_kernel<N, 1, false>);
  const hipError_t e = pc_raise_lds_beyond_default(kernel, lds);
  if (e != hipSuccess) return e;
  for (int f0 = 0; f0 < n_images; f0 += PC_MAX_GRID_IMAGES) {  // (the image index rides gridDim.y; even chunks keep cur | prev pairs together)
    const int nf = n_images - f0 < PC_MAX_GRID_IMAGES ? n_images - f0 : PC_MAX_GRID_IMAGES;
    PclSrc s = src;
    const int patches = src.grid_x * src.grid_y;
    const int per_unit = src.paired == 2 ? patches : 2 * patches;  // images per frame (a video) / per frame pair
    if (f0 % per_unit != 0) return hipErrorInvalidValue;  // (the caller splits at whole frames / frame pairs: mof_capi.hip)
    s.base[0] += (size_t)(f0 / per_unit) * src.stride[0];
    if (src.paired != 2) s.base[1] += (size_t)(f0 / per_unit) * src.stride[1];
    const dim3 g(R::GROUPS, (unsigned)nf), b(R::T);
    float* zo = zh + (size_t)f0 * zh_stride;
    int* fl = flags ? flags + f0 : nullptr;
    int* su = sums ? sums + (size_t)(src.sums_stride ? src.sums_stride : 4) * f0 : nullptr;
    hipLaunchKernelGGL(kernel, g, b, lds, stream, s, tw, zo, zh_stride, fl, n, su);
  }
  return hipGetLastError();
}

template <int N>
hipError_t launch_cols_seq_n(const float* zh_prev, const float* zh_cur, size_t zh_stride, const float* tw, float* Dt, int n_pairs,
                             int run, const int* flags, int n, const int* sums_prev, const int* sums_cur, int sums_stride, hipStream_t stream) {
  if (!SrNyqExact<SrPlan<N>>::value && (!sums_prev || !sums_cur)) return hipErrorInvalidValue;  // (this plan's real-only slots come from the exact sums; a run
  // of pairs in time finds pair j's quadruples at (p0 + j) * sums_stride of either pointer -- sums that live inside the Zh slots walk with them)
  constexpr int H = N / 2;
  const unsigned groups = (H + 1 + seq_cw<N>() - 1) / seq_cw<N>(), runs = (unsigned)((n_pairs + run - 1) / run);
  if (flags && n < N) hipLaunchKernelGGL((sr_cols_seq_kernel<N, true>), dim3(groups, runs), dim3(64), 0, stream, zh_prev, zh_cur, zh_stride, tw, Dt, n_pairs, run, flags, n, sums_prev, sums_cur, sums_stride);
  else hipLaunchKernelGGL((sr_cols_seq_kernel<N, false>), dim3(groups, runs), dim3(64), 0, stream, zh_prev, zh_cur, zh_stride, tw, Dt, n_pairs, run, flags, n, sums_prev, sums_cur, sums_stride);
  return hipGetLastError();
}

}  // namespace

size_t sr_zh_floats(int res) { return (size_t)(res / 2 + 1) * (((res + 7) & ~7) + 8) * 2; }  // (pitch: sr_zh_pitch)

hipError_t launch_sr_identity(double* out, double* quality, hipStream_t stream) {
  hipLaunchKernelGGL(sr_identity_kernel, dim3(1), dim3(64), 0, stream, out, quality);
  return hipGetLastError();
}

hipError_t launch_sr_rows_real(const uint8_t* lp, size_t lp_stride, const float* twiddles, float* zh, size_t zh_stride, int res,
                               int n_frames, hipStream_t stream) {
  if (n_frames <= 0) return hipSuccess;
  switch (res) {
    case 240: return launch_rows_real_n<240>(lp, lp_stride, twiddles, zh, zh_stride, n_frames, stream);
    case 256: return launch_rows_real_n<256>(lp, lp_stride, twiddles, zh, zh_stride, n_frames, stream);
    case 480: return launch_rows_real_n<480>(lp, lp_stride, twiddles, zh, zh_stride, n_frames, stream);
    default: {
      // (r06) the other tuned sizes: the frame form of the row kernel that the FFT engine's large patches use -- tightly packed log-polar
      // images are ONE patch per "frame" of a video whose patch is the whole image
      PclSrc src{};
      src.base[0] = lp;
      src.stride[0] = lp_stride;
      src.pitch = (size_t)res;
      src.paired = 2;
      src.grid_x = src.grid_y = 1;
      src.stride_x = src.stride_y = res;
      return launch_sr_rows_real_src(SrRowsSrc{src, twiddles, zh, zh_stride, nullptr, res, 1, res, nullptr}, n_frames, stream);
    }
  }
}

hipError_t launch_sr_rows_real_src(const SrRowsSrc& a, int n_images, hipStream_t stream) {
  if (n_images <= 0) return hipSuccess;
  if ((a.src.paired != 1 && a.src.paired != 2) || (a.channels != 1 && a.channels != 3) || a.n < 2 || a.n > a.res) return hipErrorInvalidValue;
  return sr_dispatch_size(a.res, [&](auto n) {
    return launch_rows_real_src_n<decltype(n)::value>(a.src, a.twiddles, a.zh, a.zh_stride, a.flags, n_images, a.channels, a.n, a.sums, stream);
  });
}

hipError_t launch_sr_cols_seq(const SrColsSeq& a, int n_pairs, hipStream_t stream) {
  if (n_pairs <= 0) return hipSuccess;
  const int run = a.run < 1 ? 1 : a.run;
  if (a.flags && run != 1) return hipErrorInvalidValue;  // (the box-zero flags are per independent pair: image 2 p = cur, 2 p + 1 = prev)
  // a run longer than one pair walks cur(p) as prev(p + 1): only valid for a contiguous sequence
  if (run > 1 && a.zh_cur != a.zh_prev + a.zh_stride) return hipErrorInvalidValue;
  return sr_dispatch_size(a.res, [&](auto n) {
    return launch_cols_seq_n<decltype(n)::value>(a.zh_prev, a.zh_cur, a.zh_stride, a.twiddles, a.Dt, n_pairs, run, a.flags, a.n <= 0 ? a.res : a.n,
                                                 a.sums_prev, a.sums_cur, a.sums_stride, stream);
  });
}

// K6s's columns per wave at transform size res (seq_cw), 0 where it has no instantiation
int sr_seq_columns_per_wave(int res) {
  int cw = 0;
  (void)sr_dispatch_size(res, [&](auto n) {
    cw = seq_cw<decltype(n)::value>();
    return hipSuccess;
  });
  return cw;
}

}  // namespace mof
