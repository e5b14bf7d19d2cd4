// fe_kernel.hip -- the camera front end for gfx950 (CDNA4): camera frames in, the gray crop out.
//
// Replaces the node's per-frame front end (/root/reference/src/optic_flow.cpp:1603-1622)
//   cv::resize(image, image_scaled, Size(W / s, H / s))          (INTER_LINEAR, integer scale_factor s)
//   cv::cvtColor(image_scaled(cropping_rectangle), imCurr, CV_RGB2GRAY)
// for a batch of mono8 (CH = 1) or interleaved BGR8 (CH = 3) frames. Any entry that takes gray frames consumes the output.
//
// Arithmetic [published OpenCV algorithm, unpinned]: at an EXACT ratio (W % s == 0, H % s == 0) the fixed-point INTER_LINEAR
// path of cv::resize on 8-bit data reduces, per channel, to closed forms (the reduction oracle/oracle.h documents for the
// long-range quarter). Destination x maps to the source coordinate (x + 0.5) s - 0.5, so
//   odd s (1 included): the single tap src(s y + (s - 1) / 2, s x + (s - 1) / 2)        (coefficients 2048 / 0)
//   even s:             (a + b + c + d + 2) >> 2 over the 2 x 2 block at rows s y + s/2 - 1 .. s y + s/2, same columns
//                       (coefficients 1024 / 1024; at s = 2 OpenCV switches to INTER_AREA, whose fast path gives the same)
// Both forms tap rows and columns from s y + (s - 1) / 2 on (integer division). CH = 3 then goes through rgb2gray_fixed
// (pc_common.hpp; byte 0 gets the R weight, as the node applies CV_RGB2GRAY to BGR data). A mono8 camera needs no gray step:
// toCvCopy(BGR8) replicates the channel and (g * 16384 + 8192) >> 14 = g.
//
// Shape: a streaming kernel, bound by the bytes of the tapped source rows. One lane owns a run of P consecutive output pixels of
// one output row: it reads the 1 (odd s) or 2 (even s) source row segments the run taps with wide loads at
// dword alignment (fe_segment: global_load_dwordx4 and narrower, realigned in registers at any byte origin or pitch) and writes
// its P bytes with one store of P bytes. No LDS. The tap spacing of s = 1 .. 6 is unrolled, P = 16, 8 or 4 so that a row segment
// stays <= 60 bytes and neighbouring lanes read neighbouring segments; other factors, and the ragged last run of a row, take the
// per-pixel path with byte loads.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mof_kernels.h"
#include "pc_common.hpp"  // rgb2gray_fixed

namespace mof {
namespace {

constexpr int FE_THREADS = 256;

// pixels per lane for the unrolled factors; s = 0 stands for every other factor (per-pixel path)
__host__ __device__ constexpr int fe_run_pixels(int ch, int s) {
  return s == 0 ? 4 : (ch * s <= 3 ? 16 : (ch * s <= 6 ? 8 : 4));
}

// one output pixel at scaled coordinates (x, y), any factor: byte loads
template <int CH, bool EVEN>
__device__ __forceinline__ uint32_t fe_pixel(const uint8_t* frame, size_t pitch, int s, int x, int y) {
  const int off = (s - 1) >> 1;
  const uint8_t* r0 = frame + (size_t)(s * y + off) * pitch + (size_t)CH * (size_t)(s * x + off);
  uint32_t v[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if constexpr (EVEN) {
      const uint8_t* r1 = r0 + pitch;
      v[c] = ((uint32_t)r0[c] + r0[CH + c] + r1[c] + r1[CH + c] + 2u) >> 2;
    } else {
      v[c] = r0[c];
    }
  }
  if constexpr (CH == 3) return rgb2gray_fixed(v[0], v[1], v[2]);
  else return v[0];
}

// L bytes from p (any alignment) as dword-aligned loads: out[k] = bytes 4k .. 4k + 3 from p on. The dwords from p & ~3 on are
// loaded whole (global_load_dwordx4 and narrower at dword alignment; the last one only where it holds a byte of the segment, so
// nothing past the segment's last dword is touched) and shifted into place with v_alignbyte_b32, so that no load is byte-misaligned
// (the taps of an even s start at an odd column).
template <int L>
__device__ __forceinline__ void fe_segment(const uint8_t* p, uint32_t* out /*[(L + 3) / 4]*/) {
  constexpr int U = (L + 3) / 4;  // dwords that hold a byte of the segment at any misalignment
  const unsigned d = (unsigned)((uintptr_t)p & 3u);
  const uint32_t* base = (const uint32_t*)__builtin_assume_aligned(p - d, 4);
  uint32_t w[U + 1];
  __builtin_memcpy(w, base, 4 * U);
  w[U] = (d + L > 4u * U) ? base[U] : 0u;
#pragma unroll
  for (int k = 0; k < U; ++k) out[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], d);
}

__device__ __forceinline__ uint32_t fe_byte(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// one lane's run of P output pixels from (x0, y) on, for a factor S known at compile time (S = 0: any factor, per pixel)
template <int CH, bool EVEN, int S>
__device__ __forceinline__ void fe_run(const FeArgs& a, const uint8_t* frame, uint8_t* drow, int x0, int y) {
  constexpr int P = fe_run_pixels(CH, S);
  const int npx = a.crop_w - x0 < P ? a.crop_w - x0 : P;
  const int xs = a.crop_x + x0, ys = a.crop_y + y;
  if (S == 0 || npx < P) {
    for (int j = 0; j < npx; ++j) drow[x0 + j] = (uint8_t)fe_pixel<CH, EVEN>(frame, a.src_pitch, a.scale, xs + j, ys);
    return;
  }
  constexpr int SS = S > 0 ? S : 1;
  constexpr int OFF = (SS - 1) / 2;
  // bytes from the run's first tap to its last one: P - 1 tap spacings plus the last tap's one or two pixels
  constexpr int L = CH * (SS * (P - 1) + (EVEN ? 2 : 1));
  const uint8_t* r0 = frame + (size_t)(SS * ys + OFF) * a.src_pitch + (size_t)CH * (size_t)(SS * xs + OFF);
  uint32_t b0[(L + 3) / 4], b1[EVEN ? (L + 3) / 4 : 1];
  fe_segment<L>(r0, b0);
  if constexpr (EVEN) fe_segment<L>(r0 + a.src_pitch, b1);
  uint8_t o[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    uint32_t v[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int i = CH * SS * j + c;
      if constexpr (EVEN) v[c] = (fe_byte(b0, i) + fe_byte(b0, i + CH) + fe_byte(b1, i) + fe_byte(b1, i + CH) + 2u) >> 2;
      else v[c] = fe_byte(b0, i);
    }
    if constexpr (CH == 3) o[j] = (uint8_t)rgb2gray_fixed(v[0], v[1], v[2]);
    else o[j] = (uint8_t)v[0];
  }
  __builtin_memcpy(drow + x0, o, P);
}

template <int CH, bool EVEN, int S>
__device__ __forceinline__ void fe_body(const FeArgs& a) {
  constexpr int P = fe_run_pixels(CH, S);
  const unsigned t = blockIdx.x * (unsigned)FE_THREADS + threadIdx.x;
  if (t >= a.total) return;
  const int runs = (a.crop_w + P - 1) / P;
  const unsigned per_frame = (unsigned)runs * (unsigned)a.crop_h;
  const unsigned f = t / per_frame, rem = t - f * per_frame;
  const int y = (int)(rem / (unsigned)runs), r = (int)(rem - (unsigned)y * (unsigned)runs);
  const uint8_t* frame = a.src + (size_t)f * a.src_stride;
  uint8_t* drow = a.dst + (size_t)f * a.dst_stride + (size_t)y * a.dst_pitch;
  fe_run<CH, EVEN, S>(a, frame, drow, r * P, y);
}

// two forms (odd / even taps) x CH; the factor is a run-time value, its common values unrolled
template <int CH, bool EVEN>
__global__ void __launch_bounds__(FE_THREADS) fe_kernel(FeArgs a) {
  switch (a.scale) {
    case EVEN ? 2 : 1: fe_body<CH, EVEN, EVEN ? 2 : 1>(a); break;
    case EVEN ? 4 : 3: fe_body<CH, EVEN, EVEN ? 4 : 3>(a); break;
    case EVEN ? 6 : 5: fe_body<CH, EVEN, EVEN ? 6 : 5>(a); break;
    default: fe_body<CH, EVEN, 0>(a); break;
  }
}

}  // namespace

int frontend_run_pixels(int channels, int scale) { return fe_run_pixels(channels, scale <= 6 ? scale : 0); }

hipError_t launch_frontend(const FeArgs& args, int channels, int n_frames, hipStream_t stream) {
  const int P = frontend_run_pixels(channels, args.scale);
  const unsigned long long per_frame = (unsigned long long)((args.crop_w + P - 1) / P) * (unsigned long long)args.crop_h;
  // threads of one launch stay below 2^31 and its frames at 65535 (as the video entries' launches); longer batches go out
  // in several launches
  if (per_frame == 0 || per_frame > (1ull << 31)) return hipErrorInvalidValue;
  unsigned long long fpl = (1ull << 31) / per_frame;
  if (fpl > 65535) fpl = 65535;
  for (long long f0 = 0; f0 < n_frames; f0 += (long long)fpl) {
    const long long nf = n_frames - f0 < (long long)fpl ? n_frames - f0 : (long long)fpl;
    FeArgs a = args;
    a.src = args.src + (size_t)f0 * args.src_stride;
    a.dst = args.dst + (size_t)f0 * args.dst_stride;
    a.total = (unsigned)(per_frame * (unsigned long long)nf);
    const dim3 grid((a.total + FE_THREADS - 1) / FE_THREADS);
    const bool even = (args.scale & 1) == 0;
    if (channels == 3) {
      if (even) hipLaunchKernelGGL((fe_kernel<3, true>), grid, dim3(FE_THREADS), 0, stream, a);
      else hipLaunchKernelGGL((fe_kernel<3, false>), grid, dim3(FE_THREADS), 0, stream, a);
    } else {
      if (even) hipLaunchKernelGGL((fe_kernel<1, true>), grid, dim3(FE_THREADS), 0, stream, a);
      else hipLaunchKernelGGL((fe_kernel<1, false>), grid, dim3(FE_THREADS), 0, stream, a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mof
