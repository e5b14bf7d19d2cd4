// pc_offset_kernel.hip -- predicted-shift window offsets for the FFT engine (include/mof.h, "Predicted-shift window offsets"): small
// kernels AROUND the field's kernels. On the gather route (MOF_PRED_ROUTE_GATHER, the default) none of the field's kernels changes: the
// displaced previous window is materialised (1.). On the fused route (MOF_PRED_ROUTE_FUSED) K1 and K1h read it themselves -- a change of
// the previous patch's base address, scalar per workgroup (pc_kernel.hip, pc_half_kernel.hip: OFF) -- and only the clamp (1b.) runs first.
//
//  1. pc_offset_gather_kernel, before the field: one workgroup per (pair, patch). It clamps the patch's prediction p to the applied
//     prediction a (pred_clamp_axis, mof_kernels.h), stores a, and copies the n x n bytes of prev at (x0 - a_x, y0 - a_y) into the
//     engine's scratch frame at (x0, y0). The scratch has the caller's pitch, so the field's kernels run on it as on any prev frame.
//     Everything per patch -- the patch's coordinates, the two loads of p, the clamp, the two base addresses -- depends on blockIdx
//     alone: scalar loads and scalar arithmetic. The copy moves 16 bytes per lane and step: a load from the unaligned source (the
//     form K1's fetch16 takes at origin (1, 1)) and a store of the same width; the last chunk of a row whose n is no multiple of
//     16 starts at n - 16 and overlaps its neighbour with the same bytes. n < 16 copies bytes.
//  1b. pc_offset_clamp_kernel (the fused route): one lane per patch, a = clamp(p) stored, no copy.
//  2. pc_offset_finish_kernel, behind the field and the response gate: one lane per patch, total = a + residual, the speed gate on
//     the total. Shaped like the gate kernel.
//  3. pc_pred_from_coarse_kernel: one lane per fine patch, p = rint(4 s) of its long-range patch (pred_from_coarse, mof_kernels.h).
// No LDS anywhere. Included by mof_capi.hip, the only caller (csrc/Makefile): not a translation unit of its own.

#include <hip/hip_runtime.h>

#include "mof_kernels.h"

namespace mof {
namespace {
typedef double offset_xy __attribute__((ext_vector_type(2), aligned(8)));
typedef int32_t offset_ixy __attribute__((ext_vector_type(2), aligned(4)));  // (a caller's int32 buffer)
struct Chunk16 {
  uint32_t w[4];
};

__global__ void __launch_bounds__(256) pc_offset_gather_kernel(PcOffsetArgs a, unsigned q0) {
  // ---- uniform per workgroup
  const unsigned q = q0 + blockIdx.x;  // patch of the launch: pair * patches + patch
  const unsigned patches = (unsigned)(a.grid_x * a.grid_y);
  const unsigned pair = q / patches, pt = q % patches;
  const int x0 = a.origin_x + (int)(pt % (unsigned)a.grid_x) * a.stride_x;
  const int y0 = a.origin_y + (int)(pt / (unsigned)a.grid_x) * a.stride_y;
  const int32_t ax = pred_clamp_axis(a.pred[2 * (size_t)q], x0, a.frame_w, a.n);
  const int32_t ay = pred_clamp_axis(a.pred[2 * (size_t)q + 1], y0, a.frame_h, a.n);
  // source window (x0 - ax, y0 - ay): inside [0, w - n] x [0, h - n] by the clamp
  const uint8_t* src = a.prev + (size_t)pair * a.prev_stride + (size_t)(y0 - ay) * a.pitch + (size_t)(x0 - ax);
  uint8_t* dst = a.scratch + (size_t)pair * ((size_t)a.frame_h * a.pitch) + (size_t)y0 * a.pitch + (size_t)x0;
  const int n = a.n;
  if (threadIdx.x == 0) *reinterpret_cast<offset_ixy*>(a.applied + 2 * (size_t)q) = offset_ixy{ax, ay};
  // ---- per lane
  if (n >= 16) {
    const int cpr = (n + 15) >> 4, chunks = n * cpr;  // chunks per row, per patch
    for (int c = (int)threadIdx.x; c < chunks; c += (int)blockDim.x) {
      const int row = c / cpr, k = c - row * cpr;
      const int col = k * 16 < n - 16 ? k * 16 : n - 16;
      Chunk16 v;
      __builtin_memcpy(&v, src + (size_t)row * a.pitch + col, 16);
      __builtin_memcpy(dst + (size_t)row * a.pitch + col, &v, 16);
    }
  } else {
    for (int c = (int)threadIdx.x; c < n * n; c += (int)blockDim.x) {
      const int row = c / n, col = c - row * n;
      dst[(size_t)row * a.pitch + col] = src[(size_t)row * a.pitch + col];
    }
  }
}

// the gather kernel's clamp without the copy (the fused route): one lane per patch. The fused field kernels read ONLY what this kernel
// stored -- never a caller's raw prediction --: the clamp is what keeps their displaced loads inside the frame.
__global__ void __launch_bounds__(256) pc_offset_clamp_kernel(PcOffsetArgs a, size_t n_patches) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n_patches) return;
  const unsigned patches = (unsigned)(a.grid_x * a.grid_y);
  const unsigned pt = (unsigned)(q % patches);
  const int x0 = a.origin_x + (int)(pt % (unsigned)a.grid_x) * a.stride_x;
  const int y0 = a.origin_y + (int)(pt / (unsigned)a.grid_x) * a.stride_y;
  const offset_ixy p = *reinterpret_cast<const offset_ixy*>(a.pred + 2 * q);
  *reinterpret_cast<offset_ixy*>(a.applied + 2 * q) =
      offset_ixy{pred_clamp_axis(p.x, x0, a.frame_w, a.n), pred_clamp_axis(p.y, y0, a.frame_h, a.n)};
}

__global__ void __launch_bounds__(256) pc_offset_finish_kernel(double* __restrict__ out, const int32_t* __restrict__ applied, size_t n_patches,
                                                               double max_px_speed_sq) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_patches) return;
  const offset_ixy a = *reinterpret_cast<const offset_ixy*>(applied + 2 * i);
  if ((a.x | a.y) == 0) return;  // total = residual: its bits, its own gate
  const offset_xy r = *reinterpret_cast<const offset_xy*>(out + 2 * i);
  double dx = a.x != 0 ? (double)a.x + r.x : r.x;
  double dy = a.y != 0 ? (double)a.y + r.y : r.y;
  if ((r.x != r.x) || (r.y != r.y) || (dx * dx + dy * dy > max_px_speed_sq)) dx = dy = __builtin_nan("");
  *reinterpret_cast<offset_xy*>(out + 2 * i) = offset_xy{dx, dy};
}

__global__ void __launch_bounds__(256) pc_pred_from_coarse_kernel(const double* __restrict__ coarse, int32_t* __restrict__ pred, int grid_x,
                                                                  int grid_y, size_t n_patches) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n_patches) return;
  const unsigned patches = (unsigned)(grid_x * grid_y);
  const size_t pair = g / patches;
  const unsigned pt = (unsigned)(g % patches);
  const int i = (int)(pt % (unsigned)grid_x), j = (int)(pt / (unsigned)grid_x);
  const int gx_lr = grid_x / 4, gy_lr = grid_y / 4;
  const int li = i / 4 < gx_lr - 1 ? i / 4 : gx_lr - 1, lj = j / 4 < gy_lr - 1 ? j / 4 : gy_lr - 1;
  const offset_xy s = *reinterpret_cast<const offset_xy*>(coarse + 2 * (pair * (size_t)(gx_lr * gy_lr) + (size_t)(lj * gx_lr + li)));
  int32_t px, py;
  pred_from_coarse(s.x, s.y, &px, &py);
  *reinterpret_cast<offset_ixy*>(pred + 2 * g) = offset_ixy{px, py};
}

// blocks of 256 lanes over n items, at most 2^31 - 1 of them (the entries admit no more patches per call)
inline bool lane_blocks(size_t n, unsigned* blocks) {
  const size_t b = (n + 255) / 256;
  *blocks = (unsigned)b;
  return b <= 0x7fffffffull;
}
}  // namespace

hipError_t launch_pc_offset_gather(const PcOffsetArgs& a, int n_pairs, hipStream_t stream) {
  if (n_pairs == 0) return hipSuccess;
  if (!a.prev || !a.scratch || !a.pred || !a.applied || a.n < 2 || a.n > a.frame_w || a.n > a.frame_h || a.pitch < (size_t)a.frame_w)
    return hipErrorInvalidValue;
  const unsigned long long total = (unsigned long long)n_pairs * (unsigned long long)(a.grid_x * a.grid_y);
  if (total > 0x7fffffffull) return hipErrorInvalidValue;
  // lanes: one per 16-byte chunk of the patch, whole waves, 256 at most
  const long chunks = a.n >= 16 ? (long)a.n * ((a.n + 15) >> 4) : (long)a.n * a.n;
  const unsigned threads = chunks >= 256 ? 256u : (unsigned)((chunks + 63) / 64 * 64);
  const unsigned per_launch = 1u << 22;  // workgroups
  for (unsigned long long q0 = 0; q0 < total; q0 += per_launch) {
    const unsigned nb = total - q0 < per_launch ? (unsigned)(total - q0) : per_launch;
    hipLaunchKernelGGL(pc_offset_gather_kernel, dim3(nb), dim3(threads), 0, stream, a, (unsigned)q0);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

hipError_t launch_pc_offset_clamp(const PcOffsetArgs& a, int n_pairs, hipStream_t stream) {
  const size_t n_patches = (size_t)n_pairs * (size_t)(a.grid_x * a.grid_y);
  if (n_patches == 0) return hipSuccess;
  unsigned blocks;
  if (!a.pred || !a.applied || a.n < 2 || a.n > a.frame_w || a.n > a.frame_h || !lane_blocks(n_patches, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pc_offset_clamp_kernel, dim3(blocks), dim3(256), 0, stream, a, n_patches);
  return hipGetLastError();
}

hipError_t launch_pc_offset_finish(double* out, const int32_t* applied, size_t n_patches, double max_px_speed_sq, hipStream_t stream) {
  if (n_patches == 0) return hipSuccess;
  unsigned blocks;
  if (!out || !applied || !lane_blocks(n_patches, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pc_offset_finish_kernel, dim3(blocks), dim3(256), 0, stream, out, applied, n_patches, max_px_speed_sq);
  return hipGetLastError();
}

hipError_t launch_pc_pred_from_coarse(const double* coarse, int32_t* pred, int grid_x, int grid_y, int n_pairs, hipStream_t stream) {
  const size_t n_patches = (size_t)n_pairs * (size_t)(grid_x * grid_y);
  if (n_patches == 0) return hipSuccess;
  unsigned blocks;
  if (!coarse || !pred || grid_x < 4 || grid_y < 4 || !lane_blocks(n_patches, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pc_pred_from_coarse_kernel, dim3(blocks), dim3(256), 0, stream, coarse, pred, grid_x, grid_y, n_patches);
  return hipGetLastError();
}

}  // namespace mof
