// pc_gate_kernel.hip -- the FFT engine's opt-in response gate (include/mof.h, mof_fft_set_min_response): one small streaming kernel behind
// the field's kernels, so that the tuned peak tails keep their registers (profiles/fft_min_response_static.txt: fused into peak_finish the
// threshold costs 2 .. 6 SGPRs on most instantiations and new spills on the half-tile video forms).
//
// One lane per patch: it loads the stored response quality[2 i] -- the very double a host that reads `quality` back sees -- and, where
// !(response >= min_response) (a NaN response included), stores (NaN, NaN) over the patch's shift, the NaN of peak_finish (pc_common.hpp).
// It writes nothing otherwise: a patch that passes keeps its bits, one that the validity rule already made NaN stays NaN either way.
// No LDS, 16 bytes read and at most 16 written per lane; 256 lanes per workgroup, the last one ragged.
// Included by mof_capi.hip, its only caller (csrc/Makefile): not a translation unit of its own.

#include <hip/hip_runtime.h>

#include "mof_kernels.h"

namespace mof {
namespace {
// (the caller's shift buffer is only known to be aligned as doubles are)
typedef double gate_xy __attribute__((ext_vector_type(2), aligned(8)));

__global__ void __launch_bounds__(256) pc_response_gate_kernel(double* __restrict__ out, const double* __restrict__ quality, size_t n_patches,
                                                               double min_response) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_patches) return;
  const double response = quality[2 * i];
  if (!(response >= min_response)) {
    const double nan = __builtin_nan("");
    *reinterpret_cast<gate_xy*>(out + 2 * i) = gate_xy{nan, nan};
  }
}
}  // namespace

hipError_t launch_pc_response_gate(double* out, const double* quality, size_t n_patches, double min_response, hipStream_t stream) {
  if (n_patches == 0) return hipSuccess;
  if (!out || !quality) return hipErrorInvalidValue;
  const size_t blocks = (n_patches + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;  // (the entries admit at most 2^31 - 1 patches per call)
  hipLaunchKernelGGL(pc_response_gate_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, out, quality, n_patches, min_response);
  return hipGetLastError();
}

}  // namespace mof
