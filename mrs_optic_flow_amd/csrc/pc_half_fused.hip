// pc_half_fused.hip -- K1h's fused window-offset forms (include/mof.h, "Predicted-shift window offsets": MOF_PRED_ROUTE_FUSED): the
// pair kernel of pc_half_kernel.hip with OFF on, gray and BGR8, at every pair size of MOF_HALF_SIZES. A translation unit of its own:
// the half-tile kernel's file is the longest of the build, and these 2 x 14 instantiations beside its own would lengthen the build's
// critical path; here they compile next to it. The kernel and the size dispatch are that file's, compiled in without its host side.

#define MOF_HALF_KERNEL_ONLY 1
#include "pc_half_kernel.hip"

namespace mof {

// the dynamic-LDS limit of the fused forms of padded size m, by the enumeration the launch below dispatches them by
hipError_t pc_configure_half_fused(int m) {
  return dispatch_half_pair_size(m, [](auto ms) {
    return pc_each_form<PC_FORMS_CH>([&](auto, auto ch, auto) { return pc_raise_lds(&pc_half_kernel<ch, ms, false, true>, HalfPlanOf<ms>::HP.lds_bytes); });
  });
}

// launch_pc_half with a.prev_off set (it checks the front end and the sizes): one workgroup per patch, the pair index on gridDim.z
hipError_t launch_pc_half_fused(const PcArgs& a_in, int m, int n, int n_pairs, hipStream_t stream) {
  if (!a_in.prev_off || a_in.downscale != 1 || a_in.peak_model != 0 || n > m || n < 2) return hipErrorInvalidValue;
  return pc_split_pairs(a_in, n_pairs, [&](const PcArgs& c, int nk) {
    const dim3 g((unsigned)c.grid_x, (unsigned)c.grid_y, (unsigned)nk);
    return dispatch_half_pair_size(m, [&](auto ms) {
      return pc_dispatch_form<PC_FORMS_CH>(c, [&](auto, auto ch, auto) {
        hipLaunchKernelGGL((pc_half_kernel<ch, ms, false, true>), g, dim3((unsigned)HalfPlanOf<ms>::T), (size_t)HalfPlanOf<ms>::HP.lds_bytes, stream, c, n, nk, 1);
        return hipGetLastError();
      });
    });
  });
}

}  // namespace mof
