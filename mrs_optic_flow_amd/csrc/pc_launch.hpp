// pc_launch.hpp -- what the host-side launchers at the bottom of the kernel files share (host code only, not installed): the front-end
// form dispatch and its enumeration, the 65535-pair split of a PcArgs, the CU count of the current device, and the dynamic-LDS limit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <type_traits>

#include "mof_kernels.h"

namespace mof {

// ---- 1. the front-end forms of a kernel: (DS, CH, PK) = (downscale, channels, peak model) as compile-time constants --------------
// A kernel family has the forms of its set: gray and BGR8 always, the long-range mode (quarter-resolution gray patches) and the
// OpenCL peak model where the family's kernels have a DS / PK parameter.
enum PcFormSet {
  PC_FORMS_CH = 0,        // (1, 1, 0) (1, 3, 0)
  PC_FORMS_CH_PK = 1,     // ... x both peak models
  PC_FORMS_DS_CH = 2,     // ... and (4, 1, 0)
  PC_FORMS_ALL = 3,       // {(1, 1), (1, 3), (4, 1)} x both peak models
};
template <int V>
using pc_const = std::integral_constant<int, V>;

// f(ds, ch, pk) with the integral constants of one form of SET; hipErrorInvalidValue for everything else: the long-range mode on BGR8
// frames, channels outside {1, 3}, downscale outside {1, 4}, peak_model outside {0, 1}, and what SET does not hold
template <int SET = PC_FORMS_ALL, class F>
hipError_t pc_dispatch_form(int downscale, int channels, int peak_model, F&& f) {
  constexpr bool LR = (SET & PC_FORMS_DS_CH) != 0, PK1 = (SET & PC_FORMS_CH_PK) != 0;
  const int front = downscale == 1 ? (channels == 1 ? 0 : (channels == 3 ? 1 : -1)) : ((LR && downscale == 4 && channels == 1) ? 2 : -1);
  if (front < 0 || (peak_model != 0 && !(PK1 && peak_model == 1))) return hipErrorInvalidValue;
  switch (2 * front + peak_model) {
    case 0: return f(pc_const<1>{}, pc_const<1>{}, pc_const<0>{});
    case 2: return f(pc_const<1>{}, pc_const<3>{}, pc_const<0>{});
    case 1:
      if constexpr (PK1) return f(pc_const<1>{}, pc_const<1>{}, pc_const<1>{});
      break;
    case 3:
      if constexpr (PK1) return f(pc_const<1>{}, pc_const<3>{}, pc_const<1>{});
      break;
    case 4:
      if constexpr (LR) return f(pc_const<4>{}, pc_const<1>{}, pc_const<0>{});
      break;
    case 5:
      if constexpr (LR && PK1) return f(pc_const<4>{}, pc_const<1>{}, pc_const<1>{});
      break;
    default: break;
  }
  return hipErrorInvalidValue;
}
template <int SET = PC_FORMS_ALL, class F>
hipError_t pc_dispatch_form(const PcArgs& a, F&& f) {
  return pc_dispatch_form<SET>(a.downscale, a.channels, a.peak_model, static_cast<F&&>(f));
}

// f on EVERY form pc_dispatch_form<SET> can return, through pc_dispatch_form itself (what a configure function sets its kernels'
// attribute with: the list cannot differ from the launch's); the first error ends the walk
template <int SET = PC_FORMS_ALL, class F>
hipError_t pc_each_form(F&& f) {
  for (int pk = 0; pk <= ((SET & PC_FORMS_CH_PK) ? 1 : 0); ++pk)
    for (int front = 0; front < ((SET & PC_FORMS_DS_CH) ? 3 : 2); ++front) {
      const hipError_t e = pc_dispatch_form<SET>(front == 2 ? 4 : 1, front == 1 ? 3 : 1, pk, f);
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

// ---- 2. a grid dimension holds 65535: the pair (or image) index of a long batch goes out in several launches ---------------------
constexpr int PC_MAX_GRID_PAIRS = 65535;
constexpr int PC_MAX_GRID_IMAGES = 65534;  // images of pairs: an even count keeps cur / prev together

// launch(slice, nk) for every slice of at most 65535 pairs of a.cur / a.prev / a.out / a.quality / a.prev_off, slice.total = its patches; ends at
// the first error. max_pairs: a smaller slice, where a launcher has another bound as well (K1 at 64: its record buffer)
template <class F>
hipError_t pc_split_pairs(const PcArgs& a, int n_pairs, F&& launch, int max_pairs = PC_MAX_GRID_PAIRS) {
  const int patches = a.grid_x * a.grid_y;
  for (int k0 = 0; k0 < n_pairs; k0 += max_pairs) {
    const int nk = n_pairs - k0 < max_pairs ? n_pairs - k0 : max_pairs;
    PcArgs c = a;
    c.cur = a.cur + (size_t)k0 * a.cur_stride;
    c.prev = a.prev + (size_t)k0 * a.prev_stride;
    c.out = a.out + (size_t)k0 * patches * 2;
    if (a.quality) c.quality = a.quality + (size_t)k0 * patches * 2;
    if (a.prev_off) c.prev_off = a.prev_off + (size_t)k0 * patches * 2;
    c.total = nk * patches;
    const hipError_t e = launch(c, nk);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---- 3. compute units of a device (default: the calling thread's current one). Asked per call -- an attribute query, no
// synchronisation --, because the devices of a shard group need not be alike; 256 where the query fails
inline int pc_cu_count(int device = -1) {
  int cus = 0;
  if ((device < 0 && hipGetDevice(&device) != hipSuccess) ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
    cus = 256;
  return cus;
}

// ---- 4. dynamic LDS ---------------------------------------------------------------------------------------------------------------
// Diagnostic knob (occupancy and co-scheduling experiments only): MOF_PC_EXTRA_LDS=<bytes> pads the dynamic LDS request of K1, the
// sequence kernels and the half-tile sequence / pair kernels, i.e. caps their workgroups per CU. Read once per process.
inline size_t pc_extra_lds() {
  static const size_t v = [] {
    const char* e = getenv("MOF_PC_EXTRA_LDS");
    return e ? (size_t)atol(e) : (size_t)0;
  }();
  return v;
}

constexpr size_t PC_DEFAULT_LDS_LIMIT = 48 * 1024;  // what a kernel may ask for without the attribute
template <class K>
hipError_t pc_raise_lds(K* kernel, size_t bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
// ... for the launchers that set it at every launch: only where the request is beyond the default limit
template <class K>
hipError_t pc_raise_lds_beyond_default(K* kernel, size_t bytes) {
  return bytes > PC_DEFAULT_LDS_LIMIT ? pc_raise_lds(kernel, bytes) : hipSuccess;
}

}  // namespace mof
