/*
 * ref_fft_peak.cpp -- runs the peak stage of the reference's FFT OpenCL text (its minmaxloc and refine functions, the tail of
 * the phaseCorrelateField kernel) on the CPU. TEST INFRASTRUCTURE ONLY; built into oracle/_ref/ (never committed) and only
 * where the reference checkout exists.
 *
 * Nothing of the text is copied: oracle/Makefile compiles the reference's .cl file with clang in OpenCL mode for x86-64, with
 * the host's compile-time defines, and this driver links that object. The defines fix the patch size, so there is one
 * library per size; REF_N, REF_KERCN, REF_WGS and REF_WGS2_ALIGNED repeat the values the object was compiled with.
 *
 * The launch is the kernel's own: n groups along dimension 1 (one per surface row), WGS work-items along dimension 0, each
 * group with its own pair of __local reduction arrays, and barrier() across the whole launch (cl_host.h) -- group 0 reads
 * what the other groups wrote. The two functions are called back to back as the kernel calls them, with a barrier between.
 */
#include <cstdint>
#include <cstring>
#include <vector>

#define CLH_MANGLED_NAMES
#include "cl_host.h"

#if !defined(REF_N) || !defined(REF_KERCN) || !defined(REF_WGS) || !defined(REF_WGS2_ALIGNED)
#error "REF_N, REF_KERCN, REF_WGS and REF_WGS2_ALIGNED must repeat the defines of the linked object"
#endif
static_assert(REF_KERCN * REF_WGS == REF_N, "one pass of the arg-max covers a row: kercn * WGS == LOCAL_SIZE");
static_assert(REF_WGS2_ALIGNED < REF_WGS && 2 * REF_WGS2_ALIGNED >= REF_WGS, "largest power of two below WGS");

/* the two functions of the linked object (OpenCL C has C linkage for its own functions; address spaces do not reach the ABI) */
extern "C" void minmaxloc(const unsigned char* surface, int step_bytes, int offset_bytes, int patch_cols, int patch_cells,
                          int unused_rows, int unused_cols, int n_groups, unsigned char* record, int patch_index,
                          float* group_max, unsigned* group_loc, int patch_x, int patch_y, int patch_size);
extern "C" void refine(unsigned char* surface, int step_bytes, int offset_bytes, int patch_cols, int patch_rows, int n_groups,
                       unsigned char* record, int patch_index, int patch_x, int patch_y, int patch_size, int window_radius);

namespace {
struct PeakArgs {
  unsigned char* pcr;
  int step, xvec, yvec;
  unsigned char* dst;
  float* lmax;       /* [n][WGS2_ALIGNED] */
  unsigned* lmaxloc; /* [n][WGS2_ALIGNED] */
};

void work_item(void* p) {
  PeakArgs* a = static_cast<PeakArgs*>(p);
  const size_t gid = clh_get_group_id(1);
  minmaxloc(a->pcr, a->step, 0, REF_N, REF_N * REF_N, REF_N, REF_N / 2 + 1, REF_N, a->dst, 0, a->lmax + gid * REF_WGS2_ALIGNED,
            a->lmaxloc + gid * REF_WGS2_ALIGNED, a->xvec, a->yvec, REF_N);
  clh_barrier();
  refine(a->pcr, a->step, 0, REF_N, REF_N, REF_N, a->dst, 0, a->xvec, a->yvec, REF_N, 3);
}
}  // namespace

extern "C" {

/* out[4] = {LOCAL_SIZE, kercn, WGS, WGS2_ALIGNED} of this library */
void ref_fft_peak_params(int* out) {
  out[0] = REF_N; out[1] = REF_KERCN; out[2] = REF_WGS; out[3] = REF_WGS2_ALIGNED;
}

/* pcr: a frame-sized f32 surface image with rows `step` BYTES apart and frame_cols columns, holding at least (yvec + 1) n rows;
 * the patch is the n x n tile at column xvec n, row yvec n. out_xy_f32 receives the two floats the kernel stores for the patch.
 * Returns 0; -1 on arguments that do not fit this library's n or the frame. */
int ref_fft_peak(const float* pcr, int step, int frame_cols, int n, int xvec, int yvec, float* out_xy_f32) {
  if (!pcr || !out_xy_f32 || n != REF_N || xvec < 0 || yvec < 0 || (xvec + 1) * n > frame_cols) return -1;
  if (step < frame_cols * (int)sizeof(float) || step % (int)sizeof(float)) return -1;
  /* the kernel's result record: n maxima, n locations, each block aligned to 8 bytes (its align()) */
  const size_t valstep = ((size_t)n * 4 + 7) & ~(size_t)7, fullstep = (valstep + (size_t)n * 4 + 7) & ~(size_t)7;
  std::vector<unsigned char> dst(fullstep, 0);
  std::vector<float> lmax((size_t)n * REF_WGS2_ALIGNED, 0.0f);
  std::vector<unsigned> lmaxloc((size_t)n * REF_WGS2_ALIGNED, 0u);
  PeakArgs a{reinterpret_cast<unsigned char*>(const_cast<float*>(pcr)), step, xvec, yvec, dst.data(), lmax.data(), lmaxloc.data()};
  const size_t groups[2] = {1, (size_t)n}, local[2] = {REF_WGS, 1}, zero[2] = {0, 0};
  if (clh_launch(work_item, &a, groups, local, zero, groups, 32 * 1024)) return -2;
  std::memcpy(out_xy_f32, dst.data() + sizeof(float), 2 * sizeof(float)); /* slots 1 and 2 of the record (cl:1368-1373) */
  return 0;
}
}
