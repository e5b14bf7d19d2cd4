// mof_kernels.h -- internal launch interface between the C ABI (mof_capi.hip) and the
// gfx950 kernels (pc_kernel.hip, bm_kernel.hip). Not installed; the public surface is include/mof.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace mof {

// ---- K1: per-patch FFT phase correlation ----------------------------------------------------
struct PcArgs {
  const uint8_t* cur;     // device, pair k at cur + k*cur_stride
  const uint8_t* prev;
  size_t cur_stride;      // bytes between consecutive pairs' frames
  size_t prev_stride;
  size_t pitch;           // bytes per frame row
  int grid_x, grid_y;     // patches per frame
  int origin_x, origin_y;
  int stride_x, stride_y;
  int total;              // n_pairs * grid_x * grid_y (set by the launcher)
  int stagger_div, stagger_units;  // start-up stagger of co-resident workgroups (set by the launcher)
  int channels;           // 1 = gray frames; 3 = interleaved BGR8, CV_RGB2GRAY fused into the load
  int downscale;          // 1, or 4 = long-range mode (quarter-resolution patches formed on the fly)
  int peak_model;         // 0 = cv::phaseCorrelate (useOCL=false), 1 = the OpenCL kernel's model (useOCL=true)
  int search_radius;      // peak_model 1: SEARCH_RADIUS (FftMethod.cpp:820)
  double max_px_speed_sq; // FftMethod.cpp:1686
  const float* twiddles;  // device, N (cos, -sin) pairs, computed in double on the host
  double* out;            // device, [pair][patch] (x, y)
  double* quality;        // device, nullable: [pair][patch] (response, peak) of the correlation surface (pc_common.hpp, quality_store)
  const int32_t* prev_off;  // device, nullable: [pair][patch][2] APPLIED predictions (a_x, a_y) of the launch's first pair -- the fused
                            // window-offset forms read the previous patch at (x0 - a_x, y0 - a_y) (pc_offset_clamp_kernel wrote them: the
                            // clamp keeps the window inside the frame). Last member: every older kernel's argument offsets stay put.
};

// K1 at 64 ends a patch with a 128-byte record; pc_finish_kernel, one lane per patch, turns a piece's records into shifts and quality.
//   dwords 0 .. 24: the 5 x 5 window, lane l's centroid_window_value (0 outside the clamped window)
//   25: the first maximum's value   26: its shifted index   27: 1 = one of the two patches is constant   28: C_dc (0 unless 27 is set)
constexpr int PC_FINISH_DWORDS = 32;
// the ONE spelling of which K1 forms end a patch with a record: the kernel's argument type, its tail and the engine's buffer follow it
constexpr bool pc_field_records(int patch_size, int peak_model) { return patch_size == 64 && peak_model == 0; }
// records the engine of a K1 route must own for launch_pc_field (0: that route writes none): one launch piece of whole frame pairs --
// 65536 patches (8 MiB), or one frame pair's where a frame holds more. A fixed size, made with the engine: nothing grows at a call, so a
// fresh engine's first batch can still be captured into a graph.
int pc_finish_records(int patch_size, int peak_model, int patches);

// twiddles W_n^k = exp(-2 pi i k / n), k < n, as (re, im) float pairs (mof_capi.hip; both engines' d_twiddles)
std::vector<float> twiddle_table(int n);

// Run-time plan of the general K1 (pc_kernel_generic.hip): any samplePointSize n whose padded transform size
// m = cv::getOptimalDFTSize(n) gives an m x m complex tile that fits one CU's LDS (m <= 135)
struct PcPlan {
  int n, m;          // patch size; padded transform size (smallest 2^a 3^b 5^c >= n)
  int pitch;         // complex elements per tile row
  int skew_mask;     // ~0: tile column c sits at c + (c >> 3); 0: no skew
  int threads;       // workgroup size (multiple of 64)
  int n_stages;      // Stockham stages of a 1-D transform
  int radix[8];      // their radices, each of {2, 3, 4, 5, 8}, product m
  uint32_t radix_packed;  // the same, four bits per stage (what the kernel reads)
  int hermitian;     // 1: m even, the inverse runs on the half spectrum; 0: m odd, full complex inverse
  int lds_bytes;     // dynamic LDS of a workgroup
};
int pc_optimal_dft_size(int n);                          // cv::getOptimalDFTSize
int pc_radix_chain(int m, int* radix, int max_stages);   // number of stages, -1 if m is not 5-smooth
bool pc_build_plan(int n, PcPlan* out);                  // false: n needs the large-patch pipeline (or is < 2)
hipError_t pc_configure_generic();
// use_static (FftRoute::planned_static): the compile-time plan of the transform size where there is one; false: the run-time plan
hipError_t launch_pc_generic(const PcArgs& a, const PcPlan& plan, bool use_static, int n_pairs, hipStream_t stream);

// ---- images too large for a CU (padded side m > 135): the planned pipeline through HBM scratch (pc_large_kernel.hip) ----
bool pc_build_line_plan(int n, PcPlan* out);  // n, m, radix chain only (no LDS tile); false for n < 2 or m > 960
// where image f of a launch comes from
struct PclSrc {
  const uint8_t* base[2];  // paired: [0] = cur frames, [1] = prev frames; else base[0] alone
  size_t stride[2];        // bytes between consecutive frame pairs (paired) / images (not paired)
  size_t pitch;            // bytes per frame row
  int paired;              // 1: image f = 2 (pair * patches + patch) + which (0 cur, 1 prev); 0: image f = base[0] + f * stride[0];
                           // 2 (r06, a VIDEO): image f = frame * patches + patch of base[0] + frame * stride[0] -- every frame transformed once
  int grid_x, grid_y, origin_x, origin_y, stride_x, stride_y;  // patch grid inside a frame (paired)
  int sums_stride;         // ints between the exact-sum quadruples of consecutive images (sr_rows_real_src_kernel; 0 = 4: a dense array)
};
struct PclFinal {
  const float* Dt;         // [pairs][m/2 + 1][m] complex
  const float2* cand;      // [pairs][n_cand]
  int n_cand;              // set by the launcher
  const float* twiddles;   // m (cos, -sin) pairs
  int m, n;                // set by the launcher from the plan
  int mode;                // 0: scaleRotationEstimator (out[pair][4] = scale, rot, pt.x, pt.y); 1: FftMethod (out[pair][2] = shift or NaN)
  double M_log;            // mode 0: log-polar magnitude
  double max_px_speed_sq;  // mode 1
  double* out;
  const int* flags;        // mode 1, nullable: [2 pairs] constant-patch flags written by pcl_rows (bit 0: not constant, bit 1: pixel 0 != 0)
  const float* cdc;        // mode 1, with flags: [pairs] DC bin of the cross-power spectrum
  int peak_model;          // mode 1: 0 = cv::phaseCorrelate, 1 = the OpenCL kernel's model (m == n; L7 + L8 of the planned pipeline only)
  int search_radius;       // peak_model 1
  double* quality;         // nullable: [pairs] (response, peak), as PcArgs::quality (mode 0: as SrPcArgs::quality)
  double min_response;     // mode 0: the estimator's response gate, as SrPcArgs::min_response
};
size_t pcl_zh_floats(const PcPlan& pl);  // floats of one image's row half-spectra Zh: (m/2 + 1) * m complex
int pcl_candidates(const PcPlan& pl);    // peak candidates per pair
// L5: images -> Zh (image f at zh + f * zh_stride floats); flags (nullable, ZEROED by the caller): 1 int per image
hipError_t launch_pcl_rows(const PclSrc& src, const PcPlan& pl, const float* twiddles, float* zh, size_t zh_stride, int* flags,
                           int n_images, int channels, int downscale, hipStream_t stream);
// L6: pair p = (cur: zh_cur + p * zh_stride, prev: zh_prev + p * zh_stride) -> Dt[p]; cdc nullable; peak_model as PclFinal
hipError_t launch_pcl_cols(const float* zh_prev, const float* zh_cur, size_t zh_stride, const PcPlan& pl, const float* twiddles,
                           float* Dt, float* cdc, const int* flags, int n_pairs, hipStream_t stream, int peak_model = 0);
// L7 + L8 (a.Dt, a.cand, a.twiddles, a.mode, a.out, a.quality [, a.M_log, a.min_response | a.max_px_speed_sq, a.flags, a.cdc, a.peak_model, a.search_radius])
hipError_t launch_pcl_peak(const PclFinal& a, const PcPlan& pl, int n_pairs, hipStream_t stream, bool candidates_done = false);
// C_dc of every pair from its row spectra (for pipelines whose column kernel does not hand it out)
hipError_t launch_pcl_cdc(const float* zh_prev, const float* zh_cur, size_t zh_stride, int m, float* cdc, int n_pairs, hipStream_t stream);

// ---- the fused kernel on a HALF-size tile (pc_half_kernel.hip): even padded sizes m in (135, 192] -- and 64 / 96 / 120 / 128 for A/B --,
// cv::phaseCorrelate's model on full-resolution gray or BGR8 frames. m = padded transform size (a.twiddles: m entries), n = patch size
bool pc_half_supported(int m);
int pc_half_workgroups_per_cu(int m);
hipError_t pc_configure_half(int m);
hipError_t launch_pc_half(const PcArgs& a, int m, int n, int n_pairs, hipStream_t stream);
// ... with a.prev_off set (pc_half_fused.hip, a translation unit of its own): the fused window-offset form of every pair size
hipError_t pc_configure_half_fused(int m);
hipError_t launch_pc_half_fused(const PcArgs& a, int m, int n, int n_pairs, hipStream_t stream);
// ... on a video (r05): runs of `run` consecutive pairs per workgroup, a frame's spectrum kept in registers for the next pair; a.cur = the
// launch's first frame, frame f at a.cur + f * a.cur_stride (as launch_pc_sequence)
bool pc_half_sequence_supported(int m);
hipError_t launch_pc_half_sequence(const PcArgs& a, int m, int n, int n_pairs, int run, hipStream_t stream);

bool pc_patch_size_supported(int n);  // the hand-tuned instantiations: 32, 64, 120, 128
hipError_t pc_configure(int patch_size);  // once per device before the first launch
// PcArgs::pitch must stay below PC_MAX_PITCH (16 MiB per frame row): the one-patch forms of K1 address a lane's pixels as a scalar patch
// base plus ONE 32-bit lane offset, row-in-patch * pitch + column bytes, formed with a 24-bit multiply (pc_kernel.hip, fetch16). Every
// field launch of the FFT engine is held to it (mof_capi.hip, launch_field: MOF_ERR_BAD_ARG); launch_pc_field itself answers
// hipErrorInvalidValue beyond it.
constexpr size_t PC_MAX_PITCH = (size_t)1 << 24;
// finish, finish_records: the engine's record buffer (device, PC_FINISH_DWORDS dwords per record) where pc_finish_records says the route
// needs one -- a kernel argument of its own beside PcArgs, whose size every other kernel's code depends on
hipError_t launch_pc_field(const PcArgs& a, int patch_size, int n_pairs, hipStream_t stream, uint32_t* finish = nullptr, int finish_records = 0);
// launch_pc_field's a.twiddles at 32 and 64: twiddle_table(n) with the packed per-index rows appended (TwRows, pc_passes.hpp); other
// sizes are left as they are. The classic table stays at offset 0 for every kernel that reads it.
void pc_append_twiddle_rows(std::vector<float>& table, int n);
// Frame sequences (pc_seq_kernel.hip; 64 x 64 patches): a.cur = frame 0, a.cur_stride = bytes between frames, pair k =
// (frame k + 1, frame k) for k < n_pairs; one workgroup per patch position walks `run` consecutive pairs
bool pc_sequence_supported(int patch_size);
hipError_t pc_configure_sequence();
hipError_t launch_pc_sequence(const PcArgs& a, int n_pairs, int run, hipStream_t stream);
// The same on a half-size tile (pc_seq_half.hip): 128 x 128 patches, two workgroups per CU
bool pc_sequence_half_supported(int patch_size);
hipError_t pc_configure_sequence_half(int patch_size);
hipError_t launch_pc_sequence_half(const PcArgs& a, int patch_size, int n_pairs, int run, hipStream_t stream);
// N = 120 (15 x 8) lives in pc_kernel_mixed.hip
hipError_t pc_configure_120();
hipError_t launch_pc_field_120(const PcArgs& a, int n_pairs, hipStream_t stream);
// The response gate behind any of the above (pc_gate_kernel.hip): patch i < n_patches with !(quality[2 i] >= min_response) gets (NaN, NaN)
// at out[2 i], every other patch is left as it is
hipError_t launch_pc_response_gate(double* out, const double* quality, size_t n_patches, double min_response, hipStream_t stream);

// ---- predicted-shift window offsets (pc_offset_kernel.hip; include/mof.h, "Predicted-shift window offsets") ----
// The two definitions, shared by the kernels and the pure host helpers (mof_fft_pred_clamp, mof_fft_pred_from_coarse).
// Applied prediction on one axis: p clamped into [x0 - (w - n), x0], so that the previous window [x0 - a, x0 - a + n) stays inside
// [0, w). 0 <= x0 <= w - n, so neither bound overflows and p is only compared.
__host__ __device__ inline int32_t pred_clamp_axis(int32_t p, int x0, int w, int n) {
  const int32_t lo = x0 - (w - n), hi = x0;
  return p < lo ? lo : (p > hi ? hi : p);
}
// Prediction from a long-range shift (quarter-pixels): rint(4 s) in fp64, half to even; a NaN shift predicts (0, 0)
__host__ __device__ inline int32_t pred_round4(double s) {
  double v = __builtin_rint(4.0 * s);
  v = v < -2147483648.0 ? -2147483648.0 : (v > 2147483647.0 ? 2147483647.0 : v);
  return (int32_t)v;
}
__host__ __device__ inline void pred_from_coarse(double sx, double sy, int32_t* px, int32_t* py) {
  const bool nan = sx != sx || sy != sy;
  *px = nan ? 0 : pred_round4(sx);
  *py = nan ? 0 : pred_round4(sy);
}
struct PcOffsetArgs {
  const uint8_t* prev;   // device, pair k at prev + k * prev_stride
  size_t prev_stride;
  uint8_t* scratch;      // device, pair k at scratch + k * frame_h * pitch: the window of patch (x0, y0) lands AT (x0, y0)
  size_t pitch;          // of both
  int frame_w, frame_h, n;
  int grid_x, grid_y, origin_x, origin_y, stride_x, stride_y;
  const int32_t* pred;   // device, [pair][patch][2]
  int32_t* applied;      // device, [pair][patch][2]: written
};
// The clamp alone (the fused route): applied[q] = clamp(pred[q]) for every patch of n_pairs pairs; a.prev / a.scratch are not read
hipError_t launch_pc_offset_clamp(const PcOffsetArgs& a, int n_pairs, hipStream_t stream);
// Window gather: the n x n bytes of prev at (x0 - a_x, y0 - a_y) into scratch at (x0, y0), a = the clamped pred, for every patch of n_pairs pairs
hipError_t launch_pc_offset_gather(const PcOffsetArgs& a, int n_pairs, hipStream_t stream);
// Finish, behind the field's kernels and the response gate: out[i] = applied[i] + out[i] per component (a zero component keeps the residual's
// bits), (NaN, NaN) where the residual is NaN or |total|^2 > max_px_speed_sq; a patch with applied = (0, 0) is left as it is
hipError_t launch_pc_offset_finish(double* out, const int32_t* applied, size_t n_patches, double max_px_speed_sq, hipStream_t stream);
// Prediction of fine patch (i, j) from the long-range patch (min(i / 4, gx_lr - 1), min(j / 4, gy_lr - 1)) of its pair
hipError_t launch_pc_pred_from_coarse(const double* coarse, int32_t* pred, int grid_x, int grid_y, int n_pairs, hipStream_t stream);

// ---- K2/K3: SAD block scan + histogram mode -------------------------------------------------
struct BmArgs {
  const uint8_t* cur;
  const uint8_t* prev;
  size_t cur_stride, prev_stride, pitch;
  int grid_x, grid_y;
  int block, step, radius;
  int low_contrast_rule;
  int channels;  // 1: gray frames; 3: interleaved BGR8, CV_RGB2GRAY fused into the staging loads
  int8_t* dx;    // [pair][by*grid_x+bx]
  int8_t* dy;
  int8_t* mode;  // [pair][8]
};

// What the scans' Q forms get beside BmArgs: the per-block quality output {min_sad, zero_sad, max_sad} (may be null) and the match
// gate -- a block is valid iff min_sad <= max_min_sad and max_sad - min_sad >= min_sad_range; an invalid one reports BM_INVALID twice
struct BmQArgs {
  uint32_t* quality = nullptr;  // [pair][by*grid_x+bx][3]
  uint32_t max_min_sad = 0xffffffffu, min_sad_range = 0u;
};
constexpr int BM_INVALID = -128;  // MOF_BM_INVALID: outside every scan range (radius <= 48)
inline bool bm_gate_armed(const BmQArgs& q) { return q.max_min_sad != 0xffffffffu || q.min_sad_range != 0u; }

// The MOF_BM_* knobs of the scans (README), read once per process (bm_kernel.hip: bm_knobs). A default-constructed value: nothing set
struct BmKnobs {
  bool generic = false;   // MOF_BM_GENERIC set, whatever the value: 16 x 16 blocks on the generic scan too
  int xb = 0, bpw = 0;    // MOF_BM_XB / MOF_BM_BPW != 0: the plan search held to that many blocks per lane / per workgroup
  int g = 0;              // MOF_BM_G != 0: the row chunk, over the one chosen from the block size
  bool verbose = false;   // MOF_BM_VERBOSE set: the plan line on stderr at every launch of the generic scan
};
// Everything a launch of the scan needs beside its arguments, decided once at create (bm_route)
struct BmRoute {
  bool scan16 = false;    // the 16 x 16 scan (block 16, step % 4 == 0, even radius <= 16, strip within 64 KB); else the generic scan
  // scan16: blocks per wave, waves per block row, dwords per strip row, dynamic LDS of the plain form (the Q form: one more reduce array)
  int bpw = 0, waves_per_row = 0, strip_dwords = 0;
  size_t lds = 0;
  // the generic scan: blocks per lane, row chunk (instantiated: 6, 7, 10, anything else as 8), and the launch shape without / with quality
  int xb = 0, g = 8;
  struct Form {
    int bpw = 0, wpd = 0, slot_dwords = 0, threads = 0;
    size_t lds = 0;
    double cost = 1e30;   // modelled issue cycles per useful v_qsad (16 = the instruction's own rate)
  } plain, q;
  bool verbose = false;   // BmKnobs::verbose as the launches read it
};
// Pure host code (no HIP call, no environment, no static state): the route of a geometry; grid_x = 0: any width (one block per workgroup,
// never scan16). False: no block's window fits the LDS.
bool bm_route(int block, int step, int radius, int grid_x, const BmKnobs& k, BmRoute* r);
const BmKnobs& bm_knobs();

// the two below: projections of bm_route under bm_knobs()
bool bm_config_supported(int block, int radius);
bool bm_scan_plan(int block, int step, int radius, int grid_x, bool quality, int out[4]);
// the Q form iff q holds a quality pointer or an armed gate; r: bm_route of a's geometry
hipError_t launch_bm_scan(const BmArgs& a, const BmQArgs& q, const BmRoute& r, int n_pairs, hipStream_t stream);
hipError_t launch_bm_mode(const BmArgs& a, const BmQArgs& q, int32_t* n_invalid, int n_pairs, hipStream_t stream);
// BlockMethod::Refine building blocks (K9 2x resize, K10 nine cut-out SADs)
hipError_t launch_bm_resize2x(const uint8_t* src, size_t pitch, int w, int h, uint8_t* dst, hipStream_t stream);
hipError_t launch_bm_refine_sad(const uint8_t* A, const uint8_t* B, int W2, int spx, int spy, int cw, int ch,
                                unsigned long long* out9, hipStream_t stream);

// ---- K4..K8: scale / rotation estimator (log-polar remap + whole-frame phase correlation) ----
struct SrMapEntry {
  int16_t ax, ay;   // anchor pixel (map coordinate >> 5), saturated to int16
  uint16_t widx;    // (fy & 31) * 32 + (fx & 31): row of the 2-D weight table
  uint16_t valid;   // anchor inside the source (BORDER_TRANSPARENT otherwise)
};

// Bounding box (source pixels) of the K x K footprints of the valid pixels of one 8 x 8 destination tile, taps that
// leave the image reflected back in (BORDER_REFLECT_101); w = h = 0 when the tile has no valid pixel.
struct SrTileBox {
  int16_t x0, y0, w, h;
};

struct SrLpArgs {
  const uint8_t* src;   // image i at src + i*src_stride, `pitch` bytes per row, res x res pixels
  size_t src_stride, pitch;
  uint8_t* dst;         // image i at dst + i*dst_stride, tightly packed res*res
  size_t dst_stride;
  const SrMapEntry* map;   // res*res
  const int16_t* weights;  // [1024][K*K]
  const uint32_t* wplanes; // [1024][K*K/2 + 2]: signed-byte planes of the same weights (sr_weight_planes), staged kernel
  const SrTileBox* sboxes; // [res/16 * res/16]: boxes of the 16 x 16 super-tiles (four 8 x 8 tiles of one workgroup), or null
  int sbox_dwords_max;     // dwords of the largest super-tile box as the kernel lays it out
  int res;
  int zero_invalid;        // 1: pixels mapped outside the source are written as 0 (destination known to start as zeros)
  const SrTileBox* boxes;  // [tiles*tiles] for THIS interpolation's footprint size
  int lds_per_wave;        // bytes of LDS one wave needs for the largest box (multiple of 16)
  int box_dwords_max;      // dwords of the largest box
};

// Residue, kept on purpose: lp_cur, lp_prev and Zt were read by the retired packed pair kernels K5 / K6 only
// (docs/history/retired_switches.md) and are always zero now. K7 and K8 take this struct by value: without the fields K7's kernel
// arguments move and it comes out with another SGPR count and other code; with them it is the instantiation measured so far
// (profiles/runtime_forms_retirement.txt). min_response and quality, read by K8 alone, sit in the eight-byte slots of two more such
// fields (lp_stride, degen), so K7's arguments keep their size and offsets (profiles/sr_quality_static.txt).
struct SrPcArgs {
  const uint8_t* lp_cur;   // (residue)
  const uint8_t* lp_prev;  // (residue)
  double min_response;     // 0: no response gate; > 0: !(response >= min_response) -> (1, 0) (pc_common.hpp, sr_finish)
  const float* twiddles;   // res (cos, -sin) pairs
  float* Zt;               // (residue)
  float* Dt;               // scratch [pairs][res/2+1 u][res y] complex: half spectrum after the column passes
  float2* cand;            // scratch [pairs][n_cand] (value, shifted index)
  int n_cand;
  double M;                // log-polar magnitude
  double* out;             // [pairs][4] = scale, rot, pt.x, pt.y
  double* quality;         // nullable: [pairs][2] = response, peak of the surface pt was read from (pc_common.hpp, quality_store)
};

// host-side tables of cv::logPolar / cv::remap (mof_sr.hip); exposed so that the CPU suite can compare them with the oracle
std::vector<SrMapEntry> sr_logpolar_map(int res, double M, int variant);
std::vector<int16_t> sr_weight_table(int ksize /* 4 cubic, 8 Lanczos4 */);  // [32*32][ksize*ksize], each summing to 2^15
// The same weights as two planes of signed bytes, w = 256 hi + lo, four taps per dword, for v_dot4c_i32_i8 against
// (pixel - 128): per table row K*K/4 dwords hi, K*K/4 dwords lo, then 128 * sum(w) and the index of the one tap whose
// hi would be 128 (kept at 127; -1 if none): sum w p = 256 sum hi p' + sum lo p' + 128 sum w [+ 256 p'(tap)].
std::vector<uint32_t> sr_weight_planes(const std::vector<int16_t>& weights, int ksize);
// per-tile footprint boxes for a ksize x ksize kernel; *lds_per_wave receives the LDS bytes of the largest one
// tile = 8 (per-wave boxes) or 16 (super-tile boxes shared by a workgroup)
std::vector<SrTileBox> sr_tile_boxes(const std::vector<SrMapEntry>& map, int res, int ksize, int* lds_per_wave, int tile_px);

bool sr_always_tuned(int res);             // 240, 256, 480: on the tuned transforms whatever MOF_SR_TUNED_ALL says
bool sr_transform_size_tuned(int m, bool* exact_nyquist);  // the tuned transforms K5s / K6s / K7 exist for transform size m (sr_common.hpp: MOF_SR_TUNED_SIZES)

// The MOF_FFT_* knobs of the FFT engine and MOF_PLANNED_STATIC (README), read once per process (mof_capi.hip: fft_knobs)
struct FftKnobs {
  int half = -1;               // MOF_FFT_HALF: -1 unset
  bool force_planned = false;  // MOF_FFT_FORCE_PLANNED, MOF_FFT_FORCE_LARGE, MOF_FFT_SEQ_PAIRS, MOF_FFT_SEQ_HALF128: set, whatever the value
  bool force_large = false;
  bool seq_pairs = false;
  bool seq_half128 = false;
  bool half_seq_off = false;   // MOF_FFT_HALF_SEQ=0
  bool large_tuned = true;     // MOF_FFT_LARGE_TUNED=0, MOF_FFT_LARGE_VIDEO=0 clear them
  bool large_video = true;
  int seq_run = 0;             // MOF_FFT_SEQ_RUN >= 1: pairs a workgroup of a video kernel walks in time; 0: the launchers pick
  int large_pass = 0;          // MOF_FFT_LARGE_PASS > 0: frame pairs per pass of the large-patch scratch; 0: from the scratch's size
  bool planned_static = true;  // MOF_PLANNED_STATIC=0: the planned kernel on its run-time plan also where a compile-time one exists
};
// Which kernels an FFT engine launches, decided once at create (fft_route)
struct FftRoute {
  enum Family { TUNED, PLANNED, LARGE };
  enum Video { PAIRS, SEQ, SEQ_HALF, HALF_SEQ };
  Family family = TUNED;    // what every launch can run: the hand-tuned K1 of the patch size, the planned LDS kernel
                            // (pc_kernel_generic.hip), or -- padded patch too large for a CU -- the planned pipeline through HBM (pc_large_kernel.hip)
  int m = 0;                // transform size: the patch size (TUNED) or the size cv::phaseCorrelate pads it to
  int half_m = 0;           // > 0: full-resolution pair launches run the fused half-tile kernel of this size instead (pc_half_kernel.hip;
                            //      cv::phaseCorrelate model only)
  Video video = PAIRS;      // a video: the pair form on consecutive frames, K1s (pc_seq_kernel.hip), pc_seq_half.hip, or the half-tile
  int video_m = 0;          // kernel's sequence form at transform size video_m
  bool large_tuned = false; // LARGE, full resolution: the estimator's tuned K5s / K6s / K7 instead of L5 / L6 / L7
  bool odd_tail = false;    // ... on a size whose Nyquist bins are not exact (the rows kernel's exact sums stand in)
  bool large_video = false; // ... and a video transforms every frame once per pass
  const char* variant = ""; // mof_fft_kernel_variant: "stockham", "planned", "planned-large", or "planned-half" wherever half_m > 0
  int min_run = 0;          // the least run length the video form's launcher picks on its own (HALF_SEQ 4, SEQ 2, SEQ_HALF 16; PAIRS 0):
                            // with the 65535 runs of a launch, the pairs a launch can take
  int seq_run = 0;          // FftKnobs::seq_run, large_pass, planned_static as the launches read them
  int large_pass = 0;
  bool planned_static = true;
};
// Pure host code (no HIP call, no environment): the route of a patch size >= 2 under a peak model; *plan receives the plan of the planned
// families. False: the patch pads beyond the planned transforms (> 960).
bool fft_route(int patch_size, int peak_model, const FftKnobs& k, PcPlan* plan, FftRoute* r);
// Pure: the pair kernel of route r has a fused window-offset form (a.prev_off read inside the field kernel) -- K1h at every pair size,
// K1 at 32 / 64 / 128; not the 15 x 8 kernel at 120, the planned LDS kernel or the large-patch pipeline, and cv::phaseCorrelate's
// peak model only
inline bool fft_pred_fused_supported(const FftRoute& r, int peak_model) {
  return peak_model == 0 && (r.half_m > 0 || (r.family == FftRoute::TUNED && r.m != 120));
}
const FftKnobs& fft_knobs();

// The MOF_SR_* knobs of the estimator's engine (README), read once per process (mof_sr.hip: sr_knobs)
struct SrKnobs {
  bool tuned_all = true;  // MOF_SR_TUNED_ALL=0: tuned transforms at 240 / 256 / 480 only, every other resolution on the planned pipeline
  bool verbose = false;   // MOF_SR_VERBOSE
  int seq_run = 0;        // MOF_SR_SEQ_RUN in 1 .. 4096: the fixed run of K6s; 0: chosen per pass
  int chunk = 0;          // MOF_SR_CHUNK: pairs per pass over mof_sr_config.batch_chunk (a value outside 1 .. 4096: the default); 0: unset
  int overlap = -1;       // MOF_SR_OVERLAP: 0 / 1 over mof_sr_config.pipeline_lanes; -1: unset
  // the log-polar remap (K4), A/B runs and the tests of each form
  bool lp_global = false; // MOF_SR_LP_GLOBAL != 0: the per-pixel kernel (weights fetched from L2) for every batch
  bool lp_staged = true;  // MOF_SR_LP_STAGED=0: no LDS-staged source boxes, the table-in-LDS kernel instead
  bool lp_super = true;   // MOF_SR_LP_SUPER=0: staged per wave also where a 16 x 16 super-tile's box would fit
  bool lp_xcd = true;     // MOF_SR_LP_XCD=0: workgroups in plain order, not grouped by XCD
  bool lp_long_ring = false;  // MOF_SR_LP_RING=16: the 16-deep staging ring also for maps whose boxes fit the 12-deep one
  int lp_ipw = 0;         // MOF_SR_LP_IPW > 0: images per wave of the staged kernel; 0: from the batch size
};
// Which kernels an estimator launches and how large its buffers are, decided once at create (sr_route)
struct SrRoute {
  enum Family { TUNED, TUNED_PAD, PLANNED };
  Family family = TUNED;  // TUNED: K5s / K6s / K7 + K8 on the resolution itself; the resolution padded to m = getOptimalDFTSize: TUNED_PAD, the
                          // zero-padding frame form of K5s, K6s, K7 and the planned pipeline's final kernel -- or PLANNED, L5 - L8 (pc_large_kernel.hip)
  int m = 0;              // transform size
  bool sums = false;      // TUNED_PAD at 250 / 400 / 432: a frame's four exact pixel sums sit `sums_off` floats into its Zh slot (the slack
  size_t sums_off = 0;    // behind the padded rows), so they travel wherever the slot is copied
  size_t zh_floats = 0;   // floats of one image's row half-spectra (Dt has the same shape)
  int candidates = 0;     // peak candidates per pair
  int seq_run = 0;        // pairs one wave of K6s walks in time: 0 = chosen per pass, MOF_SR_SEQ_RUN fixes it (r05: 16)
};
// Pure host code (no HIP call): the route of an even resolution >= 16; *plan receives the line plan of the padded families. False: the
// resolution pads beyond the planned transforms.
bool sr_route(int resolution, const SrKnobs& k, PcPlan* plan, SrRoute* r);
int sr_candidates(int res);
// Which remap kernel an estimator's batches take under one interpolation, decided once at create (sr_lp_route) from the map's boxes
struct SrLpRoute {
  // PIXEL: one gather per destination pixel, weights from L2; TABLE: the weight table in LDS; WAVE / SUPER: tile-stationary with the
  // source box of an 8 x 8 tile (one wave) / a 16 x 16 super-tile (four waves) staged in LDS
  enum Form { PIXEL, TABLE, WAVE, SUPER };
  Form form = PIXEL;
  int interp = 2;         // 2 cubic, 4 Lanczos4
  int res = 0;
  int ring = 0;           // WAVE / SUPER: depth of the staging ring, 12 or 16
  size_t lds = 0;         // WAVE / SUPER: dynamic LDS of a workgroup
  int ipw = 0;            // SrKnobs::lp_ipw, lp_xcd as the plans read them
  bool xcd = true;
};
// What one call launches (sr_lp_plan)
struct SrLpPlan {
  SrLpRoute::Form form = SrLpRoute::PIXEL;  // the form this batch takes: fewer than four staged images fall to TABLE, fewer than four images to PIXEL
  int n_st = 0;           // images of that launch: all of them, or all but the last where last_pixel
  bool last_pixel = false;  // WAVE / SUPER on a layout that is not whole dwords: the last image takes the per-pixel kernel (it has nothing behind it)
  int ipw = 0, xcd_groups = 0;  // WAVE / SUPER: images per wave; image groups the workgroups are ordered by XCD over (0: plain order)
  long grid = 0;          // workgroups (PIXEL: per image; TABLE: before the cap at the device's CU count)
};
// Pure host code (no HIP call, no environment, no static state). box_dwords_max / sbox_dwords_max: the largest per-tile / per-super-tile box
// of the map under this interpolation's footprint (sr_tile_boxes); has_sboxes: the super-tile boxes exist (res % 16 == 0)
SrLpRoute sr_lp_route(int res, int box_dwords_max, int sbox_dwords_max, bool has_sboxes, int interp, const SrKnobs& k);
// dword_layout: row pitch and image stride of the source are whole dwords
SrLpPlan sr_lp_plan(const SrLpRoute& r, int n_images, bool dword_layout);
// a.boxes, a.wplanes [, a.sboxes] as r was made from
hipError_t launch_sr_logpolar(const SrLpArgs& a, const SrLpRoute& r, int n_images, hipStream_t stream);
// K7 + K8 alone (uses a.Dt, a.cand, a.twiddles, a.M, a.out)
hipError_t launch_sr_peak(const SrPcArgs& a, int res, int n_pairs, hipStream_t stream);
// Sequence pipeline (sr_seq_kernel.hip). Zh = the row half-spectra of ONE log-polar image, doubled and transposed:
// [(res/2 + 1) u][res v] complex floats = sr_zh_floats(res) floats.
size_t sr_zh_floats(int res);
// (1, 0, 0, 0): the first frame's result (:74); quality2 (nullable): (NaN, NaN), no correlation ran
hipError_t launch_sr_identity(double* out4, double* quality2, hipStream_t stream);
// K5s: images lp + f * lp_stride (res * res u8, tightly packed rows) -> zh + f * zh_stride (strides: bytes / floats)
hipError_t launch_sr_rows_real(const uint8_t* lp, size_t lp_stride, const float* twiddles, float* zh, size_t zh_stride, int res,
                               int n_frames, hipStream_t stream);
// K5s on patches of frames and K7 alone: the tuned transforms under the FFT engine's large-patch pipeline and the estimator's padded resolutions
struct SrRowsSrc {
  PclSrc src;
  const float* twiddles;  // res (cos, -sin) pairs
  float* zh;              // image f -> zh + f * zh_stride floats
  size_t zh_stride;
  int* flags;             // as launch_pcl_rows (nullable)
  int res;                // transform size
  int channels;           // 1 or 3
  int n;                  // n <= res: the unpadded patch size (zeros beyond n x n)
  int* sums;              // nullable: 4 ints per image (zeroed; src.sums_stride apart), the exact sums sum (+-1)^y (+-1)^x p -- filled by the plans
                          // whose Nyquist bin is not exact (250, 400, 432)
};
hipError_t launch_sr_rows_real_src(const SrRowsSrc& a, int n_images, hipStream_t stream);
hipError_t launch_sr_rows_inv(const float* Dt, const float* twiddles, float2* cand, int res, int n_pairs, hipStream_t stream);
// a video's per-image flags fs[frame * patches + patch] -> the per-pair layout the column kernel and the tail read: f2[2 q] = cur = fs[q + patches],
// f2[2 q + 1] = prev = fs[q] (pair q = k * patches + patch of frames k + 1, k)
hipError_t launch_pcl_seq_flags(const int* fs, int* f2, int patches, int n_pairs, hipStream_t stream);
// K6s: pair p = (cur: zh_cur + p * zh_stride, prev: zh_prev + p * zh_stride) -> Dt[p]
struct SrColsSeq {
  const float* zh_prev;
  const float* zh_cur;
  size_t zh_stride;
  const float* twiddles;
  float* Dt;
  int res;                // transform size
  int run;                // > 1 lets one wave walk that many consecutive pairs re-using cur(p) as prev(p + 1) -- only valid when
                          // zh_cur == zh_prev + zh_stride (a sequence)
  const int* flags;       // nullable; flags + n < res: the box-zero rule of padded constant patches (run = 1)
  int n;                  // the unpadded size; 0: res
  const int* sums_prev;   // the rows kernel's exact sums (nullable where the plan's Nyquist bin is exact), pair p at p * sums_stride ints
  const int* sums_cur;
  int sums_stride;
};
hipError_t launch_sr_cols_seq(const SrColsSeq& a, int n_pairs, hipStream_t stream);
int sr_seq_columns_per_wave(int res);  // K6s's columns per wave at transform size res; 0: no K6s there

// ---- the camera front end (fe_kernel.hip): cv::resize by an exact integer factor, crop, CV_RGB2GRAY -> gray crops ----
struct FeArgs {
  const uint8_t* src;      // device, frame f at src + f * src_stride, rows src_pitch bytes apart, CH bytes per pixel
  size_t src_stride, src_pitch;
  uint8_t* dst;            // device, frame f at dst + f * dst_stride, rows dst_pitch bytes apart
  size_t dst_stride, dst_pitch;
  int scale;               // integer downscale factor s >= 1 (the source sides divisible by it)
  int crop_x, crop_y, crop_w, crop_h;  // in the downscaled image
  unsigned total;          // lanes of one launch (set by the launcher)
};
int frontend_run_pixels(int channels, int scale);  // output pixels per lane
// channels 1 or 3; lanes per frame = crop_h * ceil(crop_w / frontend_run_pixels) must stay <= 2^31
hipError_t launch_frontend(const FeArgs& a, int channels, int n_frames, hipStream_t stream);

}  // namespace mof
