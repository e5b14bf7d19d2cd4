// mof_capi.hip -- implementation of the C ABI declared in include/mof.h.
//
// Host-side engine objects (device buffers, one HIP stream each, the stateful previous
// frame of the reference's processors) around the gfx950 kernels. There is no CPU compute
// path in this library: without a HIP device every create() fails with MOF_ERR_NO_DEVICE.

#include "mof.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "capi_graph.hpp"
#include "host_pipe.hpp"
#include "mof_kernels.h"
#include "pc_launch.hpp"

// The response gate's kernel and its launcher (mof::launch_pc_response_gate): no translation unit of its own -- this file is its only
// caller and held no device code before, so the gate adds one code object to the library and changes none.
#include "pc_gate_kernel.hip"
// ... and so are the kernels of the predicted-shift window offsets (launch_pc_offset_gather / _finish, launch_pc_pred_from_coarse)
#include "pc_offset_kernel.hip"

namespace {
thread_local char g_err[512] = "";
}  // namespace

namespace mof {
// shared with the other host files (capi_graph.hpp): records the calling thread's last error text, returns `code`
int capi_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// twiddles W_n^k = exp(-2 pi i k / n), k < n, as (re, im) float pairs: computed in double, the axis values exact
std::vector<float> twiddle_table(int n) {
  std::vector<float> tw(2 * (size_t)n);
  for (int k = 0; k < n; ++k) {
    double ang = -2.0 * 3.14159265358979323846 * (double)k / (double)n;
    double c = std::cos(ang), s = std::sin(ang);
    if ((4 * k) % n == 0) {
      const int q = (4 * k) / n;
      c = (q == 0) ? 1.0 : (q == 2) ? -1.0 : 0.0;
      s = (q == 1) ? -1.0 : (q == 3) ? 1.0 : 0.0;
    }
    tw[2 * (size_t)k] = (float)c;
    tw[2 * (size_t)k + 1] = (float)s;
  }
  return tw;
}

namespace {
struct Parked {
  void (*destroy_now)(void*);
  void* engine;
};
std::mutex g_parked_mutex;
std::vector<Parked> g_parked;
}  // namespace

void park_engine(void (*destroy_now)(void*), void* engine) {
  std::lock_guard<std::mutex> lock(g_parked_mutex);
  g_parked.push_back(Parked{destroy_now, engine});
}

int purge_parked() {
  std::vector<Parked> todo;
  {
    std::lock_guard<std::mutex> lock(g_parked_mutex);
    todo.swap(g_parked);
  }
  for (const Parked& p : todo) p.destroy_now(p.engine);
  return (int)todo.size();
}

int parked_count() {
  std::lock_guard<std::mutex> lock(g_parked_mutex);
  return (int)g_parked.size();
}
}  // namespace mof

namespace mof {

// The knobs, read at the first create of the process
const FftKnobs& fft_knobs() {
  static const FftKnobs k = [] {
    FftKnobs r;
    const char* v;
    r.half = (v = getenv("MOF_FFT_HALF")) ? atoi(v) : -1;
    r.force_planned = getenv("MOF_FFT_FORCE_PLANNED") != nullptr;
    r.force_large = getenv("MOF_FFT_FORCE_LARGE") != nullptr;
    r.seq_pairs = getenv("MOF_FFT_SEQ_PAIRS") != nullptr;
    r.seq_half128 = getenv("MOF_FFT_SEQ_HALF128") != nullptr;
    r.half_seq_off = (v = getenv("MOF_FFT_HALF_SEQ")) && atoi(v) == 0;
    r.large_tuned = !(v = getenv("MOF_FFT_LARGE_TUNED")) || atoi(v) != 0;
    r.large_video = !(v = getenv("MOF_FFT_LARGE_VIDEO")) || atoi(v) != 0;
    if ((v = getenv("MOF_FFT_SEQ_RUN")) && atoi(v) >= 1) r.seq_run = atoi(v);
    if ((v = getenv("MOF_FFT_LARGE_PASS")) && atoi(v) > 0) r.large_pass = atoi(v);
    r.planned_static = !(v = getenv("MOF_PLANNED_STATIC")) || atoi(v) != 0;
    return r;
  }();
  return k;
}

// The planned transform sizes where the fused half-tile kernel (K1h) is the default: it beats the full-tile planned kernel on the box at
// 60, 96, 100 (p60 1.10 -> 1.38 M, p96 757 -> 855 k pairs/s, profiles/r05_half_vs_planned_bench_ab.txt, r05_half_vs_planned_rates.txt),
// at 72, 90 (+3 % on pairs, and the video form: profiles/r05_half_vs_planned_final.txt) and at 120 -- patches of 109 .. 119 pixels pad
// to 120 and follow N = 120 itself (the planned kernel at 120: 869 k against 1.30 M pairs/s). On patches padded to 64 it loses 4 % (p62).
static bool half_default_planned(int m) {
  for (int s : {60, 72, 90, 96, 100, 120})
    if (m == s) return true;
  return false;
}

bool fft_route(int patch_size, int peak_model, const FftKnobs& k, PcPlan* plan, FftRoute* r) {
  const bool ocv = peak_model == MOF_PEAK_OPENCV;
  *r = FftRoute{};
  if (pc_patch_size_supported(patch_size) && !k.force_planned && !k.force_large)
    r->family = FftRoute::TUNED;
  else if (!(k.force_large && ocv) && pc_build_plan(patch_size, plan))  // (MOF_FFT_FORCE_LARGE with MOF_PEAK_OCL: the planned kernel)
    r->family = FftRoute::PLANNED;
  else if (pc_build_line_plan(patch_size, plan))
    r->family = FftRoute::LARGE;
  else
    return false;
  const bool tuned = r->family == FftRoute::TUNED, planned = r->family == FftRoute::PLANNED;
  const int m = r->m = tuned ? patch_size : plan->m;
  // The fused half-tile kernel: the default for large patches whose half tile fits a CU (even padded size <= 192); MOF_FFT_HALF=0 keeps
  // them on the pipeline through HBM scratch, MOF_FFT_HALF=1 also routes the tuned / planned sizes it is instantiated for through it.
  // r05: N = 120 -- the reference's default samplePointSize -- takes it by default too: two workgroups per CU and every phase on all
  // waves beat the tuned one-workgroup kernel there (1.14 M against 1.10 M pairs/s same-box, profiles/r05_half_raw_pairsrc_ab.txt),
  // and so do the planned sizes of half_default_planned; the tuned N = 64 / 128 pair kernels stay faster than it and keep their sizes.
  // Long-range launches stay on the family's kernel (launch_field).
  const bool half_ok = ocv && k.half != 0 && !k.force_large && !k.force_planned;
  if (half_ok && pc_half_supported(m) &&
      (r->family == FftRoute::LARGE || k.half == 1 || (tuned && m == 120) || (planned && half_default_planned(m))))
    r->half_m = m;
  // The video form. The half-tile kernel's sequence form: every size it serves by default but 162 (MOF_FFT_HALF_SEQ=0 keeps the pair form);
  // 128 x 128 patches, whose pair form stays on the tuned kernel -- there it beats the older half-tile sequence kernel (pc_seq_half.hip: one
  // 8-wave workgroup per CU, 192 VGPRs), c4seq 93.3 k -> 112 k pairs/s, MOF_FFT_SEQ_HALF128=1 keeps that one; and the planned sizes where only
  // the video form wins (50, 54, 108: pc_half_kernel.hip, MOF_HALF_SEQ_SIZES).
  int kh_m = r->half_m;
  if (kh_m == 0 && tuned && m == 128 && !k.seq_half128) kh_m = 128;
  if (kh_m == 0 && planned && half_ok && !pc_half_supported(m)) kh_m = m;
  if (kh_m > 0 && ocv && !k.seq_pairs && !k.half_seq_off && pc_half_sequence_supported(kh_m)) {
    r->video = FftRoute::HALF_SEQ;
    r->video_m = kh_m;
    r->min_run = 4;  // (the launchers' own run lengths are at least 4 / 2; pc_seq_half.hip takes 16)
  } else if (tuned && !k.seq_pairs && pc_sequence_half_supported(m)) {
    r->video = FftRoute::SEQ_HALF;
    r->min_run = 16;
  } else if (tuned && !k.seq_pairs && pc_sequence_supported(m)) {
    r->video = FftRoute::SEQ;
    r->min_run = 2;
  }
  if (r->family == FftRoute::LARGE) {
    // r06: the tuned transform sizes from 200 on (sr_transform_size_tuned; 96 .. 192 keep L5 / L6 / L7 under MOF_FFT_HALF=0 and
    // MOF_FFT_FORCE_LARGE=1), and patches that PAD to one of them: the row kernel zero-pads, the column kernel applies the box-zero rule
    // of padded constant patches from the row kernel's flags. Unpadded patches of 240 / 256 / 480 pixels (the reference's whole-frame
    // fallback among them, FftMethod.cpp:1709-1716) run them 2.5 x faster than the planned kernels, same Zh / Dt / candidate formats.
    bool exact = true;
    // MOF_PEAK_OCL (never padded) keeps L5 - L8, whose PK = 1 forms carry its model (the tuned K6s / K7 have cv::phaseCorrelate's only)
    r->large_tuned = ocv && k.large_tuned && m >= 200 && sr_transform_size_tuned(m, &exact);
    r->odd_tail = r->large_tuned && !exact;
    r->large_video = r->large_tuned && k.large_video;
  }
  r->variant = r->half_m > 0 ? "planned-half" : (r->family == FftRoute::LARGE ? "planned-large" : (planned ? "planned" : "stockham"));
  r->seq_run = k.seq_run;
  r->large_pass = k.large_pass;
  r->planned_static = k.planned_static;
  return true;
}

}  // namespace mof

namespace {

constexpr auto& fail = mof::capi_fail;

using mof::BusyGuard;
using mof::FftRoute;

}  // namespace

// Member order is the teardown order in reverse (dev_mem.hpp): the stream and the fence's event are declared before the buffers, the
// host pipes last, so `delete e` -- after the waits of fft_destroy_now -- releases pipes, buffers, event, stream in that order.
struct mof_fft_engine {
  mof_fft_config cfg{};
  mof::Stream stream;
  mof::ScratchFence fence;                // cross-stream ordering of the large-patch scratch
  mof::ScratchFence gate_fence;           // ... and of the response gate's quality buffer (d_gate_q; created with it)
  mof::ScratchFence pred_fence;           // ... and of the window-offset scratch (d_pred_*; created with it)
  mof::ScratchFence finish_fence;         // ... and of K1's peak records (d_finish; created with it)
  mof::DevMem<float> d_twiddles;
  mof::DevMem<uint8_t> d_frames[2];       // [cur_slot], [1-cur_slot] = previous
  int prev_slot = 0;
  size_t frame_bytes = 0;
  mof::DevMem<double> d_out;              // one frame's results
  mof::PinnedMem<double> h_out;
  mof::DevMem<double> d_quality;          // one frame's (response, peak) per patch, beside d_out / h_out (the stateful *_q entries)
  mof::PinnedMem<double> h_quality;
  mof::PinnedMem<uint8_t> h_stage;        // upload staging (tightly packed frame)
  bool first = true;                      // FftMethod.cpp:1761
  FftRoute route;
  mof::PcPlan plan{};                     // route.family PLANNED / LARGE
  // scratch of the large-patch pipeline, for `cap` patch pairs per pass: row half-spectra of 2 cap patches, Dt, peak
  // candidates, constant-patch flags, C_dc. Grown by a batch that needs more (never under a graph capture, never while pinned).
  mof::DevMem<float> d_zh, d_dt, d_cdc;
  mof::DevMem<float2> d_cand;
  mof::DevMem<int> d_flags;
  int cap = 0;
  // K1 at 64 under cv::phaseCorrelate's peak model: the records between the field kernel and pc_finish_kernel, one launch piece's worth
  // (mof_kernels.h, pc_finish_records). Made with the engine and never resized: no call grows it, inside a capture or outside.
  mof::DevMem<uint32_t> d_finish;
  int finish_records = 0;
  // the response gate (mof_fft_set_min_response; 0 = off): where a batched call brings no quality buffer the kernels store the response
  // the gate reads into d_gate_q, for gate_cap patches -- made and grown as the large-patch scratch is, ordered by a fence of its own
  std::atomic<double> min_response{0.0};  // (mof_fft_min_response reads it without the busy flag)
  mof::DevMem<double> d_gate_q;
  size_t gate_cap = 0;
  // predicted-shift window offsets (mof_fft_process_batch_device_pred, the coarse-to-fine entries): the displaced previous windows of one
  // pass of frame pairs (pred_bytes, at the caller's pitch), and per pair of a call the predictions and applied predictions the caller
  // did not bring plus the long-range shifts (pred_pairs). Made by the first call, grown as the gate's buffer is.
  mof::DevMem<uint8_t> d_pred_frames;
  size_t pred_bytes = 0;
  mof::DevMem<int32_t> d_pred_xy, d_pred_applied;
  mof::DevMem<double> d_pred_coarse;
  int pred_pairs = 0;
  // how the window-offset entries read the displaced windows (mof_fft_set_pred_route): MOF_PRED_ROUTE_GATHER through d_pred_frames, or
  // MOF_PRED_ROUTE_FUSED inside the field kernel (PcArgs::prev_off) -- no d_pred_frames, overlapping layouts and BGR8 frames served
  std::atomic<int> pred_route{MOF_PRED_ROUTE_GATHER};  // (mof_fft_pred_route reads it without the busy flag)
  std::atomic<bool> busy{false};
  std::atomic<bool> graph_pinned{false};  // a batch call was captured into a HIP graph (capi_graph.hpp)
  std::mutex host_mu;                     // mof_fft_process_batch_host: upload / run / download pipeline (host_pipe.hpp), made by its first call
  std::unique_ptr<mof::HostPipe> host_pipe;
  std::unique_ptr<mof::HostPipe> host_pipe_q;  // mof_fft_process_batch_host_q with a quality output: the same pipeline with a second output
};

static hipError_t large_alloc(mof_fft_engine* e, int cap) {
  mof::RelaxedCapture relaxed;
  const size_t zhf = mof::pcl_zh_floats(e->plan), n = (size_t)cap;
  e->cap = 0;
  // d_flags: [0, 2 cap): flags per pair (cur | prev); [2 cap, 4 cap): flags per image of a video pass; [4 cap, 12 cap): four exact pixel sums
  // per image (the tuned transform sizes whose Nyquist bin is not exact: 250, 400, 432)
  const hipError_t err = mof::alloc_all(e->d_zh, 2 * n * zhf, e->d_dt, n * zhf, e->d_cand, n * mof::pcl_candidates(e->plan), e->d_flags, 12 * n,
                                        e->d_cdc, n);
  if (err == hipSuccess) e->cap = cap;
  return err;
}

// Frame pairs per pass of the large-patch pipeline: as many as keep the scratch (three Zh-sized planes per patch pair) under
// ~1.5 GB, at least one (MOF_FFT_LARGE_PASS overrides, sweeps)
static int large_pass_pairs(const mof_fft_engine* e, int patches) {
  if (e->route.large_pass > 0) return e->route.large_pass;
  const size_t per_pair = (size_t)3 * patches * mof::pcl_zh_floats(e->plan) * sizeof(float);
  const size_t n = ((size_t)3 << 29) / (per_pair ? per_pair : 1);
  return n < 1 ? 1 : (n > 4096 ? 4096 : (int)n);
}

// the scratch of a call of n_pairs frame pairs of `patches` patches on stream s: a whole pass at most (launch_large, mof_fft_reserve_pred)
static int large_reserve(mof_fft_engine* e, int patches, int n_pairs, hipStream_t s) {
  const int pass_max = large_pass_pairs(e, patches);
  const int want_pairs = n_pairs < pass_max ? n_pairs : pass_max;
  return mof::grow_scratch(e->graph_pinned.load(), e->fence, {e->stream}, mof::stream_capturing(s), "the large-patch scratch (patch pairs)",
                           e->cap, (long)want_pairs * patches, (long)e->cfg.grid_x * e->cfg.grid_y,
                           [e](long cap) { return large_alloc(e, (int)cap); });
}

// The large-patch pipeline on n_pairs frame pairs (a.grid_* patches each; a.downscale / a.channels as K1): passes of whole frame
// pairs through the engine's scratch. Returns a MOF status.
static int launch_large(mof_fft_engine* e, const mof::PcArgs& a, int n_pairs, hipStream_t s) {
  const int patches = a.grid_x * a.grid_y;
  {
    const int rc = large_reserve(e, patches, n_pairs, s);
    if (rc != MOF_OK) return rc;
  }
  HIP_TRY(e->fence.acquire(s));
  const size_t zhf = mof::pcl_zh_floats(e->plan);
  const FftRoute& r = e->route;
  const bool tuned = r.large_tuned && a.downscale == 1;  // (the long-range mode keeps the planned kernels)
  // r06, a VIDEO on the tuned transforms (pair k = (frame k + 1, frame k): mof_fft_process_sequence_device, or any caller whose cur = prev + one frame):
  // every frame's row spectra are formed ONCE per pass -- Zh slot = frame * patches + patch, so pair q = k * patches + patch finds its previous
  // image at slot q and its current one at slot q + patches, which is exactly what the column kernel's (zh_prev, zh_cur, stride) takes; the
  // kernels and their arithmetic are the pair form's, so are the bits. Otherwise image 2 q + which (0 cur, 1 prev) of every pair q.
  const bool video = r.large_video && tuned && n_pairs >= 2 && a.cur == a.prev + a.prev_stride && a.cur_stride == a.prev_stride;
  mof::PclSrc src{};
  src.base[0] = video ? a.prev : a.cur;  // one unit of images: a frame of the video, or a frame pair
  src.stride[0] = video ? a.prev_stride : a.cur_stride;
  if (!video) {
    src.base[1] = a.prev;
    src.stride[1] = a.prev_stride;
  }
  src.pitch = a.pitch;
  src.paired = video ? 2 : 1;
  src.grid_x = a.grid_x;
  src.grid_y = a.grid_y;
  src.origin_x = a.origin_x;
  src.origin_y = a.origin_y;
  src.stride_x = a.stride_x;
  src.stride_y = a.stride_y;
  auto units_on = [&src](int k) {  // the source from unit k on
    mof::PclSrc u = src;
    u.base[0] += (size_t)k * src.stride[0];
    if (src.paired == 1) u.base[1] += (size_t)k * src.stride[1];
    return u;
  };
  const int per_unit = video ? patches : 2 * patches;  // images
  int* flags = e->d_flags + (video ? (size_t)2 * e->cap : 0);  // per image of a pass (the video's are spread to pairs by launch_pcl_seq_flags)
  int* sums = e->d_flags + (size_t)4 * e->cap;  // four ints per image (r->odd_tail)
  const float* zh_prev = e->d_zh + (video ? 0 : zhf);
  const float* zh_cur = e->d_zh + (video ? (size_t)patches * zhf : 0);
  const size_t zh_stride = video ? zhf : 2 * zhf;
  const int* sums_prev = sums + (video ? 0 : 4);
  const int* sums_cur = sums + (video ? 4 * patches : 0);
  const int sums_stride = video ? 4 : 8;
  mof::PclFinal f{};
  f.Dt = e->d_dt;
  f.cand = e->d_cand;
  f.twiddles = e->d_twiddles;
  f.mode = 1;
  f.max_px_speed_sq = a.max_px_speed_sq;
  f.flags = e->d_flags;
  f.cdc = e->d_cdc;
  f.peak_model = e->cfg.peak_model;
  f.search_radius = e->cfg.search_radius;
  const int per_pass = e->cap / patches;
  for (int k0 = 0; k0 < n_pairs; k0 += per_pass) {
    const int np = n_pairs - k0 < per_pass ? n_pairs - k0 : per_pass, nq = np * patches;
    const int units = video ? np + 1 : np;
    HIP_TRY(hipMemsetAsync(flags, 0, (size_t)units * per_unit * sizeof(int), s));
    if (tuned && r.odd_tail) HIP_TRY(hipMemsetAsync(sums, 0, (size_t)4 * units * per_unit * sizeof(int), s));
    // (the row launchers split at 65534 images, a pair form on pair boundaries: keep a launch's image count a multiple of a unit below that)
    const int units_per_launch = mof::PC_MAX_GRID_IMAGES / per_unit > 0 ? mof::PC_MAX_GRID_IMAGES / per_unit : 1;
    for (int j0 = 0; j0 < units; j0 += units_per_launch) {
      const int nj = units - j0 < units_per_launch ? units - j0 : units_per_launch;
      const mof::PclSrc sj = units_on(k0 + j0);
      float* zh = e->d_zh + (size_t)j0 * per_unit * zhf;
      if (tuned)
        HIP_TRY(mof::launch_sr_rows_real_src(mof::SrRowsSrc{sj, e->d_twiddles, zh, zhf, flags + (size_t)j0 * per_unit, e->plan.m, a.channels, e->plan.n,
                                                            sums + (size_t)4 * j0 * per_unit}, nj * per_unit, s));
      else
        HIP_TRY(mof::launch_pcl_rows(sj, e->plan, e->d_twiddles, zh, zhf, flags + (size_t)j0 * per_unit, nj * per_unit, a.channels,
                                     a.downscale, s));
    }
    if (video) HIP_TRY(mof::launch_pcl_seq_flags(flags, e->d_flags, patches, nq, s));
    if (tuned) {
      HIP_TRY(mof::launch_sr_cols_seq(mof::SrColsSeq{zh_prev, zh_cur, zh_stride, e->d_twiddles, e->d_dt, e->plan.m, 1, e->d_flags, e->plan.n,
                                                     sums_prev, sums_cur, sums_stride}, nq, s));
      HIP_TRY(mof::launch_pcl_cdc(zh_prev, zh_cur, zh_stride, e->plan.m, e->d_cdc, nq, s));
      HIP_TRY(mof::launch_sr_rows_inv(e->d_dt, e->d_twiddles, e->d_cand, e->plan.m, nq, s));
    } else {
      HIP_TRY(mof::launch_pcl_cols(zh_prev, zh_cur, zh_stride, e->plan, e->d_twiddles, e->d_dt, e->d_cdc, e->d_flags, nq, s, e->cfg.peak_model));
    }
    f.out = a.out + (size_t)k0 * patches * 2;
    f.quality = a.quality ? a.quality + (size_t)k0 * patches * 2 : nullptr;
    HIP_TRY(mof::launch_pcl_peak(f, e->plan, nq, s, tuned));
  }
  HIP_TRY(e->fence.release(s));
  return MOF_OK;
}

// every K1 launch of an engine: the hand-tuned instantiation of its patch size, the planned general kernel, or -- for patches
// too large for a CU -- the planned pipeline through HBM scratch. Returns a MOF status.
static int launch_field(mof_fft_engine* e, const mof::PcArgs& a, int n_pairs, hipStream_t stream) {
  const FftRoute& r = e->route;
  // one bound for every entry and every kernel family (K1's one-patch forms need it: mof_kernels.h, PC_MAX_PITCH)
  if (a.pitch >= mof::PC_MAX_PITCH) return fail(MOF_ERR_BAD_ARG, "row pitch of 16 MiB or more");
  if (a.prev_off && !(a.downscale == 1 && mof::fft_pred_fused_supported(r, a.peak_model)))  // (mof_fft_set_pred_route keeps this from happening)
    return fail(MOF_ERR_UNSUPPORTED, "this engine's kernels have no fused window-offset form");
  if (r.half_m > 0 && a.downscale == 1) {  // (no scratch, nothing engine-owned but the twiddles)
    HIP_TRY(mof::launch_pc_half(a, r.half_m, e->cfg.patch_size, n_pairs, stream));
    return MOF_OK;
  }
  if (r.family == FftRoute::LARGE) return launch_large(e, a, n_pairs, stream);
  if (r.family == FftRoute::PLANNED) {
    HIP_TRY(mof::launch_pc_generic(a, e->plan, r.planned_static, n_pairs, stream));
    return MOF_OK;
  }
  // the tuned kernels; K1 at 64 hands its peak records to its finish kernel through the engine's buffer, ordered across streams as the
  // other engine-owned scratch is
  const bool records = e->finish_records > 0;
  if (records) HIP_TRY(e->finish_fence.acquire(stream));
  HIP_TRY(mof::launch_pc_field(a, e->cfg.patch_size, n_pairs, stream, e->d_finish, e->finish_records));
  if (records) HIP_TRY(e->finish_fence.release(stream));
  return MOF_OK;
}
// once per engine, before its first launch: the dynamic-LDS limits of the kernels launch_field and fft_sequence can launch on route r
// (a video's half-tile form runs at half_m whenever that is set); the large-patch pipeline's kernels need none
static hipError_t configure_route(const FftRoute& r) {
  hipError_t err = hipSuccess;
  if (r.half_m > 0 || r.video == FftRoute::HALF_SEQ) err = mof::pc_configure_half(r.half_m > 0 ? r.half_m : r.video_m);
  if (err == hipSuccess && r.family == FftRoute::PLANNED) err = mof::pc_configure_generic();
  if (err == hipSuccess && r.family == FftRoute::TUNED) err = mof::pc_configure(r.m);
  if (err == hipSuccess && r.video == FftRoute::SEQ) err = mof::pc_configure_sequence();
  if (err == hipSuccess && r.video == FftRoute::SEQ_HALF) err = mof::pc_configure_sequence_half(r.m);
  return err;
}
#define FIELD_TRY(expr)       \
  do {                        \
    const int _rc = (expr);   \
    if (_rc != MOF_OK) return _rc; \
  } while (0)

// The response gate of the batched entries (mof_fft_set_min_response), in two steps around the field's launches on stream s.
// gate_begin, before anything is launched and before a capturing call pins the engine: where the gate is armed and the caller brought no
// quality buffer, *quality becomes the engine's own, grown to n_patches patches by the rules of the large-patch scratch (grow_scratch: not
// while pinned, not inside a capture) and acquired for s. gate_end, behind the last launch: the gate kernel over the call's patches, reading
// the doubles the field's kernels stored. Disarmed, neither does anything.
// A launch that fails between the two leaves the fence unreleased for the kernels already enqueued, as launch_large's error path leaves
// its own: the call has failed, its outputs are void, and every later user of the buffer on another stream is still ordered behind the
// last release; the buffer is freed only after the stream and the fence have been waited for (fft_destroy_now, grow_scratch's drain).
static int gate_begin(mof_fft_engine* e, size_t n_patches, hipStream_t s, double** quality, bool* own) {
  *own = false;
  if (!(e->min_response > 0.0) || *quality) return MOF_OK;
  const int rc = mof::grow_scratch(e->graph_pinned.load(), e->gate_fence, {e->stream}, mof::stream_capturing(s),
                                   "the response gate's quality buffer (patches)", (long)e->gate_cap, (long)n_patches, 0, [e](long cap) {
                                     mof::RelaxedCapture relaxed;
                                     e->gate_cap = 0;
                                     e->d_gate_q.reset();
                                     if (cap == 0) return hipSuccess;
                                     if (!e->gate_fence.ev) {
                                       const hipError_t err = e->gate_fence.create();
                                       if (err != hipSuccess) return err;
                                     }
                                     const hipError_t err = e->d_gate_q.alloc(2 * (size_t)cap);
                                     if (err == hipSuccess) e->gate_cap = (size_t)cap;
                                     return err;
                                   });
  if (rc != MOF_OK) return rc;
  HIP_TRY(e->gate_fence.acquire(s));
  *quality = e->d_gate_q;
  *own = true;
  return MOF_OK;
}
static int gate_end(mof_fft_engine* e, double* out, const double* quality, size_t n_patches, hipStream_t s, bool own) {
  if (!(e->min_response > 0.0)) return MOF_OK;
  HIP_TRY(mof::launch_pc_response_gate(out, quality, n_patches, e->min_response, s));
  if (own) HIP_TRY(e->gate_fence.release(s));
  return MOF_OK;
}

// (member order = teardown order in reverse, as mof_fft_engine: stream, buffers, host pipe)
struct mof_bm_engine {
  mof_bm_config cfg{};
  mof::Stream stream;
  mof::DevMem<uint8_t> d_frames[2];
  int prev_slot = 0;
  size_t frame_bytes = 0;
  mof::DevMem<int8_t> d_dx, d_dy, d_mode;
  mof::PinnedMem<int8_t> h_res;  // dx | dy | mode
  // the stateful _q entry's outputs (allocated by the first call that asks for one): 3 uint32 per block, then the gated-block count
  mof::DevMem<uint32_t> d_q;
  mof::PinnedMem<uint32_t> h_q;
  // the match gate (mof_bm_set_gate): kernel arguments, no buffer -- block-matching batches keep "never pin"
  uint32_t max_min_sad = 0xffffffffu, min_sad_range = 0u;
  mof::BmRoute route;  // which scan every launch runs and its shape (bm_route)
  mof::PinnedMem<uint8_t> h_stage;
  // BlockMethod::Refine scratch (allocated on first use): the two 2x images, nine SADs
  mof::DevMem<uint8_t> d_up[2];
  mof::DevMem<unsigned long long> d_sad9;
  mof::PinnedMem<unsigned long long> h_sad9;
  bool have_pair = false;      // a processImage call has been made (both frame slots are meaningful)
  std::atomic<bool> busy{false};
  std::atomic<bool> graph_pinned{false};
  std::mutex host_mu;          // mof_bm_process_batch_host's pipeline (host_pipe.hpp)
  std::unique_ptr<mof::HostPipe> host_pipe, host_pipe_q;  // (_q: with the quality and count slots, built by the first call that asks for one)
};

static void pack_frame(uint8_t* dst, const uint8_t* src, size_t pitch, int w, int h) {
  for (int y = 0; y < h; ++y) std::memcpy(dst + (size_t)y * w, src + (size_t)y * pitch, (size_t)w);
}

// the stateful entries' upload: `frame` packed into the pinned staging, then into frame slot `slot` on the engine's stream
template <class Engine>
static hipError_t upload_frame(Engine* e, int slot, const uint8_t* frame, size_t pitch) {
  pack_frame(e->h_stage, frame, pitch, e->cfg.frame_width, e->cfg.frame_height);
  return hipMemcpyAsync(e->d_frames[slot], e->h_stage, e->frame_bytes, hipMemcpyHostToDevice, e->stream);
}

// setImPrev of both engine kinds
template <class Engine>
static int set_prev(Engine* e, const uint8_t* frame, size_t pitch) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (!frame || pitch < (size_t)e->cfg.frame_width) return fail(MOF_ERR_BAD_ARG, "bad frame/pitch");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(upload_frame(e, e->prev_slot, frame, pitch));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MOF_OK;
}

extern "C" {

const char* mof_version(void) { return "mof-hip 0.1.0 (gfx950)"; }
const char* mof_last_error(void) { return g_err; }

int mof_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n < 0 ? 0 : n;
}

/* ------------------------------------------------------------------------------------------ */
/* FFT                                                                                        */
/* ------------------------------------------------------------------------------------------ */

int mof_fft_config_reference(mof_fft_config* cfg, int frame_size, int sample_point_size, double max_px_speed) {
  if (!cfg || frame_size < 2 || sample_point_size < 1) return fail(MOF_ERR_BAD_ARG, "bad reference geometry");
  std::memset(cfg, 0, sizeof(*cfg));
  if (frame_size % 2 == 1) frame_size--;                                           // FftMethod.cpp:1706-1708
  if (frame_size % sample_point_size != 0) sample_point_size = frame_size;         // :1709-1716
  const int sq = frame_size / sample_point_size;                                   // :1719
  cfg->frame_width = cfg->frame_height = frame_size;
  cfg->patch_size = sample_point_size;
  cfg->grid_x = cfg->grid_y = sq;
  cfg->origin_x = cfg->origin_y = 0;
  cfg->stride_x = cfg->stride_y = sample_point_size;
  cfg->max_px_speed = max_px_speed;
  cfg->device = 0;
  cfg->peak_model = MOF_PEAK_OPENCV;  // useOCL = false, the live path
  cfg->search_radius = 55;            // SEARCH_RADIUS, FftMethod.cpp:820 (only read by MOF_PEAK_OCL)
  return MOF_OK;
}

static int validate_fft(const mof_fft_config* c) {
  if (!c) return fail(MOF_ERR_BAD_ARG, "null config");
  if (c->frame_width < 1 || c->frame_height < 1 || c->grid_x < 1 || c->grid_y < 1 || c->origin_x < 0 ||
      c->origin_y < 0 || c->stride_x < 0 || c->stride_y < 0)
    return fail(MOF_ERR_BAD_ARG, "bad FFT geometry");
  if (c->patch_size < 2) return fail(MOF_ERR_BAD_ARG, "patch_size %d: a patch needs at least 2 x 2 pixels", c->patch_size);
  // Whether a plan exists does not depend on the knobs: the default route answers. A size without a tuned kernel (any samplePointSize:
  // FftMethod.cpp:1680-1720 takes it from a ROS parameter) runs on the size cv::phaseCorrelate pads to, M = getOptimalDFTSize(N) -- the
  // planned kernel or, where the padded patch does not fit one CU's LDS (M > 135), the planned pipeline through HBM scratch
  mof::PcPlan plan;
  FftRoute route;
  if (!mof::fft_route(c->patch_size, c->peak_model, mof::FftKnobs{}, &plan, &route))
    return fail(MOF_ERR_UNSUPPORTED, "patch_size %d pads to %d: beyond the planned transforms (<= 960)", c->patch_size,
                mof::pc_optimal_dft_size(c->patch_size));
  // useOCL=true plans radix-{2,3,4,5,8} passes for the patch size itself and never pads (FftMethod.cpp:481-539, :787-816):
  // sizes with another prime factor have no OpenCL plan in the reference either; its CCS packing assumes an even size
  if (route.family != FftRoute::TUNED && c->peak_model == MOF_PEAK_OCL && (plan.m != plan.n || (plan.n & 1)))
    return fail(MOF_ERR_UNSUPPORTED, "peak_model MOF_PEAK_OCL needs an even patch_size of the form 2^a 3^b 5^c, up to 960 (the "
                "reference's OpenCL branch cannot plan %d either)", c->patch_size);
  if (c->origin_x + (long)(c->grid_x - 1) * c->stride_x + c->patch_size > c->frame_width ||
      c->origin_y + (long)(c->grid_y - 1) * c->stride_y + c->patch_size > c->frame_height)
    return fail(MOF_ERR_BAD_ARG, "patch grid leaves the frame");
  if ((long)c->grid_x * c->grid_y > (1 << 20)) return fail(MOF_ERR_BAD_ARG, "too many patches");
  if (!(c->max_px_speed >= 0.0)) return fail(MOF_ERR_BAD_ARG, "max_px_speed must be >= 0");
  if (c->peak_model != MOF_PEAK_OPENCV && c->peak_model != MOF_PEAK_OCL)
    return fail(MOF_ERR_BAD_ARG, "peak_model must be MOF_PEAK_OPENCV or MOF_PEAK_OCL");
  if (c->peak_model == MOF_PEAK_OCL && c->search_radius < 0) return fail(MOF_ERR_BAD_ARG, "search_radius must be >= 0");
  return MOF_OK;
}

// the waits that must precede any release of an engine's memory, then the release itself (member order, see the struct)
static void fft_destroy_now(void* p) {
  mof_fft_engine* e = static_cast<mof_fft_engine*>(p);
  mof::RelaxedCapture relaxed;  // frees must not invalidate a capture running on another thread
  (void)hipSetDevice(e->cfg.device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  e->fence.wait_idle();
  e->gate_fence.wait_idle();
  e->pred_fence.wait_idle();
  e->finish_fence.wait_idle();
  delete e;
}
struct FftDestroyNow {
  void operator()(mof_fft_engine* e) const { fft_destroy_now(e); }
};

int mof_fft_create(const mof_fft_config* cfg, mof_fft_engine** out) try {
  if (!out) return fail(MOF_ERR_BAD_ARG, "null out");
  *out = nullptr;
  int rc = validate_fft(cfg);
  if (rc) return rc;
  rc = mof::select_device(cfg->device);
  if (rc) return rc;
  mof::RelaxedCapture relaxed;  // allocating an engine must not invalidate a capture on another thread
  const size_t res = (size_t)cfg->grid_x * cfg->grid_y * 2;
  std::unique_ptr<mof_fft_engine, FftDestroyNow> e(new (std::nothrow) mof_fft_engine());  // every early return tears down what exists
  if (!e) return fail(MOF_ERR_NO_MEMORY, "out of host memory");
  e->cfg = *cfg;
  e->frame_bytes = (size_t)cfg->frame_width * cfg->frame_height;
  if (!mof::fft_route(cfg->patch_size, cfg->peak_model, mof::fft_knobs(), &e->plan, &e->route))  // (validate_fft has checked that a plan exists)
    return fail(MOF_ERR_UNSUPPORTED, "no plan for patch_size %d", cfg->patch_size);
  const FftRoute& r = e->route;
  std::vector<float> tw = mof::twiddle_table(r.m);
  mof::pc_append_twiddle_rows(tw, r.m);  // K1's packed rows behind the classic table (32 and 64; a no-op elsewhere)
  HIP_TRY(e->stream.create());
  HIP_TRY(mof::upload(e->d_twiddles, tw, e->stream));
  for (auto& frame : e->d_frames) {
    HIP_TRY(frame.alloc(e->frame_bytes));
    HIP_TRY(mof::fill_on(e->stream, frame, 0, e->frame_bytes));
  }
  HIP_TRY(mof::alloc_all(e->d_out, res, e->h_out, res, e->d_quality, res, e->h_quality, res, e->h_stage, e->frame_bytes));
  HIP_TRY(configure_route(r));
  if (r.family == FftRoute::LARGE) {
    HIP_TRY(e->fence.create());
    HIP_TRY(large_alloc(e.get(), cfg->grid_x * cfg->grid_y));  // one frame pair; a batch grows it to a whole pass
  }
  if (r.family == FftRoute::TUNED) {
    // (the long-range mode has fewer patches per frame than the full-resolution grid, never more)
    const int records = mof::pc_finish_records(cfg->patch_size, cfg->peak_model, cfg->grid_x * cfg->grid_y);
    if (records > 0) {
      HIP_TRY(e->finish_fence.create());
      HIP_TRY(e->d_finish.alloc((size_t)records * mof::PC_FINISH_DWORDS));
      e->finish_records = records;
    }
  }
  *out = e.release();
  return MOF_OK;
} catch (const std::bad_alloc&) {
  return fail(MOF_ERR_NO_MEMORY, "mof_fft_create: out of host memory");
}

const char* mof_fft_kernel_variant(const mof_fft_engine* e) {
  return e ? e->route.variant : "";
}

void mof_fft_destroy(mof_fft_engine* e) {
  if (!e) return;
  if (e->graph_pinned.load()) {  // a captured graph may still read the twiddles: keep them until the owner releases
    mof::park_engine(&fft_destroy_now, e);
    return;
  }
  fft_destroy_now(e);
}

int mof_fft_release_graphs(mof_fft_engine* e) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  e->graph_pinned.store(false);
  return MOF_OK;
}

int mof_fft_graph_pinned(const mof_fft_engine* e) { return e && e->graph_pinned.load() ? 1 : 0; }

int mof_purge_deferred(void) { return mof::purge_parked(); }
int mof_deferred_count(void) { return mof::parked_count(); }
int mof_live_buffers(void) { return mof::g_live_buffers.load(); }

static mof::PcArgs fft_args(const mof_fft_engine* e, const uint8_t* cur, size_t cs, const uint8_t* prev, size_t ps,
                            size_t pitch, double* out, double* quality) {
  mof::PcArgs a{};
  a.cur = cur;
  a.prev = prev;
  a.cur_stride = cs;
  a.prev_stride = ps;
  a.pitch = pitch;
  a.grid_x = e->cfg.grid_x;
  a.grid_y = e->cfg.grid_y;
  a.origin_x = e->cfg.origin_x;
  a.origin_y = e->cfg.origin_y;
  a.stride_x = e->cfg.stride_x;
  a.stride_y = e->cfg.stride_y;
  a.downscale = 1;
  a.channels = 1;
  a.peak_model = e->cfg.peak_model;
  a.search_radius = e->cfg.search_radius;
  a.max_px_speed_sq = e->cfg.max_px_speed * e->cfg.max_px_speed;  // pow(max_px_speed_t, 2), FftMethod.cpp:1686
  a.twiddles = e->d_twiddles;
  a.out = out;
  a.quality = quality;
  return a;
}

int mof_fft_set_prev(mof_fft_engine* e, const uint8_t* frame, size_t pitch) { return set_prev(e, frame, pitch); }

int mof_fft_reset(mof_fft_engine* e) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  e->first = true;  // (min_response stays: it is a setting, not state of the frame chain)
  return MOF_OK;
}

int mof_fft_set_min_response(mof_fft_engine* e, double min_response) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (!std::isfinite(min_response) || min_response < 0.0) return fail(MOF_ERR_BAD_ARG, "min_response must be finite and >= 0");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  // a captured graph holds the gate kernel with the old value as an argument, or no gate kernel at all: its replays would not follow
  if (e->graph_pinned.load()) return fail(MOF_ERR_BUSY, "min_response is baked into a captured graph: mof_fft_release_graphs first");
  e->min_response = min_response;
  return MOF_OK;
}

double mof_fft_min_response(const mof_fft_engine* e) { return e ? e->min_response.load() : 0.0; }

// Long-range geometry (FftMethod.cpp:1685, :1720): same patch size on the quarter-resolution frame,
// sqNum_lr = sqNum / 4 patches per side. Only defined for the reference's own tiling.
static int long_range_args(const mof_fft_engine* e, mof::PcArgs* a) {
  const mof_fft_config& c = e->cfg;
  if (c.origin_x || c.origin_y || c.stride_x != c.patch_size || c.stride_y != c.patch_size)
    return fail(MOF_ERR_UNSUPPORTED, "long-range mode needs the reference tiling (origin 0, stride = patch size)");
  if ((c.frame_width & 3) || (c.frame_height & 3) || c.grid_x < 4 || c.grid_y < 4)
    return fail(MOF_ERR_UNSUPPORTED, "long-range mode needs frame sides divisible by 4 and sqNum >= 4");
  a->grid_x = c.grid_x / 4;
  a->grid_y = c.grid_y / 4;
  a->downscale = 4;
  // the long-range gate is held in ints (`int max_px_speed_lr, max_px_speed_sq_lr`, FftMethod.h:393):
  // max_px_speed_lr = 1 * max_px_speed_t truncates, max_px_speed_sq_lr = pow(max_px_speed_lr, 2) (FftMethod.cpp:1687-1688)
  const int speed_lr = (int)c.max_px_speed;
  a->max_px_speed_sq = (double)(int)std::pow((double)speed_lr, 2);
  return MOF_OK;
}

int mof_fft_long_range_patches(const mof_fft_engine* e) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  mof::PcArgs a{};
  int rc = long_range_args(e, &a);
  return rc ? rc : a.grid_x * a.grid_y;
}

// processImage / processImageLongRange (FftMethod.cpp:1775-1900 / :1905-2004): one host frame against the engine's previous one
static int fft_process_frame(mof_fft_engine* e, const uint8_t* frame, size_t pitch, double* out_xy, double* quality, int* n_invalid,
                             bool long_range) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (!frame || !out_xy || pitch < (size_t)e->cfg.frame_width) return fail(MOF_ERR_BAD_ARG, "bad frame/pitch/out");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");  // reference: returns an empty vector
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int cur_slot = 1 - e->prev_slot;
  HIP_TRY(upload_frame(e, cur_slot, frame, pitch));
  // `first`: the frame is correlated with itself (FftMethod.cpp:1791-1793, :1920-1922)
  const uint8_t* prev = e->first ? e->d_frames[cur_slot] : e->d_frames[e->prev_slot];
  const bool armed = e->min_response > 0.0;  // (the gate reads the engine's d_quality whether or not the caller asked for it)
  mof::PcArgs a = fft_args(e, e->d_frames[cur_slot], 0, prev, 0, (size_t)e->cfg.frame_width, e->d_out, quality || armed ? e->d_quality.get() : nullptr);
  if (long_range) {
    int rc = long_range_args(e, &a);
    if (rc) return rc;
  }
  FIELD_TRY(launch_field(e, a, 1, e->stream));
  const size_t res = (size_t)a.grid_x * a.grid_y * 2;
  if (armed) HIP_TRY(mof::launch_pc_response_gate(e->d_out, e->d_quality, res / 2, e->min_response, e->stream));
  HIP_TRY(hipMemcpyAsync(e->h_out, e->d_out, res * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (quality) HIP_TRY(hipMemcpyAsync(e->h_quality, e->d_quality, res * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (quality) std::memcpy(quality, e->h_quality, res * sizeof(double));
  int bad = 0;
  for (size_t i = 0; i < res; i += 2) {
    out_xy[i] = e->h_out[i];
    out_xy[i + 1] = e->h_out[i + 1];
    if (std::isnan(e->h_out[i])) ++bad;
  }
  if (n_invalid) *n_invalid = bad;
  e->prev_slot = cur_slot;  // imPrev = imCurr.clone(), FftMethod.cpp:1872, :1992
  e->first = false;         // :1900, :2004
  return MOF_OK;
}

int mof_fft_process(mof_fft_engine* e, const uint8_t* frame, size_t pitch, double* out_xy, int* n_invalid) {
  return fft_process_frame(e, frame, pitch, out_xy, nullptr, n_invalid, false);
}

int mof_fft_process_q(mof_fft_engine* e, const uint8_t* frame, size_t pitch, double* out_xy, double* quality, int* n_invalid) {
  return fft_process_frame(e, frame, pitch, out_xy, quality, n_invalid, false);
}

int mof_fft_process_long_range(mof_fft_engine* e, const uint8_t* frame, size_t pitch, double* out_xy, int* n_invalid) {
  return fft_process_frame(e, frame, pitch, out_xy, nullptr, n_invalid, true);
}

int mof_fft_process_long_range_q(mof_fft_engine* e, const uint8_t* frame, size_t pitch, double* out_xy, double* quality, int* n_invalid) {
  return fft_process_frame(e, frame, pitch, out_xy, quality, n_invalid, true);
}

// The device batch entries: n_pairs frame pairs of `channels` interleaved channels (1 gray, 3 BGR8)
static int fft_batch(mof_fft_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev, size_t prev_stride, size_t pitch,
                     int n_pairs, double* d_out_xy, double* d_quality, void* stream, int channels, bool long_range) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (n_pairs == 0) return MOF_OK;  // an empty batch carries no pointers to check
  if (!d_cur || !d_prev || !d_out_xy || n_pairs < 0 || pitch < (size_t)channels * (size_t)e->cfg.frame_width)
    return fail(MOF_ERR_BAD_ARG, "bad batch arguments");
  if ((unsigned long long)n_pairs * (unsigned long long)(e->cfg.grid_x * e->cfg.grid_y) > 0x7fffffffull)
    return fail(MOF_ERR_BAD_ARG, "batch too large for one launch");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  mof::PcArgs a = fft_args(e, d_cur, cur_stride, d_prev, prev_stride, pitch, d_out_xy, d_quality);
  a.channels = channels;
  if (long_range) {
    int rc = long_range_args(e, &a);
    if (rc) return rc;
  }
  const size_t n_patches = (size_t)n_pairs * a.grid_x * a.grid_y;
  bool own_q = false;
  FIELD_TRY(gate_begin(e, n_patches, (hipStream_t)stream, &a.quality, &own_q));
  if (mof::stream_capturing((hipStream_t)stream)) e->graph_pinned.store(true);
  FIELD_TRY(launch_field(e, a, n_pairs, (hipStream_t)stream));
  return gate_end(e, a.out, a.quality, n_patches, (hipStream_t)stream, own_q);
}

int mof_fft_process_batch_device(mof_fft_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev,
                                 size_t prev_stride, size_t pitch, int n_pairs, double* d_out_xy, void* stream) {
  return fft_batch(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, d_out_xy, nullptr, stream, 1, false);
}

int mof_fft_process_batch_device_q(mof_fft_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev, size_t prev_stride,
                                   size_t pitch, int n_pairs, int channels, int long_range, double* d_out_xy, double* d_quality,
                                   void* stream) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if ((channels != 1 && channels != 3) || (long_range != 0 && long_range != 1))
    return fail(MOF_ERR_BAD_ARG, "channels must be 1 or 3 and long_range 0 or 1");
  if (channels == 3 && long_range) return fail(MOF_ERR_BAD_ARG, "the long-range mode takes gray frames only");
  return fft_batch(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, d_out_xy, d_quality, stream, channels, long_range != 0);
}

int mof_fft_process_batch_device_bgr(mof_fft_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev,
                                     size_t prev_stride, size_t pitch, int n_pairs, double* d_out_xy, void* stream) {
  return fft_batch(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, d_out_xy, nullptr, stream, 3, false);
}

int mof_fft_process_long_range_batch_device(mof_fft_engine* e, const uint8_t* d_cur, size_t cur_stride,
                                            const uint8_t* d_prev, size_t prev_stride, size_t pitch, int n_pairs,
                                            double* d_out_xy, void* stream) {
  return fft_batch(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, d_out_xy, nullptr, stream, 1, true);
}

/* ---- predicted-shift window offsets (include/mof.h) ----------------------------------------- */

int mof_fft_pred_clamp(const mof_fft_config* cfg, int patch, int32_t px, int32_t py, int32_t* ax, int32_t* ay) {
  if (!cfg || !ax || !ay) return fail(MOF_ERR_BAD_ARG, "mof_fft_pred_clamp: null pointer");
  const mof_fft_config& c = *cfg;
  if (c.grid_x < 1 || c.grid_y < 1 || patch < 0 || patch >= (long)c.grid_x * c.grid_y)
    return fail(MOF_ERR_BAD_ARG, "mof_fft_pred_clamp: patch %d outside the %d x %d grid", patch, c.grid_x, c.grid_y);
  const long x0 = c.origin_x + (long)(patch % c.grid_x) * c.stride_x, y0 = c.origin_y + (long)(patch / c.grid_x) * c.stride_y;
  if (c.patch_size < 1 || c.origin_x < 0 || c.origin_y < 0 || c.stride_x < 0 || c.stride_y < 0 || x0 + c.patch_size > c.frame_width ||
      y0 + c.patch_size > c.frame_height)
    return fail(MOF_ERR_BAD_ARG, "mof_fft_pred_clamp: the patch leaves the frame");
  *ax = mof::pred_clamp_axis(px, (int)x0, c.frame_width, c.patch_size);
  *ay = mof::pred_clamp_axis(py, (int)y0, c.frame_height, c.patch_size);
  return MOF_OK;
}

int mof_fft_pred_from_coarse(double sx, double sy, int32_t* px, int32_t* py) {
  if (!px || !py) return fail(MOF_ERR_BAD_ARG, "mof_fft_pred_from_coarse: null pointer");
  mof::pred_from_coarse(sx, sy, px, py);
  return MOF_OK;
}

// Frame pairs per pass of the window gather: as many as keep the scratch frames under the large-patch pipeline's bound (~1.5 GB), at least one
static int pred_pass_pairs(const mof_fft_engine* e, size_t pitch) {
  const size_t per_pair = (size_t)e->cfg.frame_height * pitch;
  const size_t n = ((size_t)3 << 29) / per_pair;
  return n < 1 ? 1 : (n > 0x7fffffffull ? 0x7fffffff : (int)n);
}

// The window-offset scratch for a call of n_pairs pairs at `pitch` on stream s: the frames of one pass, zero-filled when they are made, and
// the per-pair side buffers. Both by the rules of every engine-owned scratch (grow_scratch), ordered by pred_fence.
static int pred_reserve(mof_fft_engine* e, size_t pitch, int n_pairs, hipStream_t s) {
  const int pass = pred_pass_pairs(e, pitch);
  // (the fused route materialises no window: no displaced frames, the side buffers alone)
  const bool fused = e->pred_route.load() == MOF_PRED_ROUTE_FUSED;
  const size_t want_bytes = fused ? 0 : (size_t)(n_pairs < pass ? n_pairs : pass) * e->cfg.frame_height * pitch;
  const bool pinned = e->graph_pinned.load(), capturing = mof::stream_capturing(s);
  int rc = mof::grow_scratch(pinned, e->pred_fence, {e->stream}, capturing, "the window-offset scratch (bytes of displaced frames)",
                             (long)e->pred_bytes, (long)want_bytes, 0, [e](long bytes) {
                               mof::RelaxedCapture relaxed;
                               e->pred_bytes = 0;
                               e->d_pred_frames.reset();
                               if (bytes == 0) return hipSuccess;
                               if (!e->pred_fence.ev) {
                                 const hipError_t err = e->pred_fence.create();
                                 if (err != hipSuccess) return err;
                               }
                               hipError_t err = e->d_pred_frames.alloc((size_t)bytes);
                               if (err == hipSuccess) err = mof::fill_on(e->stream, e->d_pred_frames, 0, (size_t)bytes);
                               if (err == hipSuccess) e->pred_bytes = (size_t)bytes;
                               return err;
                             });
  if (rc != MOF_OK) return rc;
  return mof::grow_scratch(pinned, e->pred_fence, {e->stream}, capturing, "the window-offset scratch (pairs of predictions)", e->pred_pairs,
                           n_pairs, 0, [e](long pairs) {
                             mof::RelaxedCapture relaxed;
                             e->pred_pairs = 0;
                             if (pairs > 0 && !e->pred_fence.ev) {  // (an engine that only ever ran fused makes the fence here)
                               const hipError_t err = e->pred_fence.create();
                               if (err != hipSuccess) return err;
                             }
                             const size_t n = (size_t)pairs * e->cfg.grid_x * e->cfg.grid_y;
                             const hipError_t err = mof::alloc_all(e->d_pred_xy, 2 * n, e->d_pred_applied, 2 * n, e->d_pred_coarse, 2 * (n / 16 + (size_t)pairs));
                             if (err == hipSuccess) e->pred_pairs = (int)pairs;
                             return err;
                           });
}

// what the window-offset entries share: arguments, then the limits of the feature, each with its own message. *empty: nothing to do.
static int pred_check(const mof_fft_engine* e, const void* d_cur, const void* d_prev, size_t pitch, int n_pairs, const void* d_out_xy,
                      bool* empty, int channels = 1) {
  *empty = false;
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (n_pairs == 0) {
    *empty = true;  // an empty batch carries no pointers to check
    return MOF_OK;
  }
  if (!d_cur || !d_prev || !d_out_xy || n_pairs < 0) return fail(MOF_ERR_BAD_ARG, "bad batch arguments (null pointer or negative count)");
  if (pitch < (size_t)channels * (size_t)e->cfg.frame_width)
    return fail(MOF_ERR_BAD_ARG, "pitch %zu is smaller than the frame width %d (x %d channels)", pitch, e->cfg.frame_width, channels);
  if ((unsigned long long)n_pairs * (unsigned long long)(e->cfg.grid_x * e->cfg.grid_y) > 0x7fffffffull)
    return fail(MOF_ERR_BAD_ARG, "batch too large for one launch");
  const mof_fft_config& c = e->cfg;
  const bool fused = e->pred_route.load() == MOF_PRED_ROUTE_FUSED;  // (only set where the route has the form and the model is cv::phaseCorrelate's)
  if (!fused && channels != 1)
    return fail(MOF_ERR_UNSUPPORTED, "window offsets on BGR8 frames need the fused route (mof_fft_set_pred_route): the gather's scratch "
                "frames are gray");
  if (!fused && ((c.grid_x > 1 && c.stride_x < c.patch_size) || (c.grid_y > 1 && c.stride_y < c.patch_size)))
    return fail(MOF_ERR_UNSUPPORTED, "window offsets need patches that do not overlap (stride >= patch_size on both axes): overlapping "
                "windows cannot share one displaced frame");
  if (c.peak_model != MOF_PEAK_OPENCV) return fail(MOF_ERR_UNSUPPORTED, "window offsets are not defined for peak_model MOF_PEAK_OCL");
  return MOF_OK;
}

// The window-offset pipeline on stream s (busy flag held, device current, pred_check passed). d_pred_xy == nullptr: coarse-to-fine --
// the long-range pass first, the predictions from its shifts. Returns a MOF status.
static int pred_run(mof_fft_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev, size_t prev_stride, size_t pitch,
                    int n_pairs, const int32_t* d_pred_xy, double* d_out_xy, double* d_quality, int32_t* d_applied_xy, double* d_coarse_xy,
                    hipStream_t s, int channels = 1) {
  const bool coarse = d_pred_xy == nullptr;
  const bool fused = e->pred_route.load() == MOF_PRED_ROUTE_FUSED;
  const int patches = e->cfg.grid_x * e->cfg.grid_y;
  const size_t n_patches = (size_t)n_pairs * patches;
  mof::PcArgs a = fft_args(e, d_cur, cur_stride, d_prev, prev_stride, pitch, d_out_xy, d_quality);
  mof::PcArgs lr = a;  // (gray: coarse to fine has no BGR8 form)
  a.channels = channels;
  if (coarse) {
    const int rc = long_range_args(e, &lr);
    if (rc) return rc;
  }
  FIELD_TRY(pred_reserve(e, pitch, n_pairs, s));
  bool own_q = false;
  FIELD_TRY(gate_begin(e, n_patches, s, &a.quality, &own_q));
  if (mof::stream_capturing(s)) e->graph_pinned.store(true);
  HIP_TRY(e->pred_fence.acquire(s));
  if (coarse) {
    // the long-range shifts; armed, the gate acts on them too (their responses pass through the fine pass's quality buffer, which the
    // fine pass then overwrites), and a gated patch -- NaN -- predicts 0
    const size_t n_lr = (size_t)n_pairs * lr.grid_x * lr.grid_y;
    lr.out = d_coarse_xy ? d_coarse_xy : e->d_pred_coarse.get();
    lr.quality = e->min_response > 0.0 ? a.quality : nullptr;
    FIELD_TRY(launch_field(e, lr, n_pairs, s));
    if (lr.quality) HIP_TRY(mof::launch_pc_response_gate(lr.out, lr.quality, n_lr, e->min_response, s));
    HIP_TRY(mof::launch_pc_pred_from_coarse(lr.out, e->d_pred_xy, a.grid_x, a.grid_y, n_pairs, s));
    d_pred_xy = e->d_pred_xy;
  }
  int32_t* applied = d_applied_xy ? d_applied_xy : e->d_pred_applied.get();
  mof::PcOffsetArgs g{};
  g.prev_stride = prev_stride;
  g.pitch = pitch;
  g.frame_w = e->cfg.frame_width;
  g.frame_h = e->cfg.frame_height;
  g.n = e->cfg.patch_size;
  g.grid_x = a.grid_x;
  g.grid_y = a.grid_y;
  g.origin_x = a.origin_x;
  g.origin_y = a.origin_y;
  g.stride_x = a.stride_x;
  g.stride_y = a.stride_y;
  if (fused) {
    // the clamp, then the field kernel on the caller's own previous frames, reading every patch at its applied prediction: no window is
    // materialised, so the whole batch is one pass, and overlapping patches and BGR8 frames are frames like any other
    g.pred = d_pred_xy;
    g.applied = applied;
    HIP_TRY(mof::launch_pc_offset_clamp(g, n_pairs, s));
    mof::PcArgs f = a;
    f.prev_off = applied;
    FIELD_TRY(launch_field(e, f, n_pairs, s));
  } else {
    // the gather: passes of as many pairs as the scratch holds displaced frames for
    const size_t frame = (size_t)e->cfg.frame_height * pitch;
    const int pass = (int)(e->pred_bytes / frame);  // (>= 1: pred_reserve)
    for (int k0 = 0; k0 < n_pairs; k0 += pass) {
      const int np = n_pairs - k0 < pass ? n_pairs - k0 : pass;
      const size_t q0 = (size_t)k0 * patches;
      g.prev = d_prev + (size_t)k0 * prev_stride;
      g.scratch = e->d_pred_frames;
      g.pred = d_pred_xy + 2 * q0;
      g.applied = applied + 2 * q0;
      HIP_TRY(mof::launch_pc_offset_gather(g, np, s));
      mof::PcArgs f = a;
      f.cur = d_cur + (size_t)k0 * cur_stride;
      f.prev = e->d_pred_frames;
      f.prev_stride = frame;
      f.out = a.out + 2 * q0;
      f.quality = a.quality ? a.quality + 2 * q0 : nullptr;
      FIELD_TRY(launch_field(e, f, np, s));
    }
  }
  FIELD_TRY(gate_end(e, a.out, a.quality, n_patches, s, own_q));
  HIP_TRY(mof::launch_pc_offset_finish(a.out, applied, n_patches, a.max_px_speed_sq, s));
  HIP_TRY(e->pred_fence.release(s));
  return MOF_OK;
}

int mof_fft_reserve_pred(mof_fft_engine* e, int n_pairs) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (n_pairs < 0) return fail(MOF_ERR_BAD_ARG, "n_pairs must be >= 0");
  const int patches = e->cfg.grid_x * e->cfg.grid_y;
  if ((unsigned long long)n_pairs * (unsigned long long)patches > 0x7fffffffull) return fail(MOF_ERR_BAD_ARG, "batch too large for one launch");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  if (n_pairs == 0) return MOF_OK;
  HIP_TRY(hipSetDevice(e->cfg.device));
  // everything a window-offset call of n_pairs pairs of dense frames (pitch = frame_width) may have to grow: its own scratch, the
  // large-patch pipeline's for one pass, the gate's buffer where the gate is armed now
  const size_t pitch = (size_t)e->cfg.frame_width;
  FIELD_TRY(pred_reserve(e, pitch, n_pairs, e->stream));
  if (e->route.family == FftRoute::LARGE) {
    const int pass = pred_pass_pairs(e, pitch);
    FIELD_TRY(large_reserve(e, patches, n_pairs < pass ? n_pairs : pass, e->stream));
  }
  double* q = nullptr;
  bool own_q = false;
  return gate_begin(e, (size_t)n_pairs * patches, e->stream, &q, &own_q);
}

static int pred_batch(mof_fft_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev, size_t prev_stride, size_t pitch,
                      int n_pairs, const int32_t* d_pred_xy, double* d_out_xy, double* d_quality, int32_t* d_applied_xy, void* stream,
                      int channels) {
  bool empty = false;
  const int rc = pred_check(e, d_cur, d_prev, pitch, n_pairs, d_out_xy, &empty, channels);
  if (rc != MOF_OK || empty) return rc;
  if (!d_pred_xy) return fail(MOF_ERR_BAD_ARG, "null predictions");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  // (the route pred_check saw cannot have changed: mof_fft_set_pred_route takes the busy flag, and an engine is driven by one thread)
  HIP_TRY(hipSetDevice(e->cfg.device));
  return pred_run(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, d_pred_xy, d_out_xy, d_quality, d_applied_xy, nullptr,
                  (hipStream_t)stream, channels);
}

int mof_fft_process_batch_device_pred(mof_fft_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev, size_t prev_stride,
                                      size_t pitch, int n_pairs, const int32_t* d_pred_xy, double* d_out_xy, double* d_quality,
                                      int32_t* d_applied_xy, void* stream) {
  return pred_batch(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, d_pred_xy, d_out_xy, d_quality, d_applied_xy, stream, 1);
}

int mof_fft_process_batch_device_pred_bgr(mof_fft_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev,
                                          size_t prev_stride, size_t pitch, int n_pairs, const int32_t* d_pred_xy, double* d_out_xy,
                                          double* d_quality, int32_t* d_applied_xy, void* stream) {
  return pred_batch(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, d_pred_xy, d_out_xy, d_quality, d_applied_xy, stream, 3);
}

int mof_fft_pred_route_supported(const mof_fft_config* cfg, int route) {
  if (!cfg || (route != MOF_PRED_ROUTE_GATHER && route != MOF_PRED_ROUTE_FUSED))
    return fail(MOF_ERR_BAD_ARG, "mof_fft_pred_route_supported: null config or unknown route %d", route);
  if (route == MOF_PRED_ROUTE_GATHER) return 1;
  mof::PcPlan plan;
  FftRoute r;
  if (cfg->patch_size < 2 || !mof::fft_route(cfg->patch_size, cfg->peak_model, mof::FftKnobs{}, &plan, &r)) return 0;
  return mof::fft_pred_fused_supported(r, cfg->peak_model) ? 1 : 0;
}

int mof_fft_set_pred_route(mof_fft_engine* e, int route) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (route != MOF_PRED_ROUTE_GATHER && route != MOF_PRED_ROUTE_FUSED)
    return fail(MOF_ERR_BAD_ARG, "route must be MOF_PRED_ROUTE_GATHER or MOF_PRED_ROUTE_FUSED");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  // a captured graph holds the kernels of the route it was captured on: its replays would not follow (the rule of mof_fft_set_min_response)
  if (e->graph_pinned.load()) return fail(MOF_ERR_BUSY, "the route is baked into a captured graph: mof_fft_release_graphs first");
  if (route == MOF_PRED_ROUTE_FUSED && !mof::fft_pred_fused_supported(e->route, e->cfg.peak_model))
    return fail(MOF_ERR_UNSUPPORTED, "the fused route exists on K1 (patch sizes 32, 64, 128) and the half-tile kernel under "
                "cv::phaseCorrelate's peak model; this engine runs '%s'", e->route.variant);
  e->pred_route = route;  // (frees nothing: the gather's scratch stays for the way back)
  return MOF_OK;
}

int mof_fft_pred_route(const mof_fft_engine* e) { return e ? e->pred_route.load() : MOF_PRED_ROUTE_GATHER; }

int mof_fft_process_coarse_to_fine_batch_device(mof_fft_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev,
                                                size_t prev_stride, size_t pitch, int n_pairs, double* d_out_xy, double* d_quality,
                                                int32_t* d_applied_xy, double* d_coarse_xy, void* stream) {
  bool empty = false;
  int rc = pred_check(e, d_cur, d_prev, pitch, n_pairs, d_out_xy, &empty);
  if (rc != MOF_OK || empty) return rc;
  mof::PcArgs lr{};
  rc = long_range_args(e, &lr);  // (coarse-to-fine off the reference tiling: MOF_ERR_UNSUPPORTED, before anything is enqueued)
  if (rc) return rc;
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return pred_run(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, nullptr, d_out_xy, d_quality, d_applied_xy, d_coarse_xy,
                  (hipStream_t)stream);
}

// processImage's frame chain around the coarse-to-fine pipeline: the first frame against itself, previous <- current always
int mof_fft_process_coarse_to_fine(mof_fft_engine* e, const uint8_t* frame, size_t pitch, double* out_xy, double* quality, int* n_invalid) {
  bool empty = false;
  int rc = pred_check(e, frame, frame, pitch, 1, out_xy, &empty);
  if (rc != MOF_OK) return rc;
  mof::PcArgs lr{};
  rc = long_range_args(e, &lr);
  if (rc) return rc;
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int cur_slot = 1 - e->prev_slot;
  HIP_TRY(upload_frame(e, cur_slot, frame, pitch));
  const uint8_t* prev = e->first ? e->d_frames[cur_slot] : e->d_frames[e->prev_slot];
  FIELD_TRY(pred_run(e, e->d_frames[cur_slot], 0, prev, 0, (size_t)e->cfg.frame_width, 1, nullptr, e->d_out, quality ? e->d_quality.get() : nullptr,
                     nullptr, nullptr, e->stream));
  const size_t res = (size_t)e->cfg.grid_x * e->cfg.grid_y * 2;
  HIP_TRY(hipMemcpyAsync(e->h_out, e->d_out, res * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (quality) HIP_TRY(hipMemcpyAsync(e->h_quality, e->d_quality, res * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (quality) std::memcpy(quality, e->h_quality, res * sizeof(double));
  int bad = 0;
  for (size_t i = 0; i < res; i += 2) {
    out_xy[i] = e->h_out[i];
    out_xy[i + 1] = e->h_out[i + 1];
    if (std::isnan(e->h_out[i])) ++bad;
  }
  if (n_invalid) *n_invalid = bad;
  e->prev_slot = cur_slot;
  e->first = false;
  return MOF_OK;
}

// A video: pair k = (frame k + 1, frame k), in the route's video form (fft_route); the pair form runs the engine's pair kernels on
// cur = frames + 1, prev = frames (no copy either).
static int fft_sequence(mof_fft_engine* e, const uint8_t* d_frames, size_t frame_stride, size_t pitch, int n_frames,
                        double* d_out_xy, double* d_quality, void* stream, int channels) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (n_frames == 0 || n_frames == 1) return MOF_OK;  // no pair
  if (!d_frames || !d_out_xy || n_frames < 0 || pitch < (size_t)channels * (size_t)e->cfg.frame_width)
    return fail(MOF_ERR_BAD_ARG, "bad sequence arguments");
  const int n_pairs = n_frames - 1;
  if ((unsigned long long)n_pairs * (unsigned long long)(e->cfg.grid_x * e->cfg.grid_y) > 0x7fffffffull)
    return fail(MOF_ERR_BAD_ARG, "sequence too long for one launch");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  mof::PcArgs a = fft_args(e, d_frames + frame_stride, frame_stride, d_frames, frame_stride, pitch, d_out_xy, d_quality);
  a.channels = channels;
  const size_t n_patches = (size_t)n_pairs * a.grid_x * a.grid_y;
  bool own_q = false;
  FIELD_TRY(gate_begin(e, n_patches, (hipStream_t)stream, &a.quality, &own_q));
  d_quality = a.quality;
  if (mof::stream_capturing((hipStream_t)stream)) e->graph_pinned.store(true);
  const FftRoute& r = e->route;
  if (r.video == FftRoute::PAIRS) {
    FIELD_TRY(launch_field(e, a, n_pairs, (hipStream_t)stream));
    return gate_end(e, a.out, a.quality, n_patches, (hipStream_t)stream, own_q);
  }
  // pairs a workgroup walks in time (MOF_FFT_SEQ_RUN; 0: the launchers pick the run length; pc_seq_half.hip takes 16)
  const int run_knob = r.seq_run;
  // the run index rides gridDim.z (at most 65535 per launch): a very long video goes out in several launches
  const size_t per_pair = (size_t)e->cfg.grid_x * e->cfg.grid_y * 2;
  const int max_pairs = 65535 * (run_knob ? run_knob : r.min_run);
  for (int k0 = 0; k0 < n_pairs; k0 += max_pairs) {
    const int nk = n_pairs - k0 < max_pairs ? n_pairs - k0 : max_pairs;
    mof::PcArgs c = a;
    c.cur = d_frames + (size_t)k0 * frame_stride;  // the sequence kernels index frames, not pairs
    c.out = d_out_xy + (size_t)k0 * per_pair;
    c.quality = d_quality ? d_quality + (size_t)k0 * per_pair : nullptr;
    if (r.video == FftRoute::HALF_SEQ) HIP_TRY(mof::launch_pc_half_sequence(c, r.video_m, e->cfg.patch_size, nk, run_knob, (hipStream_t)stream));
    else if (r.video == FftRoute::SEQ_HALF) HIP_TRY(mof::launch_pc_sequence_half(c, e->cfg.patch_size, nk, run_knob ? run_knob : 16, (hipStream_t)stream));
    else HIP_TRY(mof::launch_pc_sequence(c, nk, run_knob, (hipStream_t)stream));
  }
  return gate_end(e, a.out, a.quality, n_patches, (hipStream_t)stream, own_q);
}

int mof_fft_process_sequence_device(mof_fft_engine* e, const uint8_t* d_frames, size_t frame_stride, size_t pitch, int n_frames,
                                    double* d_out_xy, void* stream) {
  return fft_sequence(e, d_frames, frame_stride, pitch, n_frames, d_out_xy, nullptr, stream, 1);
}

int mof_fft_process_sequence_device_q(mof_fft_engine* e, const uint8_t* d_frames, size_t frame_stride, size_t pitch, int n_frames,
                                      int channels, double* d_out_xy, double* d_quality, void* stream) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (channels != 1 && channels != 3) return fail(MOF_ERR_BAD_ARG, "channels must be 1 or 3");
  return fft_sequence(e, d_frames, frame_stride, pitch, n_frames, d_out_xy, d_quality, stream, channels);
}

int mof_fft_process_sequence_device_bgr(mof_fft_engine* e, const uint8_t* d_frames, size_t frame_stride, size_t pitch, int n_frames,
                                        double* d_out_xy, void* stream) {
  return fft_sequence(e, d_frames, frame_stride, pitch, n_frames, d_out_xy, nullptr, stream, 3);
}

int mof_fft_process_batch_host(mof_fft_engine* e, const uint8_t* cur, size_t cur_stride, const uint8_t* prev,
                               size_t prev_stride, size_t pitch, int n_pairs, double* out_xy) {
  return mof_fft_process_batch_host_q(e, cur, cur_stride, prev, prev_stride, pitch, n_pairs, out_xy, nullptr);
}

int mof_fft_process_batch_host_q(mof_fft_engine* e, const uint8_t* cur, size_t cur_stride, const uint8_t* prev, size_t prev_stride,
                                 size_t pitch, int n_pairs, double* out_xy, double* quality) try {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (n_pairs == 0) return MOF_OK;  // an empty batch carries no pointers to check
  if (!cur || !prev || !out_xy || n_pairs < 0 || pitch < (size_t)e->cfg.frame_width)
    return fail(MOF_ERR_BAD_ARG, "bad batch arguments");
  HIP_TRY(hipSetDevice(e->cfg.device));
  mof::RelaxedCapture relaxed;  // the pipeline's first-call allocations must not disturb a capture on another thread
  const size_t res = (size_t)e->cfg.grid_x * e->cfg.grid_y * 2 * sizeof(double);
  {
    std::lock_guard<std::mutex> lock(e->host_mu);
    if (!e->host_pipe) e->host_pipe.reset(new mof::HostPipe(e->frame_bytes, &res, 1));
    const size_t res2[2] = {res, res};
    if (quality && !e->host_pipe_q) e->host_pipe_q.reset(new mof::HostPipe(e->frame_bytes, res2, 2));
  }
  const mof::HostPipe::Out out[2] = {{out_xy, res}, {quality, res}};
  mof::HostPipe* pipe = (quality ? e->host_pipe_q : e->host_pipe).get();
  hipError_t he = hipSuccess;
  // chunks of frames go up on the pipe's copy stream while the engine's stream runs the previous chunk through the DEVICE batch entry
  // (its kernels, its bits); a video -- cur = prev + one frame -- arrives as the two views of ONE uploaded run
  const int rc = pipe->process(
      cur, cur_stride, prev, prev_stride, pitch, e->cfg.frame_width, e->cfg.frame_height, n_pairs, out, e->stream,
      [e, quality](const mof::HostPipe::Chunk& c, hipStream_t s) {
        return fft_batch(e, c.d_cur, c.stride, c.d_prev, c.stride, (size_t)e->cfg.frame_width, c.count, static_cast<double*>(c.d_out[0]),
                         quality ? static_cast<double*>(c.d_out[1]) : nullptr, s, 1, false);
      },
      &he);
  if (rc == -1) return fail(MOF_ERR_HIP, "host batch pipeline: %s", hipGetErrorString(he));
  return rc;
} catch (const std::bad_alloc&) {
  return fail(MOF_ERR_NO_MEMORY, "mof_fft_process_batch_host: out of host memory");
}

/* Pinned host memory for callers that do not link HIP themselves: frames handed to the *_batch_host entries from such memory are DMA'd
 * from where they lie (host_pipe.hpp). */
int mof_host_alloc(size_t bytes, void** out) {
  if (!out || bytes == 0) return fail(MOF_ERR_BAD_ARG, "mof_host_alloc: null result pointer or zero bytes");
  *out = nullptr;
  HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
  return MOF_OK;
}
int mof_host_free(void* p) {
  if (!p) return MOF_OK;
  HIP_TRY(hipHostFree(p));
  return MOF_OK;
}
int mof_host_register(void* p, size_t bytes) {
  if (!p || bytes == 0) return fail(MOF_ERR_BAD_ARG, "mof_host_register: null pointer or zero bytes");
  HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
  return MOF_OK;
}
int mof_host_unregister(void* p) {
  if (!p) return fail(MOF_ERR_BAD_ARG, "mof_host_unregister: null pointer");
  HIP_TRY(hipHostUnregister(p));
  return MOF_OK;
}

int mof_fft_sync(mof_fft_engine* e) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MOF_OK;
}

/* ------------------------------------------------------------------------------------------ */
/* Block matching                                                                             */
/* ------------------------------------------------------------------------------------------ */

int mof_bm_config_block_method(mof_bm_config* cfg, int frame_size, int sample_point_size, int scan_radius) {
  if (!cfg || frame_size < 1 || sample_point_size < 1 || scan_radius < 0)
    return fail(MOF_ERR_BAD_ARG, "bad BlockMethod geometry");
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->frame_width = cfg->frame_height = frame_size;
  cfg->block_size = sample_point_size;
  cfg->step_size = 0;
  cfg->scan_radius = scan_radius;
  cfg->grid_x = cfg->grid_y = (frame_size - scan_radius * 2) / sample_point_size;  // BlockMethod.cpp:11
  cfg->low_contrast_rule = 0;
  return MOF_OK;
}

int mof_bm_config_fast_spaced(mof_bm_config* cfg, int width, int height, int sample_point_size, int step_size,
                              int scan_radius) {
  if (!cfg || width < 1 || height < 1 || sample_point_size < 1 || step_size < 0 || scan_radius < 0)
    return fail(MOF_ERR_BAD_ARG, "bad FastSpacedBM geometry");
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->frame_width = width;
  cfg->frame_height = height;
  cfg->block_size = sample_point_size;
  cfg->step_size = step_size;
  cfg->scan_radius = scan_radius;
  const int S = sample_point_size + step_size;            // FastSpacedBMMethod_OCL.cpp:82-83
  cfg->grid_x = (width - scan_radius * 2) / S;            // :90
  cfg->grid_y = (height - scan_radius * 2) / S;
  cfg->low_contrast_rule = 1;
  return MOF_OK;
}

static int validate_bm(const mof_bm_config* c) {
  if (!c) return fail(MOF_ERR_BAD_ARG, "null config");
  if (c->frame_width < 1 || c->frame_height < 1 || c->grid_x < 1 || c->grid_y < 1 || c->step_size < 0)
    return fail(MOF_ERR_BAD_ARG, "bad block-matching geometry");
  if (!mof::bm_config_supported(c->block_size, c->scan_radius))
    return fail(MOF_ERR_UNSUPPORTED, "block_size %d / scan_radius %d not supported by the HIP kernel "
                "(block multiple of 4 in 4..128, radius 1..48, window within the LDS)", c->block_size, c->scan_radius);
  const long S = c->block_size + c->step_size;
  if ((c->grid_x - 1) * S + c->block_size + 2 * c->scan_radius > c->frame_width ||
      (c->grid_y - 1) * S + c->block_size + 2 * c->scan_radius > c->frame_height)
    return fail(MOF_ERR_BAD_ARG, "block grid leaves the frame");
  return MOF_OK;
}

static mof::BmArgs bm_args(const mof_bm_engine* e, const uint8_t* cur, size_t cs, const uint8_t* prev, size_t ps,
                           size_t pitch, int8_t* dx, int8_t* dy, int8_t* mode, int channels = 1) {
  mof::BmArgs a{};
  a.channels = channels;
  a.cur = cur;
  a.prev = prev;
  a.cur_stride = cs;
  a.prev_stride = ps;
  a.pitch = pitch;
  a.grid_x = e->cfg.grid_x;
  a.grid_y = e->cfg.grid_y;
  a.block = e->cfg.block_size;
  a.step = e->cfg.step_size;
  a.radius = e->cfg.scan_radius;
  a.low_contrast_rule = e->cfg.low_contrast_rule;
  a.dx = dx;
  a.dy = dy;
  a.mode = mode;
  return a;
}

static void bm_destroy_now(void* p) {
  mof_bm_engine* e = static_cast<mof_bm_engine*>(p);
  mof::RelaxedCapture relaxed;
  (void)hipSetDevice(e->cfg.device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  delete e;
}
struct BmDestroyNow {
  void operator()(mof_bm_engine* e) const { bm_destroy_now(e); }
};

int mof_bm_create(const mof_bm_config* cfg, mof_bm_engine** out) {
  if (!out) return fail(MOF_ERR_BAD_ARG, "null out");
  *out = nullptr;
  int rc = validate_bm(cfg);
  if (rc) return rc;
  rc = mof::select_device(cfg->device);
  if (rc) return rc;
  mof::RelaxedCapture relaxed;
  std::unique_ptr<mof_bm_engine, BmDestroyNow> e(new (std::nothrow) mof_bm_engine());
  if (!e) return fail(MOF_ERR_NO_MEMORY, "out of host memory");
  e->cfg = *cfg;
  if (!mof::bm_route(cfg->block_size, cfg->step_size, cfg->scan_radius, cfg->grid_x, mof::bm_knobs(), &e->route))
    return fail(MOF_ERR_UNSUPPORTED, "block_size %d / scan_radius %d: no scan plan", cfg->block_size, cfg->scan_radius);
  e->frame_bytes = (size_t)cfg->frame_width * cfg->frame_height;
  const size_t nb = (size_t)cfg->grid_x * cfg->grid_y;
  HIP_TRY(e->stream.create());
  for (auto& frame : e->d_frames) {
    HIP_TRY(frame.alloc(e->frame_bytes));
    HIP_TRY(mof::fill_on(e->stream, frame, 0, e->frame_bytes));  // imPrev = Scalar(0), BlockMethod.cpp:17-18
  }
  HIP_TRY(mof::alloc_all(e->d_dx, nb, e->d_dy, nb, e->d_mode, 8, e->h_res, 2 * nb + 8, e->h_stage, e->frame_bytes));
  *out = e.release();
  return MOF_OK;
}

void mof_bm_destroy(mof_bm_engine* e) {
  if (!e) return;
  if (e->graph_pinned.load()) {
    mof::park_engine(&bm_destroy_now, e);
    return;
  }
  bm_destroy_now(e);
}

int mof_bm_release_graphs(mof_bm_engine* e) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  e->graph_pinned.store(false);
  return MOF_OK;
}

int mof_bm_graph_pinned(const mof_bm_engine* e) { return e && e->graph_pinned.load() ? 1 : 0; }

int mof_bm_set_prev(mof_bm_engine* e, const uint8_t* frame, size_t pitch) { return set_prev(e, frame, pitch); }

int mof_bm_reset(mof_bm_engine* e) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipMemsetAsync(e->d_frames[e->prev_slot], 0, e->frame_bytes, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MOF_OK;
}

static mof::BmQArgs bm_qargs(const mof_bm_engine* e, uint32_t* quality) {
  mof::BmQArgs q;
  q.quality = quality;
  q.max_min_sad = e->max_min_sad;
  q.min_sad_range = e->min_sad_range;
  return q;
}

int mof_bm_set_gate(mof_bm_engine* e, uint32_t max_min_sad, uint32_t min_sad_range) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  e->max_min_sad = max_min_sad;
  e->min_sad_range = min_sad_range;
  return MOF_OK;
}

int mof_bm_gate(const mof_bm_engine* e, uint32_t* max_min_sad, uint32_t* min_sad_range) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (max_min_sad) *max_min_sad = e->max_min_sad;
  if (min_sad_range) *min_sad_range = e->min_sad_range;
  return MOF_OK;
}

int mof_bm_scan_plan(int block_size, int step_size, int scan_radius, int grid_x, int quality, int* out4) {
  if (!out4 || grid_x < 0 || step_size < 0 || !mof::bm_config_supported(block_size, scan_radius))
    return fail(MOF_ERR_BAD_ARG, "mof_bm_scan_plan: unsupported geometry or null output");
  return mof::bm_scan_plan(block_size, step_size, scan_radius, grid_x, quality != 0, out4) ? MOF_OK : fail(MOF_ERR_UNSUPPORTED, "no plan");
}

int mof_bm_process_q(mof_bm_engine* e, const uint8_t* frame, size_t pitch, int8_t* dx, int8_t* dy, int8_t* mode_xy, uint32_t* quality,
                     int* n_invalid) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (!frame || !dx || !dy || pitch < (size_t)e->cfg.frame_width) return fail(MOF_ERR_BAD_ARG, "bad arguments");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int cur_slot = 1 - e->prev_slot;
  const size_t nb = (size_t)e->cfg.grid_x * e->cfg.grid_y;
  const bool want_q = quality || n_invalid;
  if (want_q && !e->d_q) {
    mof::RelaxedCapture relaxed;
    HIP_TRY(mof::alloc_all(e->h_q, 3 * nb + 1, e->d_q, 3 * nb + 1));  // (d_q, the test above, last)
  }
  HIP_TRY(upload_frame(e, cur_slot, frame, pitch));
  mof::BmArgs a = bm_args(e, e->d_frames[cur_slot], 0, e->d_frames[e->prev_slot], 0, (size_t)e->cfg.frame_width,
                          e->d_dx, e->d_dy, e->d_mode);
  const mof::BmQArgs q = bm_qargs(e, quality ? e->d_q.get() : nullptr);
  HIP_TRY(mof::launch_bm_scan(a, q, e->route, 1, e->stream));
  HIP_TRY(mof::launch_bm_mode(a, q, n_invalid ? reinterpret_cast<int32_t*>(e->d_q + 3 * nb) : nullptr, 1, e->stream));
  HIP_TRY(hipMemcpyAsync(e->h_res, e->d_dx, nb, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(e->h_res + nb, e->d_dy, nb, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(e->h_res + 2 * nb, e->d_mode, 8, hipMemcpyDeviceToHost, e->stream));
  if (quality) HIP_TRY(hipMemcpyAsync(e->h_q, e->d_q, 3 * nb * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  if (n_invalid) HIP_TRY(hipMemcpyAsync(e->h_q + 3 * nb, e->d_q + 3 * nb, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  std::memcpy(dx, e->h_res, nb);
  std::memcpy(dy, e->h_res + nb, nb);
  if (quality) std::memcpy(quality, e->h_q, 3 * nb * sizeof(uint32_t));
  if (n_invalid) *n_invalid = (int)e->h_q[3 * nb];
  if (mode_xy) {
    mode_xy[0] = e->h_res[2 * nb];
    mode_xy[1] = e->h_res[2 * nb + 1];
  }
  e->prev_slot = cur_slot;  // imPrev = imCurr.clone(), BlockMethod.cpp:89
  e->have_pair = true;
  return MOF_OK;
}

int mof_bm_process(mof_bm_engine* e, const uint8_t* frame, size_t pitch, int8_t* dx, int8_t* dy, int8_t* mode_xy) {
  return mof_bm_process_q(e, frame, pitch, dx, dy, mode_xy, nullptr, nullptr);
}

int mof_bm_refine(mof_bm_engine* e, int fullpix_x, int fullpix_y, int passes, int faithful, double* out_xy) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (!out_xy || passes < 1 || passes > 4) return fail(MOF_ERR_BAD_ARG, "bad refine arguments");
  if (!e->have_pair) return fail(MOF_ERR_NOT_INIT, "mof_bm_refine needs a preceding mof_bm_process call");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int w = e->cfg.frame_width, h = e->cfg.frame_height, W2 = 2 * w, H2 = 2 * h;
  if (!e->d_up[0]) {
    mof::RelaxedCapture relaxed;
    HIP_TRY(mof::alloc_all(e->d_up[1], (size_t)W2 * H2, e->d_sad9, 9, e->h_sad9, 9, e->d_up[0], (size_t)W2 * H2));  // (d_up[0], the test above, last)
  }
  // after mof_bm_process the frame just processed sits in the "previous" slot, its predecessor in the other one
  const uint8_t* cur = e->d_frames[e->prev_slot];
  const uint8_t* prev = e->d_frames[1 - e->prev_slot];
  int tx = fullpix_x, ty = fullpix_y, scale = 1;
  for (int i = 1; i <= passes; ++i) {
    scale *= 2;
    tx *= 2;
    ty *= 2;  // BlockMethod.cpp:106-107
    if (i == 1) {
      // :110-111 -- both images go to twice the ORIGINAL size; the reference resizes the "previous" one from the
      // CURRENT image. Later passes resize to the same 2x size, i.e. copy.
      HIP_TRY(mof::launch_bm_resize2x(cur, (size_t)w, w, h, e->d_up[0], e->stream));
      HIP_TRY(mof::launch_bm_resize2x(faithful ? cur : prev, (size_t)w, w, h, e->d_up[1], e->stream));
    }
    int spx, spy;  // :113-121
    if (tx < 0 && ty < 0) { spx = -tx + 1; spy = -ty + 1; }
    else if (tx < 0 && ty >= 0) { spx = -tx + 1; spy = 1; }
    else if (tx >= 0 && ty < 0) { spx = 1; spy = -ty + 1; }
    else { spx = 1; spy = 1; }
    const int cw = W2 - ((tx < 0 ? -tx : tx) + 2), ch = H2 - ((ty < 0 ? -ty : ty) + 2);  // :123
    if (cw <= 0 || ch <= 0) return fail(MOF_ERR_BAD_ARG, "refine: offset (%d, %d) leaves no cut-out", tx, ty);
    HIP_TRY(hipMemsetAsync(e->d_sad9, 0, 9 * sizeof(unsigned long long), e->stream));
    HIP_TRY(mof::launch_bm_refine_sad(e->d_up[0], e->d_up[1], W2, spx, spy, cw, ch, e->d_sad9, e->stream));
    HIP_TRY(hipMemcpyAsync(e->h_sad9, e->d_sad9, 9 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    int best = 0;  // cv::minMaxLoc: first minimum, row-major over (m, n)  (:140)
    for (int k = 1; k < 9; ++k)
      if ((int)e->h_sad9[k] < (int)e->h_sad9[best]) best = k;  // absDiffsMatSubpix is CV_32S
    tx += best % 3 - 1;
    ty += best / 3 - 1;  // :142
  }
  out_xy[0] = (double)((float)tx / (float)scale);  // :144
  out_xy[1] = (double)((float)ty / (float)scale);
  return MOF_OK;
}

// The device batch entries: n_pairs frame pairs of `channels` interleaved channels (1 gray, 3 BGR8)
static int bm_batch(mof_bm_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev, size_t prev_stride, size_t pitch,
                    int n_pairs, int8_t* d_dx, int8_t* d_dy, int8_t* d_mode, uint32_t* d_quality, int32_t* d_n_invalid, void* stream,
                    int channels) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (n_pairs == 0) return MOF_OK;  // an empty batch carries no pointers to check
  if (!d_cur || !d_prev || !d_dx || !d_dy || !d_mode || n_pairs < 0 || pitch < (size_t)channels * (size_t)e->cfg.frame_width)
    return fail(MOF_ERR_BAD_ARG, "bad batch arguments");
  if ((unsigned long long)n_pairs * (unsigned long long)(e->cfg.grid_x * e->cfg.grid_y) > 0x7fffffffull)
    return fail(MOF_ERR_BAD_ARG, "batch too large for one launch");
  BusyGuard g(e->busy);
  if (!g.owned) return fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  hipStream_t s = (hipStream_t)stream;  // (a captured block-matching batch reads no engine-owned memory: no pin)
  mof::BmArgs a = bm_args(e, d_cur, cur_stride, d_prev, prev_stride, pitch, d_dx, d_dy, d_mode, channels);
  const mof::BmQArgs q = bm_qargs(e, d_quality);
  HIP_TRY(mof::launch_bm_scan(a, q, e->route, n_pairs, s));
  HIP_TRY(mof::launch_bm_mode(a, q, d_n_invalid, n_pairs, s));
  return MOF_OK;
}

int mof_bm_process_batch_device_q(mof_bm_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev, size_t prev_stride,
                                  size_t pitch, int n_pairs, int8_t* d_dx, int8_t* d_dy, int8_t* d_mode, uint32_t* d_quality,
                                  int32_t* d_n_invalid, void* stream) {
  return bm_batch(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, d_dx, d_dy, d_mode, d_quality, d_n_invalid, stream, 1);
}

int mof_bm_process_batch_device_bgr_q(mof_bm_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev, size_t prev_stride,
                                      size_t pitch, int n_pairs, int8_t* d_dx, int8_t* d_dy, int8_t* d_mode, uint32_t* d_quality,
                                      int32_t* d_n_invalid, void* stream) {
  return bm_batch(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, d_dx, d_dy, d_mode, d_quality, d_n_invalid, stream, 3);
}

int mof_bm_process_batch_device(mof_bm_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev,
                                size_t prev_stride, size_t pitch, int n_pairs, int8_t* d_dx, int8_t* d_dy,
                                int8_t* d_mode, void* stream) {
  return bm_batch(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, d_dx, d_dy, d_mode, nullptr, nullptr, stream, 1);
}

int mof_bm_process_batch_device_bgr(mof_bm_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev,
                                    size_t prev_stride, size_t pitch, int n_pairs, int8_t* d_dx, int8_t* d_dy,
                                    int8_t* d_mode, void* stream) {
  return bm_batch(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, d_dx, d_dy, d_mode, nullptr, nullptr, stream, 3);
}

// (the _q pipe's slots carry all five outputs; one the caller did not ask for is neither computed nor read back)
int mof_bm_process_batch_host_q(mof_bm_engine* e, const uint8_t* cur, size_t cur_stride, const uint8_t* prev, size_t prev_stride,
                                size_t pitch, int n_pairs, int8_t* dx, int8_t* dy, int8_t* mode, uint32_t* quality, int32_t* n_invalid) try {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  if (n_pairs == 0) return MOF_OK;  // an empty batch carries no pointers to check
  if (!cur || !prev || !dx || !dy || !mode || n_pairs < 0 || pitch < (size_t)e->cfg.frame_width)
    return fail(MOF_ERR_BAD_ARG, "bad batch arguments");
  HIP_TRY(hipSetDevice(e->cfg.device));
  mof::RelaxedCapture relaxed;
  const size_t nb = (size_t)e->cfg.grid_x * e->cfg.grid_y;
  const size_t bpp[5] = {nb, nb, 8, 3 * nb * sizeof(uint32_t), sizeof(int32_t)};
  {
    std::lock_guard<std::mutex> lock(e->host_mu);
    if (!e->host_pipe) e->host_pipe.reset(new mof::HostPipe(e->frame_bytes, bpp, 3));
    if ((quality || n_invalid) && !e->host_pipe_q) e->host_pipe_q.reset(new mof::HostPipe(e->frame_bytes, bpp, 5));
  }
  mof::HostPipe* pipe = (quality || n_invalid ? e->host_pipe_q : e->host_pipe).get();
  const mof::HostPipe::Out outs[5] = {{dx, nb}, {dy, nb}, {mode, 8}, {quality, bpp[3]}, {n_invalid, bpp[4]}};
  hipError_t he = hipSuccess;
  const int rc = pipe->process(
      cur, cur_stride, prev, prev_stride, pitch, e->cfg.frame_width, e->cfg.frame_height, n_pairs, outs, e->stream,
      [e, quality, n_invalid](const mof::HostPipe::Chunk& c, hipStream_t s) {
        return mof_bm_process_batch_device_q(e, c.d_cur, c.stride, c.d_prev, c.stride, (size_t)e->cfg.frame_width, c.count,
                                             static_cast<int8_t*>(c.d_out[0]), static_cast<int8_t*>(c.d_out[1]), static_cast<int8_t*>(c.d_out[2]),
                                             quality ? static_cast<uint32_t*>(c.d_out[3]) : nullptr,
                                             n_invalid ? static_cast<int32_t*>(c.d_out[4]) : nullptr, s);
      },
      &he);
  if (rc == -1) return fail(MOF_ERR_HIP, "host batch pipeline: %s", hipGetErrorString(he));
  return rc;
} catch (const std::bad_alloc&) {
  return fail(MOF_ERR_NO_MEMORY, "mof_bm_process_batch_host: out of host memory");
}

int mof_bm_process_batch_host(mof_bm_engine* e, const uint8_t* cur, size_t cur_stride, const uint8_t* prev,
                              size_t prev_stride, size_t pitch, int n_pairs, int8_t* dx, int8_t* dy, int8_t* mode) {
  return mof_bm_process_batch_host_q(e, cur, cur_stride, prev, prev_stride, pitch, n_pairs, dx, dy, mode, nullptr, nullptr);
}

int mof_bm_sync(mof_bm_engine* e) {
  if (!e) return fail(MOF_ERR_NOT_INIT, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MOF_OK;
}

}  // extern "C"
