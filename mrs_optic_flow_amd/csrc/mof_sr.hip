// mof_sr.hip -- host side of the scale/rotation estimator behind the C ABI (mof_sr_* in include/mof.h).
//
// Mirrors scaleRotationEstimator (/root/reference/src/scaleRotationEstimator.cpp:3-32 ctor, :34-148
// processImage): state = the persistent log-polar image `tempIm` (:27), the previous log-polar image
// `prevIm_F32` (:48, :128) and `first` (:31). What cv::logPolar / cv::remap would compute on the host for
// every frame -- the float maps, their 1/32-px fixed-point form and the 2^15-scaled kernel tables -- depends
// only on (resolution, M), so it is built ONCE here and kept on the device; per frame the GPU does one gather
// (K4) and the whole-frame phase correlation (K5..K8). No CPU compute path.

#include <hip/hip_runtime.h>

#include <atomic>
#include <cfloat>
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
#include "mof.h"
#include "mof_kernels.h"
#include "pc_launch.hpp"

namespace {

constexpr int kTab = 32;            // INTER_TAB_SIZE
constexpr int kCoefScale = 1 << 15; // INTER_REMAP_COEF_SCALE
// frame pairs per pipeline pass: 512 pairs of 480^2 = 1.9 GB of scratch (log-polar images, Zt, Dt). Same-box sweeps at c5
// (tools/sweep_c5.sh, profiles/r02_c5_sweep.txt): 64 / 128 / 256 pairs -> 240 / 277 / 308 k pairs/s on one lane, 512 ->
// 326 k, 1024 -> 324 k; with the second lane 254 / 283 / 312 / 318 / 313 k -- once a pass is long enough to fill the
// chip the two-lane overlap has nothing left to hide, so one lane is the default. r03 (frame kernels, non-temporal streams;
// tools/ab_sr_chunk.sh): 256 / 512 / 1024 pairs -> 341 / 360 / 366 k (c5) and 424 / 518 / 535 k (c5seq); passes that fit the
// 256 MB Infinity Cache (64 pairs: Zt 118 MB + Dt 59 MB) are no faster per byte and pay the launch gaps (248 k). 1024-pair
// passes are worth +1.7 % at c5 and cost 3.8 GB of scratch that stays allocated (and pinned once a graph captured the engine),
// so the DEFAULT stays 512 pairs = 1.9 GB (r04, advisor); a caller that has the memory opts in through
// mof_sr_config.batch_chunk (bench.py does for c5 / c5seq).
constexpr int kChunkDefault = 512;
// The MOF_SR_* knobs of the engine (README), read once per process. MOF_SR_CHUNK / MOF_SR_OVERLAP override mof_sr_config.batch_chunk /
// .pipeline_lanes at create() (sweeps)
const mof::SrKnobs& sr_knobs() {
  static const mof::SrKnobs k = [] {
    mof::SrKnobs r;
    const char* v;
    r.tuned_all = !(v = getenv("MOF_SR_TUNED_ALL")) || atoi(v) != 0;
    r.verbose = (v = getenv("MOF_SR_VERBOSE")) && atoi(v) != 0;
    if ((v = getenv("MOF_SR_SEQ_RUN")) && atoi(v) >= 1 && atoi(v) <= 4096) r.seq_run = atoi(v);
    if ((v = getenv("MOF_SR_CHUNK"))) r.chunk = atoi(v) >= 1 && atoi(v) <= 4096 ? atoi(v) : kChunkDefault;
    if ((v = getenv("MOF_SR_OVERLAP"))) r.overlap = atoi(v) != 0;
    r.lp_global = (v = getenv("MOF_SR_LP_GLOBAL")) && atoi(v) != 0;
    r.lp_staged = !(v = getenv("MOF_SR_LP_STAGED")) || atoi(v) != 0;
    r.lp_super = !((v = getenv("MOF_SR_LP_SUPER")) && atoi(v) == 0);
    r.lp_xcd = !((v = getenv("MOF_SR_LP_XCD")) && atoi(v) == 0);
    r.lp_long_ring = (v = getenv("MOF_SR_LP_RING")) && atoi(v) == 16;
    if ((v = getenv("MOF_SR_LP_IPW"))) r.lp_ipw = atoi(v);
    return r;
  }();
  return k;
}
int chunk_pairs(int cfg_chunk) {
  if (sr_knobs().chunk) return sr_knobs().chunk;
  return cfg_chunk >= 1 && cfg_chunk <= 4096 ? cfg_chunk : kChunkDefault;
}
bool two_lane_default(int cfg_lanes) { return sr_knobs().overlap >= 0 ? sr_knobs().overlap != 0 : cfg_lanes == 2; }

void kernel_1d(int ksize, float x, float* c) {
  if (ksize == 4) {  // bicubic, A = -0.75
    const float A = -0.75f;
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
    return;
  }
  // Lanczos4: sin(pi x) sin(pi x / 4) / (pi^2 x^2 / 4) evaluated through the angle-sum table OpenCV uses
  static const double s45 = 0.70710678118654752440084436210485;
  static const double cs[8][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
  if (x < FLT_EPSILON) {
    for (int i = 0; i < 8; ++i) c[i] = 0.f;
    c[3] = 1.f;
    return;
  }
  float sum = 0.f;
  const double y0 = -(x + 3) * 3.14159265358979323846 * 0.25, s0 = std::sin(y0), c0 = std::cos(y0);
  for (int i = 0; i < 8; ++i) {
    const double y = -(x + 3 - i) * 3.14159265358979323846 * 0.25;
    c[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
    sum += c[i];
  }
  sum = 1.f / sum;
  for (int i = 0; i < 8; ++i) c[i] *= sum;
}

// [fy][fx][ksize^2] fixed-point weights, each set corrected to sum to 2^15 on one of the four centre taps
std::vector<int16_t> weight_table(int ksize) {
  std::vector<float> t1((size_t)kTab * ksize);
  for (int i = 0; i < kTab; ++i) kernel_1d(ksize, (float)i * (1.f / kTab), &t1[(size_t)i * ksize]);
  std::vector<int16_t> tab((size_t)kTab * kTab * ksize * ksize);
  for (int fy = 0; fy < kTab; ++fy)
    for (int fx = 0; fx < kTab; ++fx) {
      int16_t* w = &tab[((size_t)fy * kTab + fx) * ksize * ksize];
      int isum = 0;
      for (int r = 0; r < ksize; ++r)
        for (int c = 0; c < ksize; ++c) {
          long q = std::lrintf(t1[(size_t)fy * ksize + r] * t1[(size_t)fx * ksize + c] * (float)kCoefScale);
          q = q > 32767 ? 32767 : (q < -32768 ? -32768 : q);
          w[r * ksize + c] = (int16_t)q;
          isum += (int)q;
        }
      if (isum != kCoefScale) {
        const int diff = isum - kCoefScale, h = ksize / 2;
        int big = h * ksize + h, small = h * ksize + h;
        for (int r = h; r < h + 2; ++r)
          for (int c = h; c < h + 2; ++c) {
            const int i = r * ksize + c;
            if (w[i] < w[small]) small = i;
            else if (w[i] > w[big]) big = i;
          }
        if (diff < 0) w[big] = (int16_t)(w[big] - diff);
        else w[small] = (int16_t)(w[small] - diff);
      }
    }
  return tab;
}

// cv::logPolar's maps in remap's fixed-point form; rows = phi, columns = rho, centre (res/2, res/2)
// (cv::Point2f(resolution / 2, resolution / 2), scaleRotationEstimator.cpp:25). The reference compiles against one of
// two OpenCV generations (scaleRotationEstimator.cpp:41-46, :107-113) whose maps differ:
//   MOF_LOGPOLAR_CV4 (ROS Noetic, OpenCV 4.2) cv::logPolar = cv::warpPolar(.., maxRadius = exp(width / M), WARP_POLAR_LOG):
//     Kmag = log(maxRadius) / width, float table rhos[rho] = (float)(exp(rho * Kmag) - 1.0),
//     x = rhos[rho] * cos((2 pi / height) * phi) + cx, in double, stored as float;
//   MOF_LOGPOLAR_CV3 (ROS Melodic, OpenCV 3.2) cvLogPolar: double table exp(rho / M) -- no "- 1" --,
//     x = exp_tab[rho] * cos(phi * 2 pi / height) + cx.
// remap then rounds the float coordinates to 1/32 px: (anchor, fractional index) per destination pixel.
}  // namespace

namespace mof {

std::vector<SrMapEntry> sr_logpolar_map(int res, double M, int variant) {
  std::vector<SrMapEntry> map((size_t)res * res);
  const float cx = (float)(res / 2), cy = (float)(res / 2);
  const double PI = 3.14159265358979323846;
  std::vector<float> rhos((size_t)res);
  std::vector<double> exp_tab((size_t)res);
  const double Kmag = std::log(std::exp((double)res / M)) / (double)res, Kangle = 2.0 * PI / (double)res;
  for (int rho = 0; rho < res; ++rho) {
    rhos[(size_t)rho] = (float)(std::exp(rho * Kmag) - 1.0);
    exp_tab[(size_t)rho] = std::exp(rho / M);
  }
  for (int phi = 0; phi < res; ++phi) {
    const double ang = variant == MOF_LOGPOLAR_CV3 ? phi * 2 * PI / res : Kangle * phi;
    const double cp = std::cos(ang), sp = std::sin(ang);
    for (int rho = 0; rho < res; ++rho) {
      const double r = variant == MOF_LOGPOLAR_CV3 ? exp_tab[(size_t)rho] : (double)rhos[(size_t)rho];
      const float mx = (float)(r * cp + (double)cx), my = (float)(r * sp + (double)cy);
      const float fx = mx * (float)kTab, fy = my * (float)kTab;
      SrMapEntry e{0, 0, 0, 0};
      if (std::fabs(fx) < 1.0e9f && std::fabs(fy) < 1.0e9f) {
        const long ix = std::lrintf(fx), iy = std::lrintf(fy);
        long ax = ix >> 5, ay = iy >> 5;
        ax = ax > 32767 ? 32767 : (ax < -32768 ? -32768 : ax);
        ay = ay > 32767 ? 32767 : (ay < -32768 ? -32768 : ay);
        e.ax = (int16_t)ax;
        e.ay = (int16_t)ay;
        e.widx = (uint16_t)((iy & (kTab - 1)) * kTab + (ix & (kTab - 1)));
        e.valid = (ax >= 0 && ax < res && ay >= 0 && ay < res) ? 1 : 0;
      }
      map[(size_t)phi * res + rho] = e;
    }
  }
  return map;
}

std::vector<int16_t> sr_weight_table(int ksize) { return weight_table(ksize); }

std::vector<uint32_t> sr_weight_planes(const std::vector<int16_t>& weights, int ksize) {
  const int kk = ksize * ksize, stride = kk / 2 + 2;
  const size_t rows = weights.size() / kk;
  std::vector<uint32_t> out(rows * stride, 0u);
  for (size_t r = 0; r < rows; ++r) {
    uint32_t* o = out.data() + r * stride;
    int sum = 0, rem = -1;
    for (int t = 0; t < kk; ++t) {
      const int w = weights[r * kk + t];
      const int lo = (int)(int8_t)(w & 0xff);
      int hi = (w - lo) >> 8;
      if (hi > 127) {
        hi = 127;  // w >= 32640: at most one tap of a footprint (the weights sum to 2^15)
        rem = t;
      }
      sum += w;
      o[t / 4] |= (uint32_t)(hi & 0xff) << (8 * (t % 4));
      o[kk / 4 + t / 4] |= (uint32_t)(lo & 0xff) << (8 * (t % 4));
    }
    o[kk / 2] = (uint32_t)(128 * sum);
    o[kk / 2 + 1] = (uint32_t)rem;
  }
  return out;
}

std::vector<SrTileBox> sr_tile_boxes(const std::vector<SrMapEntry>& map, int res, int ksize, int* lds_per_wave, int tile_px) {
  const int tiles = (res + tile_px - 1) / tile_px, half = ksize / 2 - 1;
  std::vector<SrTileBox> boxes((size_t)tiles * tiles, SrTileBox{0, 0, 0, 0});
  int worst = 16;
  for (int ty = 0; ty < tiles; ++ty)
    for (int tx = 0; tx < tiles; ++tx) {
      int x0 = 1 << 20, y0 = 1 << 20, x1 = -1, y1 = -1;
      for (int l = 0; l < tile_px * tile_px; ++l) {
        const int rho = tx * tile_px + l % tile_px, phi = ty * tile_px + l / tile_px;
        if (rho >= res || phi >= res) continue;
        const SrMapEntry& m = map[(size_t)phi * res + rho];
        const int sx = m.ax - half, sy = m.ay - half;
        if (!m.valid) continue;
        // rows: every tap row, rows beyond the border reflected back in (BORDER_REFLECT_101; a valid anchor lies inside
        // the image and the kernel reaches at most ksize pixels from it, so one reflection is enough); columns: the
        // ksize-wide window the kernel reads, clamped into the image -- it contains every reflected tap column
        const int wx = sx < 0 ? 0 : (sx > res - ksize ? res - ksize : sx);
        x0 = wx < x0 ? wx : x0;
        x1 = wx + ksize > x1 ? wx + ksize : x1;
        for (int k = 0; k < ksize; ++k) {
          int yy = sy + k;
          yy = yy < 0 ? -yy : yy;
          yy = yy >= res ? 2 * res - 2 - yy : yy;
          y0 = yy < y0 ? yy : y0;
          y1 = yy + 1 > y1 ? yy + 1 : y1;
        }
      }
      if (x1 < 0) continue;
      boxes[(size_t)ty * tiles + tx] = SrTileBox{(int16_t)x0, (int16_t)y0, (int16_t)(x1 - x0), (int16_t)(y1 - y0)};
      const int lpd = ((x1 - x0) + 3 + 3) / 4 + 1;  // LDS row pitch in dwords, as the kernel computes it
      const int bytes = (y1 - y0) * lpd * 4;
      worst = bytes > worst ? bytes : worst;
    }
  *lds_per_wave = (worst + 15) & ~15;
  return boxes;
}

// Resolutions on the tuned transforms unpadded: 240 / 256 / 480, and every even tuned size with an exact Nyquist bin (MOF_SR_TUNED_ALL=0: the
// three only, A/B and tests). Any other resolution runs on the size cv::phaseCorrelate pads it to, plan.m = getOptimalDFTSize(resolution):
// where that size has tuned transforms, on the zero-padding frame form of K5s, K6s, K7 and only the final kernel of the planned pipeline (r06).
bool sr_route(int res, const SrKnobs& k, PcPlan* plan, SrRoute* r) {
  *r = SrRoute{};
  bool exact = false;
  if (sr_always_tuned(res) || (k.tuned_all && res % 2 == 0 && sr_transform_size_tuned(res, &exact) && exact)) {
    r->m = res;
    r->zh_floats = sr_zh_floats(res);
    r->candidates = sr_candidates(res);
    // Independent pairs run the FRAME kernels too (sr_seq_kernel.hip): each of the 2n log-polar images gets its own real row transform, K6s
    // correlates slot 2p against 2p + 1, one pair per wave-run, and the batch entry computes exactly what the stateful entry computes for a
    // fresh estimator fed (prev, cur): same bits. (The packed pair kernels and the fused K56 lost to them: docs/history/retired_switches.md.)
  } else {
    if (!pc_build_line_plan(res, plan)) return false;
    r->family = SrRoute::PLANNED;
    r->m = plan->m;
    r->zh_floats = pcl_zh_floats(*plan);
    r->candidates = pcl_candidates(*plan);
    exact = true;
    if (k.tuned_all && sr_transform_size_tuned(plan->m, &exact)) {
      r->family = SrRoute::TUNED_PAD;
      r->sums = !exact;
      if (r->sums) r->sums_off = (size_t)((plan->m >> 1) + 1) * ((plan->m + 7) & ~7) * 2;  // behind the padded rows; pcl_zh_floats leaves 16 floats per row of slack
    }
  }
  r->seq_run = k.seq_run;
  return true;
}

}  // namespace mof

using mof::BusyGuard;
using mof::SrRoute;

// Member order is the teardown order in reverse (dev_mem.hpp): the streams and the events are declared before the buffers, the host
// pipe last, so `delete e` -- after the waits of sr_destroy_now -- releases pipe, buffers, events, streams in that order.
struct mof_sr_engine {
  mof_sr_config cfg{};
  mof::Stream stream;
  // Two-lane batch pipeline: the log-polar remaps of chunk k+1 (bound by LDS / L1 latency, little HBM traffic) run on
  // `remap_stream` while the transforms of chunk k (bound by HBM) run on the caller's stream; the log-polar images are
  // double-buffered and handed over with events.
  mof::Stream remap_stream;
  mof::Event ev_fork;
  mof::Event ev_lp[2];   // remaps of the chunk using buffer b are done
  mof::Event ev_fft[2];  // transforms reading buffer b are done (it may be overwritten)
  mof::ScratchFence fence;  // ordering of the engine-owned scratch (d_lp, d_Zt, d_Dt, d_cand, d_out) across streams
  mof::DevMem<mof::SrMapEntry> d_map;
  mof::DevMem<mof::SrTileBox> d_boxes[2];  // cubic, Lanczos4
  int lds_per_wave[2] = {0, 0};
  mof::DevMem<int16_t> d_w_cubic, d_w_lanczos;
  mof::DevMem<uint32_t> d_wp[2];           // byte planes of the two tables (cubic, Lanczos4)
  mof::DevMem<mof::SrTileBox> d_sboxes[2]; // super-tile boxes (cubic, Lanczos4); null when res % 16 != 0
  int sbox_dwords[2] = {0, 0};
  mof::DevMem<float> d_twiddles;
  mof::DevMem<uint8_t> d_frame;    // staging for the stateful path (res*res)
  mof::DevMem<uint8_t> d_temp_im;  // tempIm, :27
  mof::DevMem<float> d_zh_prev;    // prevIm_F32 (:48, :128), kept as what the correlation needs of it: its row half-spectra
                                   // (sr_seq_kernel.hip, K5s) -- each frame is remapped and row-transformed ONCE
  // the pipeline scratch (scratch_alloc). A batch call captured into a HIP graph bakes raw pointers into it into the graph's kernel
  // nodes, so from then on it neither grows nor is freed until mof_sr_release_graphs (capi_graph.hpp)
  mof::DevMem<uint8_t> d_lp;       // batch: [kChunk][2][res*res] log-polar images (cur, prev)
  mof::DevMem<float> d_Zt, d_Dt;
  mof::DevMem<float2> d_cand;
  mof::DevMem<double> d_out;       // [kChunk][4]
  mof::DevMem<double> d_q;         // [kChunk][2]: a pass's (response, peak) where the host walks the response gate and the caller asked for no quality
  mof::PinnedMem<uint8_t> h_stage;
  mof::PinnedMem<double> h_out;    // [4 + 2]: one result and its quality
  mof::PinnedMem<double> h_seq;    // [chunk][4] + [chunk][2]: a pass's results and their quality, read back when a sequence call resolves the gates
  int chunk = 0;                 // frame pairs per pipeline pass
  int scratch_pairs = 0;         // pairs per pass the scratch holds now (1 after create, `chunk` after the first batch)
  bool two_lanes = false;        // remap of pass k+1 beside the transforms of pass k (mof_sr_config.pipeline_lanes == 2)
  bool first = true;             // :31
  double min_response = 0.0;     // mof_sr_set_min_response: 0 = the reference's gate alone
  SrRoute route;                 // which transforms every launch runs (sr_route)
  mof::SrLpRoute lp_route[2];    // which remap kernel a batch takes (sr_lp_route): cubic, Lanczos4
  mof::PcPlan plan{};            // route.family TUNED_PAD / PLANNED: the line plan of the padded size route.m
  std::atomic<bool> busy{false};
  std::atomic<bool> graph_pinned{false};  // a batch call was captured into a HIP graph
  std::mutex host_mu;  // mof_sr_process_sequence_host: the upload pipeline (host_pipe.hpp), made by its first call
  std::unique_ptr<mof::HostPipe> host_pipe;
  std::unique_ptr<mof::HostPipe> host_pipe_q;  // mof_sr_process_sequence_host_q with a quality output: the same pipeline with a second output
};

namespace {

// the three transform steps, by the engine's route
hipError_t rows_real(const mof_sr_engine* e, const uint8_t* lp, size_t lp_stride, float* zh, size_t zh_stride, int n_frames, hipStream_t s) {
  const int res = e->cfg.resolution;
  const SrRoute& r = e->route;
  if (r.family == SrRoute::TUNED) return mof::launch_sr_rows_real(lp, lp_stride, e->d_twiddles, zh, zh_stride, res, n_frames, s);
  mof::PclSrc src{};
  src.base[0] = lp;
  src.stride[0] = lp_stride;
  src.pitch = (size_t)res;  // log-polar images are tightly packed
  if (r.family == SrRoute::PLANNED) return mof::launch_pcl_rows(src, e->plan, e->d_twiddles, zh, zh_stride, nullptr, n_frames, 1, 1, s);
  src.paired = 2;  // "a video whose one patch is the whole image": image f = base[0] + f * stride[0]
  src.grid_x = src.grid_y = 1;
  src.stride_x = src.stride_y = res;
  int* sums = nullptr;
  if (r.sums) {
    sums = reinterpret_cast<int*>(zh + r.sums_off);
    src.sums_stride = (int)zh_stride;
    const hipError_t err = n_frames == 1 ? hipMemsetAsync(sums, 0, 4 * sizeof(int), s)  // (the row kernel adds into them; the stateful call passes no stride)
                                         : hipMemset2DAsync(sums, zh_stride * sizeof(float), 0, 4 * sizeof(int), (size_t)n_frames, s);
    if (err != hipSuccess) return err;
  }
  return mof::launch_sr_rows_real_src(mof::SrRowsSrc{src, e->d_twiddles, zh, zh_stride, nullptr, r.m, 1, res, sums}, n_frames, s);
}
// Run length of K6s for a pass of m consecutive pairs (r06; tools/video_probe.py showed the same shape on the FFT engine's video kernel): a
// wave walks `run` pairs one after the other, so a short video in runs of 16 leaves most of the chip idle -- 64 frames of 480^2 are 61 column
// groups x 4 runs = 244 one-wave workgroups on 2048 slots. Workgroups last run + ~0.6 column transforms (the first pair's previous spectra
// are transformed too), the launch lasts ceil(workgroups / slots) rounds: the shortest run within 3 % of the least product.
int seq_run_for(const mof_sr_engine* e, int m) {
  if (e->route.seq_run > 0) return e->route.seq_run;
  const int cus = mof::pc_cu_count(e->cfg.device);
  const int tn = e->route.m;
  const int cw = mof::sr_seq_columns_per_wave(tn);  // columns per wave
  if (cw == 0) return 16;  // (no K6s at this size: the planned L6 walks no runs)
  const long groups = (tn / 2 + 1 + cw - 1) / cw, slots = (long)cus * 8;  // one-wave workgroups, two per SIMD
  auto cost = [&](int r) {
    const long wgs = groups * ((m + r - 1) / r), rounds = (wgs + slots - 1) / slots;
    return (double)rounds * ((double)r + 0.6);
  };
  double best = cost(1);
  for (int r = 2; r <= 32; ++r) best = cost(r) < best ? cost(r) : best;
  for (int r = 1; r <= 32; ++r)
    if (cost(r) <= 1.03 * best) return r;
  return 16;
}
hipError_t cols_seq(const mof_sr_engine* e, const float* zh_prev, const float* zh_cur, size_t zh_stride, int n_pairs, int run, hipStream_t s) {
  const SrRoute& r = e->route;
  if (r.family == SrRoute::PLANNED) return mof::launch_pcl_cols(zh_prev, zh_cur, zh_stride, e->plan, e->d_twiddles, e->d_Dt, nullptr, nullptr, n_pairs, s);
  mof::SrColsSeq a{zh_prev, zh_cur, zh_stride, e->d_twiddles, e->d_Dt, r.m, run, nullptr, e->cfg.resolution, nullptr, nullptr, 0};
  if (r.sums) {
    a.sums_prev = reinterpret_cast<const int*>(zh_prev + r.sums_off);
    a.sums_cur = reinterpret_cast<const int*>(zh_cur + r.sums_off);
    a.sums_stride = (int)zh_stride;
  }
  return mof::launch_sr_cols_seq(a, n_pairs, s);
}
hipError_t peak(const mof_sr_engine* e, const mof::SrPcArgs& a, int n_pairs, hipStream_t s) {
  const SrRoute& r = e->route;
  if (r.family == SrRoute::TUNED) return mof::launch_sr_peak(a, r.m, n_pairs, s);
  mof::PclFinal f{};
  f.Dt = a.Dt;
  f.cand = a.cand;
  f.twiddles = a.twiddles;
  f.mode = 0;
  f.M_log = a.M;
  f.out = a.out;
  f.quality = a.quality;
  f.min_response = a.min_response;
  if (r.family == SrRoute::PLANNED) return mof::launch_pcl_peak(f, e->plan, n_pairs, s);
  // K7 forms the candidates; L8 (the planned pipeline's final kernel: it knows the padded geometry) reads them
  const hipError_t err = mof::launch_sr_rows_inv(a.Dt, a.twiddles, a.cand, r.m, n_pairs, s);
  return err != hipSuccess ? err : mof::launch_pcl_peak(f, e->plan, n_pairs, s, true);
}

// The pipeline scratch (log-polar images of two passes, Zt, Dt, peak candidates, results, their quality) for `pairs` pairs per pass.
hipError_t scratch_alloc(mof_sr_engine* e, int pairs) {
  mof::RelaxedCapture relaxed;  // allocation / release must not invalidate a capture on another thread
  const size_t nn = (size_t)e->cfg.resolution * e->cfg.resolution, zhf = e->route.zh_floats, n = (size_t)pairs;
  // d_Zt: the sequence pipeline's (pairs + 1) frames of half spectra; independent pairs: 2 * pairs frames of half spectra
  const size_t zh = (n + 1 > 2 * n ? n + 1 : 2 * n) * zhf;
  e->scratch_pairs = 0;
  // d_lp holds two passes: remap of pass k+1 beside the transforms of pass k; Dt has Zh's shape
  const hipError_t err = mof::alloc_all(e->d_lp, 2 * n * 2 * nn, e->d_Zt, zh, e->d_Dt, n * zhf, e->d_cand, n * e->route.candidates,
                                        e->d_out, n * 4, e->d_q, n * 2);
  if (err == hipSuccess) e->scratch_pairs = pairs;
  return err;
}

// Pairs per pass a batch of n pairs needs: n rounded up to a power of two (growing batches re-allocate O(log) times),
// a whole pass at most. mof_sr_reserve and the batch entry use the same rule.
int scratch_want(const mof_sr_engine* e, int n_pairs) {
  int want = 1;
  while (want < n_pairs && want < e->chunk) want <<= 1;
  return want < e->chunk ? want : e->chunk;
}

// Makes sure the scratch holds a pass of `pairs` pairs. Growing frees and re-allocates: not possible while `s` is
// being captured into a graph (run one batch, or mof_sr_reserve, before the capture), and only after every earlier
// user of the scratch has finished. Returns a MOF status.
int scratch_reserve(mof_sr_engine* e, int pairs, hipStream_t s) {
  return mof::grow_scratch(e->graph_pinned.load(), e->fence, {e->stream, e->remap_stream}, mof::stream_capturing(s),
                           "the estimator's scratch (pairs per pass)", e->scratch_pairs, pairs, 1, [e](long n) { return scratch_alloc(e, (int)n); });
}

}  // namespace

extern "C" {

int mof_sr_reserve(mof_sr_engine* e, int n_pairs) {
  if (!e) return mof::capi_fail(MOF_ERR_NOT_INIT, "null engine");
  if (n_pairs < 0) return mof::capi_fail(MOF_ERR_BAD_ARG, "n_pairs must be >= 0");
  BusyGuard g(e->busy);
  if (!g.owned) return mof::capi_fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return scratch_reserve(e, scratch_want(e, n_pairs), e->stream);
}

static void sr_destroy_now(void* p) {
  mof_sr_engine* e = static_cast<mof_sr_engine*>(p);
  mof::RelaxedCapture relaxed;
  (void)hipSetDevice(e->cfg.device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->remap_stream) (void)hipStreamSynchronize(e->remap_stream);
  e->fence.wait_idle();
  delete e;
}
struct SrDestroyNow {
  void operator()(mof_sr_engine* e) const { sr_destroy_now(e); }
};

void mof_sr_destroy(mof_sr_engine* e) {
  if (!e) return;
  if (e->graph_pinned.load()) {  // replays of a captured graph would run through freed scratch: park until released
    mof::park_engine(&sr_destroy_now, e);
    return;
  }
  sr_destroy_now(e);
}

int mof_sr_release_graphs(mof_sr_engine* e) {
  if (!e) return mof::capi_fail(MOF_ERR_NOT_INIT, "null engine");
  e->graph_pinned.store(false);
  return MOF_OK;
}

int mof_sr_graph_pinned(const mof_sr_engine* e) { return e && e->graph_pinned.load() ? 1 : 0; }

int mof_sr_create(const mof_sr_config* cfg, mof_sr_engine** out) try {
  if (!out) return mof::capi_fail(MOF_ERR_BAD_ARG, "null out");
  *out = nullptr;
  if (!cfg || !(cfg->magnitude > 0.0)) return mof::capi_fail(MOF_ERR_BAD_ARG, "bad scale/rotation config");
  if (cfg->logpolar_variant != MOF_LOGPOLAR_CV4 && cfg->logpolar_variant != MOF_LOGPOLAR_CV3)
    return mof::capi_fail(MOF_ERR_BAD_ARG, "logpolar_variant must be MOF_LOGPOLAR_CV4 (0) or MOF_LOGPOLAR_CV3 (1)");
  if (cfg->batch_chunk < 0 || cfg->batch_chunk > 4096 || cfg->pipeline_lanes < 0 || cfg->pipeline_lanes > 2)
    return mof::capi_fail(MOF_ERR_BAD_ARG, "batch_chunk must be 0..4096 and pipeline_lanes 0..2");
  // any even resolution: scaleRotationEstimator takes `res` from a parameter (scaleRotationEstimator.cpp:3-5)
  if (cfg->resolution < 16 || (cfg->resolution & 1))
    return mof::capi_fail(MOF_ERR_BAD_ARG, "resolution %d: an even resolution >= 16 is required", cfg->resolution);
  mof::PcPlan plan{};
  SrRoute route;
  if (!mof::sr_route(cfg->resolution, sr_knobs(), &plan, &route))
    return mof::capi_fail(MOF_ERR_UNSUPPORTED, "resolution %d pads to %d: beyond the planned transforms (<= 960)", cfg->resolution,
                          mof::pc_optimal_dft_size(cfg->resolution));
  {
    const int rc = mof::select_device(cfg->device);
    if (rc) return rc;
  }
  mof::RelaxedCapture relaxed;  // allocating an engine must not invalidate a capture on another thread
  const int res = cfg->resolution;
  const size_t nn = (size_t)res * res;
  const std::vector<mof::SrMapEntry> map = mof::sr_logpolar_map(res, cfg->magnitude, cfg->logpolar_variant);
  const std::vector<int16_t> wc = weight_table(4), wl = weight_table(8);
  int lds_c = 0, lds_l = 0;
  const std::vector<mof::SrTileBox> bc = mof::sr_tile_boxes(map, res, 4, &lds_c, 8), bl = mof::sr_tile_boxes(map, res, 8, &lds_l, 8);
  // boxes of the 16 x 16 super-tiles (one workgroup = four tiles sharing a staged box)
  int slds_c = 0, slds_l = 0;
  std::vector<mof::SrTileBox> sbc, sbl;
  if (res % 16 == 0) {
    sbc = mof::sr_tile_boxes(map, res, 4, &slds_c, 16);
    sbl = mof::sr_tile_boxes(map, res, 8, &slds_l, 16);
  }
  const std::vector<float> tw = mof::twiddle_table(route.m);
  std::unique_ptr<mof_sr_engine, SrDestroyNow> e(new (std::nothrow) mof_sr_engine());  // every early return tears down what exists
  if (!e) return mof::capi_fail(MOF_ERR_NO_MEMORY, "out of host memory");
  e->cfg = *cfg;
  e->route = route;
  e->plan = plan;
  e->chunk = chunk_pairs(cfg->batch_chunk);
  e->two_lanes = two_lane_default(cfg->pipeline_lanes);
  HIP_TRY(e->stream.create());
  HIP_TRY(e->fence.create());
  HIP_TRY(e->remap_stream.create());
  HIP_TRY(e->ev_fork.create());
  for (int b = 0; b < 2; ++b) {
    HIP_TRY(e->ev_lp[b].create());
    HIP_TRY(e->ev_fft[b].create());
  }
  HIP_TRY(mof::upload(e->d_map, map, e->stream));
  e->lds_per_wave[0] = lds_c;
  e->lds_per_wave[1] = lds_l;
  HIP_TRY(mof::upload(e->d_boxes[0], bc, e->stream));
  HIP_TRY(mof::upload(e->d_boxes[1], bl, e->stream));
  for (int k = 0; k < 2; ++k)
    e->lp_route[k] = mof::sr_lp_route(res, e->lds_per_wave[k] / 4, (k == 0 ? slds_c : slds_l) / 4, !sbc.empty(), k == 0 ? 2 : 4, sr_knobs());
  if (!sbc.empty()) {
    e->sbox_dwords[0] = slds_c / 4;
    e->sbox_dwords[1] = slds_l / 4;
    if (sr_knobs().verbose)  // diagnostics: the staged remap's largest boxes (dwords)
      fprintf(stderr, "mof_sr: res %d: largest super-tile box cubic %d, lanczos4 %d dwords; per-wave boxes %d / %d bytes\n", res, e->sbox_dwords[0],
              e->sbox_dwords[1], lds_c, lds_l);
    HIP_TRY(mof::upload(e->d_sboxes[0], sbc, e->stream));
    HIP_TRY(mof::upload(e->d_sboxes[1], sbl, e->stream));
  }
  HIP_TRY(mof::upload(e->d_w_cubic, wc, e->stream));
  HIP_TRY(mof::upload(e->d_w_lanczos, wl, e->stream));
  HIP_TRY(mof::upload(e->d_wp[0], mof::sr_weight_planes(wc, 4), e->stream));
  HIP_TRY(mof::upload(e->d_wp[1], mof::sr_weight_planes(wl, 8), e->stream));
  HIP_TRY(mof::upload(e->d_twiddles, tw, e->stream));
  HIP_TRY(mof::alloc_all(e->d_frame, nn, e->d_temp_im, nn, e->d_zh_prev, route.zh_floats));
  HIP_TRY(mof::fill_on(e->stream, e->d_temp_im, 0, nn));  // tempIm = cv::Mat::zeros, :27
  HIP_TRY(mof::fill_on(e->stream, e->d_zh_prev, 0, route.zh_floats * sizeof(float)));
  HIP_TRY(scratch_alloc(e.get(), 1));  // the stateful call needs one pair; a batch grows it to a whole pass (scratch_reserve)
  HIP_TRY(mof::alloc_all(e->h_stage, nn, e->h_out, 6, e->h_seq, (size_t)e->chunk * 6));
  *out = e.release();
  return MOF_OK;
} catch (const std::bad_alloc&) {
  return mof::capi_fail(MOF_ERR_NO_MEMORY, "mof_sr_create: out of host memory");
}

int mof_sr_reset(mof_sr_engine* e) {
  if (!e) return mof::capi_fail(MOF_ERR_NOT_INIT, "null engine");
  BusyGuard g(e->busy);
  if (!g.owned) return mof::capi_fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipMemsetAsync(e->d_temp_im, 0, (size_t)e->cfg.resolution * e->cfg.resolution, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->first = true;
  return MOF_OK;
}

int mof_sr_set_min_response(mof_sr_engine* e, double min_response) {
  if (!e) return mof::capi_fail(MOF_ERR_NOT_INIT, "null engine");
  if (!std::isfinite(min_response) || min_response < 0.0) return mof::capi_fail(MOF_ERR_BAD_ARG, "min_response must be finite and >= 0");
  BusyGuard g(e->busy);
  if (!g.owned) return mof::capi_fail(MOF_ERR_BUSY, "engine busy");
  // a captured final kernel holds the old value as an argument: a replay would gate by it while the host walks by the new one
  if (e->graph_pinned.load()) return mof::capi_fail(MOF_ERR_BUSY, "min_response is baked into a captured graph: mof_sr_release_graphs first");
  e->min_response = min_response;
  return MOF_OK;
}

double mof_sr_min_response(const mof_sr_engine* e) { return e ? e->min_response : 0.0; }

// The engine's half of a remap's arguments under one interpolation (2 cubic, 4 Lanczos4): the map and the tables lp_route[k] was made
// from. The caller sets src / dst, the strides, pitch and zero_invalid.
static mof::SrLpArgs lp_args(const mof_sr_engine* e, int interp) {
  const int k = interp == 2 ? 0 : 1;
  mof::SrLpArgs lp{};
  lp.map = e->d_map;
  lp.res = e->cfg.resolution;
  lp.weights = k == 0 ? e->d_w_cubic : e->d_w_lanczos;
  lp.wplanes = e->d_wp[k];
  lp.sboxes = e->d_sboxes[k];
  lp.sbox_dwords_max = e->sbox_dwords[k];
  lp.boxes = e->d_boxes[k];
  lp.lds_per_wave = e->lds_per_wave[k];
  lp.box_dwords_max = e->lds_per_wave[k] / 4;
  return lp;
}
static hipError_t remap(const mof_sr_engine* e, const mof::SrLpArgs& lp, int interp, int n_images, hipStream_t s) {
  return mof::launch_sr_logpolar(lp, e->lp_route[interp == 2 ? 0 : 1], n_images, s);
}

static mof::SrPcArgs pc_args(const mof_sr_engine* e, double* out, double* quality) {
  mof::SrPcArgs a{};
  a.twiddles = e->d_twiddles;
  a.Dt = e->d_Dt;
  a.cand = e->d_cand;
  a.n_cand = e->route.candidates;
  a.M = e->cfg.magnitude;
  a.out = out;
  a.quality = quality;
  a.min_response = e->min_response;
  return a;
}

// both gates on the host, from the doubles the final kernel stored and decided by (pc_common.hpp, sr_finish): the reference's |pt.x| > res / 2
// (:119-121) and, armed by min_response > 0, !(response >= min_response)
static bool sr_gated(const mof_sr_engine* e, double ptx, double response) {
  return std::fabs(ptx) > (double)(e->cfg.resolution / 2) || (e->min_response > 0.0 && !(response >= e->min_response));
}

// One pair through the sequence kernels: (cur spectra, prev spectra) -> Dt slot 0 -> (scale, rot, pt) at `out`, (response, peak) at `quality` (nullable)
static hipError_t seq_one_pair(mof_sr_engine* e, const float* zh_prev, const float* zh_cur, double* out, double* quality, hipStream_t s) {
  hipError_t err = cols_seq(e, zh_prev, zh_cur, 0, 1, 1, s);
  if (err != hipSuccess) return err;
  mof::SrPcArgs a = pc_args(e, out, quality);
  return peak(e, a, 1, s);
}

int mof_sr_process(mof_sr_engine* e, const uint8_t* frame, size_t pitch, double* out_scale_rot) {
  return mof_sr_process_q(e, frame, pitch, out_scale_rot, nullptr);
}

int mof_sr_process_q(mof_sr_engine* e, const uint8_t* frame, size_t pitch, double* out_scale_rot, double* quality) {
  if (!e) return mof::capi_fail(MOF_ERR_NOT_INIT, "null engine");
  const int res = e->cfg.resolution;
  if (!frame || !out_scale_rot || pitch < (size_t)res) return mof::capi_fail(MOF_ERR_BAD_ARG, "bad frame/pitch/out");
  BusyGuard g(e->busy);
  if (!g.owned) return mof::capi_fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t nn = (size_t)res * res, zh_bytes = e->route.zh_floats * sizeof(float);
  for (int y = 0; y < res; ++y) std::memcpy(e->h_stage + (size_t)y * res, frame + (size_t)y * pitch, (size_t)res);
  HIP_TRY(hipMemcpyAsync(e->d_frame, e->h_stage, nn, hipMemcpyHostToDevice, e->stream));
  const int interp = e->first ? 2 : 4;  // INTER_CUBIC for the very first frame (:45), INTER_LANCZOS4 from then on (:112)
  mof::SrLpArgs lp = lp_args(e, interp);
  lp.src = e->d_frame;
  lp.pitch = (size_t)res;
  lp.dst = e->d_temp_im;
  HIP_TRY(remap(e, lp, interp, 1, e->stream));
  HIP_TRY(e->fence.acquire(e->stream));
  // tempIm.convertTo(CV_32FC1) (:47, :115) + the row half of the forward DFT of cv::phaseCorrelate (:117): K5s
  HIP_TRY(rows_real(e, e->d_temp_im, 0, e->d_Zt, 0, 1, e->stream));
  if (e->first) {
    HIP_TRY(hipMemcpyAsync(e->d_zh_prev, e->d_Zt, zh_bytes, hipMemcpyDeviceToDevice, e->stream));  // prevIm_F32 = .., :48
    HIP_TRY(e->fence.release(e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->first = false;  // :73
    out_scale_rot[0] = 1.0;
    out_scale_rot[1] = 0.0;  // :74
    if (quality) quality[0] = quality[1] = std::nan("");  // no correlation ran
    return MOF_OK;
  }
  const bool want_q = quality || e->min_response > 0.0;  // (the response gate is walked from the stored double)
  HIP_TRY(seq_one_pair(e, e->d_zh_prev, e->d_Zt, e->d_out, want_q ? e->d_q.get() : nullptr, e->stream));  // :117
  HIP_TRY(hipMemcpyAsync(e->h_out, e->d_out, 4 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (want_q) HIP_TRY(hipMemcpyAsync(e->h_out + 4, e->d_q, 2 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  out_scale_rot[0] = e->h_out[0];
  out_scale_rot[1] = e->h_out[1];
  if (quality) {
    quality[0] = e->h_out[4];
    quality[1] = e->h_out[5];
  }
  // the reference returns early on the gate, BEFORE prevIm_F32 = tempIm_F32.clone() (:119-121 vs :128)
  if (!sr_gated(e, e->h_out[2], want_q ? e->h_out[4] : 0.0))
    HIP_TRY(hipMemcpyAsync(e->d_zh_prev, e->d_Zt, zh_bytes, hipMemcpyDeviceToDevice, e->stream));
  HIP_TRY(e->fence.release(e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MOF_OK;
}

// A video on the device = n_frames consecutive mof_sr_process calls (see mof.h). Per pass of up to `chunk` new frames the
// scratch holds slot 0 = the spectra the first new frame is correlated with, slots 1..m = the new frames.
int mof_sr_process_sequence_device(mof_sr_engine* e, const uint8_t* d_frames, size_t frame_stride, size_t pitch, int n_frames,
                                   double* d_out, void* stream, int* n_gated) {
  return mof_sr_process_sequence_device_q(e, d_frames, frame_stride, pitch, n_frames, d_out, nullptr, stream, n_gated);
}

int mof_sr_process_sequence_device_q(mof_sr_engine* e, const uint8_t* d_frames, size_t frame_stride, size_t pitch, int n_frames,
                                     double* d_out, double* d_quality, void* stream, int* n_gated) {
  if (!e) return mof::capi_fail(MOF_ERR_NOT_INIT, "null engine");
  const int res = e->cfg.resolution;
  if (n_gated) *n_gated = 0;
  if (n_frames == 0) return MOF_OK;
  if (!d_frames || !d_out || n_frames < 0 || pitch < (size_t)res) return mof::capi_fail(MOF_ERR_BAD_ARG, "bad sequence arguments");
  BusyGuard g(e->busy);
  if (!g.owned) return mof::capi_fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  const bool capturing = mof::stream_capturing(s);
  if (capturing && n_gated)
    return mof::capi_fail(MOF_ERR_BAD_ARG, "resolving the gate reads results back on the host: pass n_gated = NULL while capturing");
  const size_t nn = (size_t)res * res, zhf = e->route.zh_floats, zh_bytes = zhf * sizeof(float);
  {
    const int rc = scratch_reserve(e, scratch_want(e, n_frames), s);
    if (rc != MOF_OK) return rc;
  }
  // A fresh estimator's first frame takes the INTER_CUBIC branch (:45) ONCE; captured, that branch would be baked into the
  // graph and every replay would redo it while the engine believes it is in its steady state. Capture on an armed engine.
  if (capturing && e->first)
    return mof::capi_fail(MOF_ERR_BAD_ARG, "capturing a sequence on a fresh estimator would bake its one-off first-frame branch "
                                            "(INTER_CUBIC, scaleRotationEstimator.cpp:45) into the graph: process one frame first");
  HIP_TRY(e->fence.acquire(s));
  if (capturing) e->graph_pinned.store(true);
  const int C = e->scratch_pairs < e->chunk ? e->scratch_pairs : e->chunk;  // new frames per pass
  float* zh = e->d_Zt;
  // The host-side state (`first`, and the device-side prevIm_F32 = d_zh_prev, whose update is the LAST thing enqueued) is
  // committed only when every launch of the call went out: a call that fails half-way leaves the estimator exactly as it was,
  // and the scratch is released on that path too.
  bool first = e->first;
  int gated_total = 0;
  const int rc = [&]() -> int {
    // tempIm starts as zeros (:27) and transparent pixels never change: write the zeros here (zero_invalid)
    auto frames = [&](int interp, int first_frame, uint8_t* dst) {
      mof::SrLpArgs lp = lp_args(e, interp);
      lp.zero_invalid = 1;
      lp.pitch = pitch;
      lp.src = d_frames + (size_t)first_frame * frame_stride;
      lp.src_stride = frame_stride;
      lp.dst = dst;
      lp.dst_stride = nn;
      return lp;
    };
    int done = 0;
    int carry = -1;  // slot of the previous pass whose spectra are `prev` for the next frame (-1: the engine's state)
    while (done < n_frames) {
      if (first) {  // the very first frame: INTER_CUBIC (:45), becomes prev (:48), returns (1, 0) (:74)
        HIP_TRY(remap(e, frames(2, done, e->d_lp), 2, 1, s));
        HIP_TRY(rows_real(e, e->d_lp, nn, zh, zhf, 1, s));
        HIP_TRY(mof::launch_sr_identity(d_out + 4 * (size_t)done, d_quality ? d_quality + 2 * (size_t)done : nullptr, s));
        first = false;  // :73
        ++done;
      } else if (carry < 0) {
        HIP_TRY(hipMemcpyAsync(zh, e->d_zh_prev, zh_bytes, hipMemcpyDeviceToDevice, s));
      } else if (carry > 0) {
        HIP_TRY(hipMemcpyAsync(zh, zh + (size_t)carry * zhf, zh_bytes, hipMemcpyDeviceToDevice, s));
      }
      const int m = n_frames - done < C ? n_frames - done : C;
      carry = 0;
      if (m > 0) {
        HIP_TRY(remap(e, frames(4, done, e->d_lp + nn), 4, m, s));  // INTER_LANCZOS4, :112 -- every frame once
        HIP_TRY(rows_real(e, e->d_lp + nn, nn, zh + zhf, zhf, m, s));
        HIP_TRY(cols_seq(e, zh, zh + zhf, zhf, m, seq_run_for(e, m), s));
        // the pass's quality: the caller's array, or -- where the host walks the response gate below and needs it all the same -- the engine's
        double* q = d_quality ? d_quality + 2 * (size_t)done : (n_gated && e->min_response > 0.0 ? e->d_q.get() : nullptr);
        mof::SrPcArgs a = pc_args(e, d_out + 4 * (size_t)done, q);
        HIP_TRY(peak(e, a, m, s));
        carry = m;
        if (n_gated) {
          // The gates (:119-121, and the response gate that acts like it): a gated frame returns (1, 0) and does NOT become prev. The pass
          // above correlated every frame with its immediate predecessor; behind a gated frame that is the wrong partner, so
          // walk the results in order and redo the (rare) pairs whose reference partner is an older frame.
          double* hq = e->h_seq + 4 * (size_t)e->chunk;
          HIP_TRY(hipMemcpyAsync(e->h_seq, d_out + 4 * (size_t)done, (size_t)m * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
          if (q) HIP_TRY(hipMemcpyAsync(hq, q, (size_t)m * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
          HIP_TRY(hipStreamSynchronize(s));
          int prev_slot = 0;
          for (int i = 1; i <= m; ++i) {
            double ptx = e->h_seq[4 * (size_t)(i - 1) + 2], response = q ? hq[2 * (size_t)(i - 1)] : 0.0;
            if (prev_slot != i - 1) {
              double* o = d_out + 4 * (size_t)(done + i - 1);
              double* oq = q ? q + 2 * (size_t)(i - 1) : nullptr;  // the redone frame's quality is that of the pair that now stands
              HIP_TRY(seq_one_pair(e, zh + (size_t)prev_slot * zhf, zh + (size_t)i * zhf, o, oq, s));
              HIP_TRY(hipMemcpyAsync(e->h_out, o, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
              if (oq) HIP_TRY(hipMemcpyAsync(e->h_out + 4, oq, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
              HIP_TRY(hipStreamSynchronize(s));
              ptx = e->h_out[2];
              response = oq ? e->h_out[4] : 0.0;
            }
            if (sr_gated(e, ptx, response)) ++gated_total;
            else prev_slot = i;
          }
          carry = prev_slot;
        }
        done += m;
      }
    }
    // prevIm_F32 <- the last frame that passed the gate (:128)
    if (carry >= 0) HIP_TRY(hipMemcpyAsync(e->d_zh_prev, zh + (size_t)carry * zhf, zh_bytes, hipMemcpyDeviceToDevice, s));
    return MOF_OK;
  }();
  if (rc != MOF_OK) {
    (void)e->fence.release(s);  // (the error text of the failing launch stays the thread's last error)
    return rc;
  }
  e->first = first;
  HIP_TRY(e->fence.release(s));
  if (n_gated) {
    HIP_TRY(hipStreamSynchronize(s));
    *n_gated = gated_total;
  }
  return MOF_OK;
}

int mof_sr_process_sequence_host(mof_sr_engine* e, const uint8_t* frames, size_t frame_stride, size_t pitch, int n_frames,
                                 double* out, int* n_gated) {
  return mof_sr_process_sequence_host_q(e, frames, frame_stride, pitch, n_frames, out, nullptr, n_gated);
}

int mof_sr_process_sequence_host_q(mof_sr_engine* e, const uint8_t* frames, size_t frame_stride, size_t pitch, int n_frames,
                                   double* out, double* quality, int* n_gated) try {
  if (!e) return mof::capi_fail(MOF_ERR_NOT_INIT, "null engine");
  if (n_gated) *n_gated = 0;
  if (n_frames == 0) return MOF_OK;
  const int res = e->cfg.resolution;
  if (!frames || !out || n_frames < 0 || pitch < (size_t)res) return mof::capi_fail(MOF_ERR_BAD_ARG, "bad video arguments");
  HIP_TRY(hipSetDevice(e->cfg.device));
  mof::RelaxedCapture relaxed;
  const size_t bpp[2] = {4 * sizeof(double), 2 * sizeof(double)};
  {
    std::lock_guard<std::mutex> lock(e->host_mu);
    if (!e->host_pipe) e->host_pipe.reset(new mof::HostPipe((size_t)res * res, bpp, 1));
    if (quality && !e->host_pipe_q) e->host_pipe_q.reset(new mof::HostPipe((size_t)res * res, bpp, 2));
  }
  const mof::HostPipe::Out o[2] = {{out, bpp[0]}, {quality, bpp[1]}};
  mof::HostPipe* pipe = (quality ? e->host_pipe_q : e->host_pipe).get();
  hipError_t he = hipSuccess;
  int gated_total = 0;
  // the frames go up in chunks on the pipe's copy stream, each chunk runs through the DEVICE video entry -- stateful, so chunk k + 1
  // continues where chunk k stopped, and with the gate resolved (n_gated != NULL there), i.e. exactly the frame-by-frame calls
  const int rc = pipe->process_frames(
      frames, frame_stride, pitch, res, res, n_frames, o, e->stream,
      [e, quality, &gated_total](const mof::HostPipe::Chunk& c, hipStream_t s) {
        int g = 0;
        const int r = mof_sr_process_sequence_device_q(e, c.d_cur, c.stride, (size_t)e->cfg.resolution, c.count, static_cast<double*>(c.d_out[0]),
                                                       quality ? static_cast<double*>(c.d_out[1]) : nullptr, s, &g);
        gated_total += g;
        return r;
      },
      &he);
  if (rc == -1) return mof::capi_fail(MOF_ERR_HIP, "host video pipeline: %s", hipGetErrorString(he));
  if (n_gated) *n_gated = gated_total;
  return rc;
} catch (const std::bad_alloc&) {
  return mof::capi_fail(MOF_ERR_NO_MEMORY, "mof_sr_process_sequence_host: out of host memory");
}

int mof_sr_process_batch_device(mof_sr_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev,
                                size_t prev_stride, size_t pitch, int n_pairs, double* d_out, void* stream) {
  return mof_sr_process_batch_device_q(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, d_out, nullptr, stream);
}

int mof_sr_process_batch_device_q(mof_sr_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev, size_t prev_stride,
                                  size_t pitch, int n_pairs, double* d_out, double* d_quality, void* stream) {
  if (!e) return mof::capi_fail(MOF_ERR_NOT_INIT, "null engine");
  const int res = e->cfg.resolution;
  if (n_pairs == 0) return MOF_OK;  // an empty batch carries no pointers to check
  if (!d_cur || !d_prev || !d_out || n_pairs < 0 || pitch < (size_t)res) return mof::capi_fail(MOF_ERR_BAD_ARG, "bad batch arguments");
  BusyGuard g(e->busy);
  if (!g.owned) return mof::capi_fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  const size_t nn = (size_t)res * res;
  {
    const int rc = scratch_reserve(e, scratch_want(e, n_pairs), s);
    if (rc != MOF_OK) return rc;
  }
  HIP_TRY(e->fence.acquire(s));
  if (mof::stream_capturing(s)) e->graph_pinned.store(true);
  const int kChunk = e->chunk;
  // Under graph capture the fork / join below pulls the engine's stream into the caller's capture (event record on the
  // capturing stream, wait on the other), so a captured batch replays with the same two lanes.
  const bool two_lanes = e->two_lanes && n_pairs > kChunk;
  hipStream_t sr = two_lanes ? e->remap_stream : s;
  if (two_lanes) {  // fork: the remap lane starts behind whatever the caller's stream holds (also under graph capture)
    HIP_TRY(hipEventRecord(e->ev_fork, s));
    HIP_TRY(hipStreamWaitEvent(sr, e->ev_fork, 0));
  }
  int chunk_no = 0;
  for (int k0 = 0; k0 < n_pairs; k0 += kChunk, ++chunk_no) {
    const int n = (n_pairs - k0 < kChunk) ? n_pairs - k0 : kChunk;
    const int b = two_lanes ? (chunk_no & 1) : 0;
    uint8_t* lp_buf = e->d_lp + (size_t)b * kChunk * 2 * nn;
    // every pair is the two-call sequence of a fresh estimator: prev -> INTER_CUBIC (:45), cur -> INTER_LANCZOS4
    // (:112) onto the same zero-initialised tempIm; the transparent pixels are the same for both maps, so both
    // remaps simply write zeros there (zero_invalid) and the scratch needs no clearing pass
    if (two_lanes && chunk_no >= 2) HIP_TRY(hipStreamWaitEvent(sr, e->ev_fft[b], 0));  // buffer b is free again
    auto side = [&](int interp, const uint8_t* src, size_t stride, uint8_t* dst) {
      mof::SrLpArgs lp = lp_args(e, interp);
      lp.zero_invalid = 1;
      lp.pitch = pitch;
      lp.src = src + (size_t)k0 * stride;
      lp.src_stride = stride;
      lp.dst = dst;
      lp.dst_stride = 2 * nn;
      return lp;
    };
    HIP_TRY(remap(e, side(2, d_prev, prev_stride, lp_buf + nn), 2, n, sr));
    HIP_TRY(remap(e, side(4, d_cur, cur_stride, lp_buf), 4, n, sr));
    if (two_lanes) {
      HIP_TRY(hipEventRecord(e->ev_lp[b], sr));
      HIP_TRY(hipStreamWaitEvent(s, e->ev_lp[b], 0));  // also the join: every remap precedes a wait on the caller's stream
    }
    // the frame kernels: image 2p = cur of pair p, 2p + 1 = prev
    const size_t zhf = e->route.zh_floats;
    HIP_TRY(rows_real(e, lp_buf, nn, e->d_Zt, zhf, 2 * n, s));
    HIP_TRY(cols_seq(e, e->d_Zt + zhf, e->d_Zt, 2 * zhf, n, 1, s));
    HIP_TRY(peak(e, pc_args(e, d_out + 4 * (size_t)k0, d_quality ? d_quality + 2 * (size_t)k0 : nullptr), n, s));
    if (two_lanes) HIP_TRY(hipEventRecord(e->ev_fft[b], s));
  }
  HIP_TRY(e->fence.release(s));
  return MOF_OK;
}


int mof_sr_logpolar_batch_device(mof_sr_engine* e, const uint8_t* d_src, size_t src_stride, size_t pitch, int n_images,
                                 int interpolation, uint8_t* d_dst, void* stream) {
  if (!e) return mof::capi_fail(MOF_ERR_NOT_INIT, "null engine");
  const int res = e->cfg.resolution;
  if (n_images == 0) return MOF_OK;
  if (!d_src || !d_dst || n_images < 0 || pitch < (size_t)res) return mof::capi_fail(MOF_ERR_BAD_ARG, "bad batch arguments");
  if (interpolation != MOF_INTER_CUBIC && interpolation != MOF_INTER_LANCZOS4)
    return mof::capi_fail(MOF_ERR_BAD_ARG, "interpolation must be MOF_INTER_CUBIC (2) or MOF_INTER_LANCZOS4 (4)");
  BusyGuard g(e->busy);
  if (!g.owned) return mof::capi_fail(MOF_ERR_BUSY, "engine busy");
  HIP_TRY(hipSetDevice(e->cfg.device));
  mof::SrLpArgs lp = lp_args(e, interpolation);
  lp.src = d_src;
  lp.src_stride = src_stride;
  lp.pitch = pitch;
  lp.dst = d_dst;
  lp.dst_stride = (size_t)res * res;
  if (mof::stream_capturing((hipStream_t)stream)) e->graph_pinned.store(true);  // the map and the tables are the engine's
  HIP_TRY(remap(e, lp, interpolation, n_images, (hipStream_t)stream));  // touches no engine scratch
  return MOF_OK;
}

}  // extern "C"
