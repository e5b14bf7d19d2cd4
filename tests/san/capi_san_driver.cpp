// Drives the HOST side of the product library under AddressSanitizer + UndefinedBehaviorSanitizer without a device
// (tests/san/Makefile builds the library's objects with -Xarch_host -fsanitize=..., device code untouched):
//   * every geometry / configuration / argument-validation path of the C ABI that runs before a device is touched,
//   * every entry point on a null engine,
//   * the scale/rotation estimator's host-built tables (cv::logPolar maps in remap's fixed point, cubic / Lanczos4
//     weight tables), compared entry by entry with the oracle's tables,
//   * the geometry tail's host forms (getRT / get2DT and their stages),
//   * the estimator's create-time route (sr_route) for every even resolution against tests/golden/sr_route_table.txt, recorded from the
//     code before SrRoute existed, and the one list of tuned transform sizes seen through each of its three users,
//   * the FFT engine's create-time route (fft_route) for both peak models, every patch size 2 .. 1000 and every recorded knob setting
//     against tests/golden/fft_route_table.txt, recorded from the code before fft_route was a pure function; what the route carries
//     for its users; and the half-tile kernel's two size lists seen through each of their users,
//   * the block matchers' route (bm_route) and the log-polar remap's route and per-call plan (sr_lp_route, sr_lp_plan) against
//     tests/golden/bm_route_table.txt and sr_lp_route_table.txt, recorded from the launchers before the routes existed, and
//     mof_bm_scan_plan as the projection of the route,
//   * the engines' resource owners (csrc/dev_mem.hpp) and the scratch-growth guard (csrc/capi_graph.hpp) with stub callables.
// Where a device IS present the create() calls succeed and the engines are destroyed again.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "capi_graph.hpp"
#include "mof.h"
#include "mof_kernels.h"
#include "sr_common.hpp"
extern "C" {
#include "oracle.h"
}

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "check failed: %s (line %d): %s\n", #cond, __LINE__, mof_last_error()); return 1; } } while (0)

int main() {
  std::printf("%s, devices: %d\n", mof_version(), mof_device_count());
  // ---- FftMethod geometry (FftMethod.cpp:1706-1720) ----
  mof_fft_config fc;
  for (int fs = 2; fs < 700; fs += 37)
    for (int sps : {1, 32, 64, 120, 128, 481}) {
      CHECK(mof_fft_config_reference(&fc, fs, sps, 80.0) == MOF_OK);
      const int even = fs - (fs & 1);
      CHECK(fc.frame_width == even && fc.grid_x == fc.grid_y && fc.grid_x * fc.patch_size == even);
    }
  CHECK(mof_fft_config_reference(nullptr, 480, 120, 80) == MOF_ERR_BAD_ARG);
  CHECK(mof_fft_config_reference(&fc, 1, 120, 80) == MOF_ERR_BAD_ARG);
  mof_fft_engine* fe = nullptr;
  CHECK(mof_fft_config_reference(&fc, 480, 120, 80.0) == MOF_OK);
  mof_fft_config bad = fc;
  bad.patch_size = 1000;  // pads to 1000: beyond the planned transforms
  bad.frame_width = bad.frame_height = 4000;
  CHECK(mof_fft_create(&bad, &fe) == MOF_ERR_UNSUPPORTED && fe == nullptr && std::strlen(mof_last_error()) > 0);
  bad = fc; bad.patch_size = 62; bad.peak_model = MOF_PEAK_OCL;  // 62 = 2 * 31: no OpenCL plan in the reference either
  CHECK(mof_fft_create(&bad, &fe) == MOF_ERR_UNSUPPORTED && fe == nullptr);
  bad = fc; bad.patch_size = 1;
  CHECK(mof_fft_create(&bad, &fe) == MOF_ERR_BAD_ARG && fe == nullptr);
  bad = fc; bad.grid_x = 5;
  CHECK(mof_fft_create(&bad, &fe) == MOF_ERR_BAD_ARG);
  bad = fc; bad.max_px_speed = NAN;
  CHECK(mof_fft_create(&bad, &fe) == MOF_ERR_BAD_ARG);
  bad = fc; bad.peak_model = 9;
  CHECK(mof_fft_create(&bad, &fe) == MOF_ERR_BAD_ARG);
  bad = fc; bad.device = 1 << 20;
  { const int rc = mof_fft_create(&bad, &fe); CHECK(rc == MOF_ERR_BAD_ARG || rc == MOF_ERR_NO_DEVICE); }
  CHECK(mof_fft_create(nullptr, &fe) == MOF_ERR_BAD_ARG && mof_fft_create(&fc, nullptr) == MOF_ERR_BAD_ARG);
  { const int rc = mof_fft_create(&fc, &fe); CHECK(rc == MOF_OK || rc == MOF_ERR_NO_DEVICE); if (rc == MOF_OK) mof_fft_destroy(fe); }
  uint8_t px[16] = {0};
  double d2[2];
  int ninv;
  CHECK(mof_fft_set_prev(nullptr, px, 4) == MOF_ERR_NOT_INIT && mof_fft_reset(nullptr) == MOF_ERR_NOT_INIT);
  CHECK(mof_fft_process(nullptr, px, 4, d2, &ninv) == MOF_ERR_NOT_INIT && mof_fft_sync(nullptr) == MOF_ERR_NOT_INIT);
  CHECK(mof_fft_process_long_range(nullptr, px, 4, d2, &ninv) == MOF_ERR_NOT_INIT && mof_fft_long_range_patches(nullptr) == MOF_ERR_NOT_INIT);
  CHECK(mof_fft_process_batch_device(nullptr, px, 0, px, 0, 4, 1, d2, nullptr) == MOF_ERR_NOT_INIT);
  CHECK(mof_fft_process_batch_device_bgr(nullptr, px, 0, px, 0, 4, 1, d2, nullptr) == MOF_ERR_NOT_INIT);
  CHECK(mof_fft_process_long_range_batch_device(nullptr, px, 0, px, 0, 4, 1, d2, nullptr) == MOF_ERR_NOT_INIT);
  CHECK(mof_fft_process_batch_host(nullptr, px, 0, px, 0, 4, 1, d2) == MOF_ERR_NOT_INIT);
  CHECK(mof_fft_process_sequence_device(nullptr, px, 0, 4, 3, d2, nullptr) == MOF_ERR_NOT_INIT);
  CHECK(mof_fft_process_sequence_device_bgr(nullptr, px, 0, 12, 3, d2, nullptr) == MOF_ERR_NOT_INIT);
  CHECK(mof_fft_release_graphs(nullptr) == MOF_ERR_NOT_INIT && mof_fft_graph_pinned(nullptr) == 0);
  CHECK(mof_purge_deferred() == 0 && mof_deferred_count() == 0);
  CHECK(std::strcmp(mof_fft_kernel_variant(nullptr), "") == 0);
  mof_fft_destroy(nullptr);
  // ---- block matching geometry (BlockMethod.cpp:11; FastSpacedBMMethod_OCL.cpp:82-90) ----
  mof_bm_config bc;
  CHECK(mof_bm_config_block_method(&bc, 480, 120, 21) == MOF_OK && bc.grid_x == 3 && bc.low_contrast_rule == 0);
  CHECK(mof_bm_config_fast_spaced(&bc, 752, 480, 16, 8, 16) == MOF_OK && bc.grid_x == 30 && bc.grid_y == 18);
  CHECK(mof_bm_config_fast_spaced(&bc, 752, 480, 120, 24, 21) == MOF_OK && bc.grid_x == 4 && bc.grid_y == 3);
  CHECK(mof_bm_config_block_method(nullptr, 1, 1, 1) == MOF_ERR_BAD_ARG && mof_bm_config_fast_spaced(&bc, 0, 1, 1, 1, 1) == MOF_ERR_BAD_ARG);
  mof_bm_engine* be = nullptr;
  mof_bm_config bbad;
  CHECK(mof_bm_config_fast_spaced(&bbad, 752, 480, 16, 8, 16) == MOF_OK);
  bbad.grid_x = 31;
  CHECK(mof_bm_create(&bbad, &be) == MOF_ERR_BAD_ARG);
  bbad.grid_x = 30; bbad.scan_radius = 0; bbad.block_size = 3;
  CHECK(mof_bm_create(&bbad, &be) == MOF_ERR_UNSUPPORTED);
  int8_t i8[8];
  CHECK(mof_bm_set_prev(nullptr, px, 4) == MOF_ERR_NOT_INIT && mof_bm_reset(nullptr) == MOF_ERR_NOT_INIT);
  CHECK(mof_bm_process(nullptr, px, 4, i8, i8, i8) == MOF_ERR_NOT_INIT && mof_bm_refine(nullptr, 0, 0, 2, 1, d2) == MOF_ERR_NOT_INIT);
  CHECK(mof_bm_process_batch_device(nullptr, px, 0, px, 0, 4, 1, i8, i8, i8, nullptr) == MOF_ERR_NOT_INIT);
  CHECK(mof_bm_process_batch_host(nullptr, px, 0, px, 0, 4, 1, i8, i8, i8) == MOF_ERR_NOT_INIT && mof_bm_sync(nullptr) == MOF_ERR_NOT_INIT);
  CHECK(mof_bm_release_graphs(nullptr) == MOF_ERR_NOT_INIT && mof_bm_graph_pinned(nullptr) == 0);
  mof_bm_destroy(nullptr);
  // ---- scale/rotation estimator: argument paths and the host-built tables against the oracle ----
  mof_sr_engine* se = nullptr;
  mof_sr_config sc{480, 49.9, 0, MOF_LOGPOLAR_CV4, 0, 0};
  mof_sr_config sbad = sc;
  sbad.resolution = 2000;  // pads to 2000: beyond the planned transforms
  CHECK(mof_sr_create(&sbad, &se) == MOF_ERR_UNSUPPORTED);
  sbad.resolution = 101;   // odd
  CHECK(mof_sr_create(&sbad, &se) == MOF_ERR_BAD_ARG);
  sbad = sc; sbad.magnitude = 0;
  CHECK(mof_sr_create(&sbad, &se) == MOF_ERR_BAD_ARG);
  sbad = sc; sbad.logpolar_variant = 2;
  CHECK(mof_sr_create(&sbad, &se) == MOF_ERR_BAD_ARG);
  CHECK(mof_sr_process(nullptr, px, 4, d2) == MOF_ERR_NOT_INIT && mof_sr_reset(nullptr) == MOF_ERR_NOT_INIT);
  CHECK(mof_sr_process_batch_device(nullptr, px, 0, px, 0, 4, 1, d2, nullptr) == MOF_ERR_NOT_INIT);
  CHECK(mof_sr_logpolar_batch_device(nullptr, px, 0, 4, 1, 2, px, nullptr) == MOF_ERR_NOT_INIT);
  {
    int gated = 7;
    CHECK(mof_sr_process_sequence_device(nullptr, px, 0, 4, 3, d2, nullptr, &gated) == MOF_ERR_NOT_INIT);
  }
  CHECK(mof_sr_release_graphs(nullptr) == MOF_ERR_NOT_INIT && mof_sr_graph_pinned(nullptr) == 0 && mof_sr_reserve(nullptr, 1) == MOF_ERR_NOT_INIT);
  mof_sr_destroy(nullptr);
  for (int variant = 0; variant < 2; ++variant)
    for (int res : {240, 256, 480}) {
      const double M = res == 480 ? 49.9 : 40.0;
      const std::vector<mof::SrMapEntry> map = mof::sr_logpolar_map(res, M, variant);
      std::vector<float> mx((size_t)res * res), my((size_t)res * res);
      CHECK(oracle_logpolar_maps(res, M, variant, mx.data(), my.data()) == 0);
      long valid = 0;
      for (size_t i = 0; i < map.size(); ++i) {
        const long ix = std::lrintf(mx[i] * 32.f), iy = std::lrintf(my[i] * 32.f);
        const long ax = ix >> 5, ay = iy >> 5;
        const bool inside = ax >= 0 && ax < res && ay >= 0 && ay < res;
        CHECK((map[i].valid != 0) == inside);
        if (inside) {
          CHECK(map[i].ax == ax && map[i].ay == ay && map[i].widx == (unsigned)((iy & 31) * 32 + (ix & 31)));
          ++valid;
        }
      }
      CHECK(valid > (long)map.size() / 2);
    }
  {
    // weight tables: rows sum to 2^15; remapping a constant image returns the constant (what the oracle does too)
    for (int ks : {4, 8}) {
      const std::vector<int16_t> tab = mof::sr_weight_table(ks);
      CHECK(tab.size() == (size_t)1024 * ks * ks);
      for (int r = 0; r < 1024; ++r) {
        int sum = 0;
        for (int k = 0; k < ks * ks; ++k) sum += tab[(size_t)r * ks * ks + k];
        CHECK(sum == 1 << 15);
      }
    }
  }
  // ---- the estimator's route, decided without a device ----
  {
    std::FILE* f = std::fopen(MOF_GOLDEN_DIR "/sr_route_table.txt", "r");
    CHECK(f != nullptr);
    static const char* const families[] = {"TUNED", "TUNED_PAD", "PLANNED"};
    char line[256], fam[16];
    int rows = 0;
    while (std::fgets(line, sizeof line, f)) {
      if (line[0] == '#') continue;
      int all, res, m, sums, cand;
      size_t off, zh;
      const int got = std::sscanf(line, "%d %d %15s %d %d %zu %zu %d", &all, &res, fam, &m, &sums, &off, &zh, &cand);
      CHECK(got == 3 || got == 8);
      mof::SrKnobs k;
      k.tuned_all = all != 0;
      mof::PcPlan plan{};
      mof::SrRoute r;
      const bool ok = mof::sr_route(res, k, &plan, &r);
      if (got == 3) {
        CHECK(std::strcmp(fam, "unsupported") == 0 && !ok);
      } else {
        CHECK(ok && std::strcmp(fam, families[r.family]) == 0 && r.m == m && r.sums == (sums != 0) && r.sums_off == off);
        CHECK(r.zh_floats == zh && r.candidates == cand && r.seq_run == 0);
        CHECK(r.family == mof::SrRoute::TUNED || (plan.n == res && plan.m == m));
      }
      ++rows;
    }
    std::fclose(f);
    CHECK(rows == 2 * 493);  // even resolutions 16 .. 1000, MOF_SR_TUNED_ALL unset and 0
    // the fixed K6s run follows its knob
    for (int res = 16; res <= 1000; res += 2) {
      mof::SrKnobs k;
      mof::PcPlan plan{};
      mof::SrRoute r;
      k.seq_run = 7;
      if (!mof::sr_route(res, k, &plan, &r)) continue;
      CHECK(r.seq_run == 7);
    }
    // one list of tuned transform sizes, whoever is asked
    int listed = 0;
    for (int m = 2; m <= 1000; ++m) {
      bool exact = false;
      const bool tuned = mof::sr_transform_size_tuned(m, &exact);
      const bool in_list = mof::sr_dispatch_size(m, [](auto) { return hipSuccess; }) == hipSuccess;
      CHECK(tuned == in_list && tuned == (mof::sr_seq_columns_per_wave(m) != 0));
      listed += tuned;
    }
    CHECK(listed == 50);
  }
  // ---- the FFT engine's route, decided without a device: every (knob setting, peak model, patch size) of the recorded table ----
  {
    struct Row {
      bool ok = false;
      char fam[16] = "", video[16] = "";
      int m = 0, half_m = 0, video_m = 0, large_tuned = 0, odd_tail = 0, large_video = 0;
      bool same(const Row& o) const {
        return ok == o.ok && !std::strcmp(fam, o.fam) && !std::strcmp(video, o.video) && m == o.m && half_m == o.half_m && video_m == o.video_m &&
               large_tuned == o.large_tuned && odd_tail == o.odd_tail && large_video == o.large_video;
      }
    };
    struct Section { std::string label; mof::FftKnobs k; std::map<std::pair<int, int>, Row> rows; };
    std::vector<Section> sections;
    std::FILE* f = std::fopen(MOF_GOLDEN_DIR "/fft_route_table.txt", "r");
    CHECK(f != nullptr);
    char line[512];
    int rows = 0;
    while (std::fgets(line, sizeof line, f)) {
      if (line[0] == '#') continue;
      if (std::strncmp(line, "knobs ", 6) == 0) {
        // the knobs of a label, by the rules fft_knobs() reads the environment with
        Section s;
        s.label = std::string(line + 6, std::strcspn(line + 6, "\n"));
        for (size_t at = 0; s.label != "default" && at < s.label.size();) {
          const size_t eq = s.label.find('=', at), end = std::min(s.label.find(',', at), s.label.size());
          CHECK(eq != std::string::npos && eq < end);
          const std::string name = s.label.substr(at, eq - at);
          const int v = std::atoi(s.label.c_str() + eq + 1);
          if (name == "MOF_FFT_HALF") s.k.half = v;
          else if (name == "MOF_FFT_FORCE_PLANNED") s.k.force_planned = true;
          else if (name == "MOF_FFT_FORCE_LARGE") s.k.force_large = true;
          else if (name == "MOF_FFT_SEQ_PAIRS") s.k.seq_pairs = true;
          else if (name == "MOF_FFT_SEQ_HALF128") s.k.seq_half128 = true;
          else if (name == "MOF_FFT_HALF_SEQ") s.k.half_seq_off = v == 0;
          else if (name == "MOF_FFT_LARGE_TUNED") s.k.large_tuned = v != 0;
          else if (name == "MOF_FFT_LARGE_VIDEO") s.k.large_video = v != 0;
          else if (name == "MOF_FFT_SEQ_RUN") s.k.seq_run = v >= 1 ? v : 0;
          else if (name == "MOF_FFT_LARGE_PASS") s.k.large_pass = v > 0 ? v : 0;
          else if (name == "MOF_PLANNED_STATIC") s.k.planned_static = v != 0;
          else CHECK(!"a knob the driver does not know");
          at = end + 1;
        }
        sections.push_back(s);
        continue;
      }
      CHECK(!sections.empty());
      Row r;
      int model, n;
      const int got = std::sscanf(line, "%d %d %15s %d %d %15s %d %d %d %d", &model, &n, r.fam, &r.m, &r.half_m, r.video, &r.video_m, &r.large_tuned,
                                  &r.odd_tail, &r.large_video);
      CHECK((got == 3 && std::strcmp(r.fam, "unsupported") == 0) || got == 10);
      r.ok = got == 10;
      CHECK((model == 0 || model == 1) && n >= 2 && n <= 1000 && sections.back().rows.emplace(std::make_pair(model, n), r).second);
      ++rows;
    }
    std::fclose(f);
    CHECK(sections.size() == 15 && sections[0].label == "default" && sections[0].rows.size() == 2 * 999 && rows == 6097);
    static const char* const families[] = {"TUNED", "PLANNED", "LARGE"};
    static const char* const videos[] = {"PAIRS", "SEQ", "SEQ_HALF", "HALF_SEQ"};
    static const int min_runs[] = {0, 2, 16, 4};
    int supported[2] = {0, 0};
    for (const Section& s : sections)
      for (int model = 0; model <= 1; ++model)
        for (int n = 2; n <= 1000; ++n) {
          const auto key = std::make_pair(model, n);
          const auto own = s.rows.find(key);
          const Row& want = own != s.rows.end() ? own->second : sections[0].rows.at(key);  // (no row under a label: the default's)
          CHECK(&s == &sections[0] || own == s.rows.end() || !want.same(sections[0].rows.at(key)));  // (listed: it differs)
          mof::PcPlan plan{};
          mof::FftRoute r;
          const bool ok = mof::fft_route(n, model, s.k, &plan, &r);
          if (&s == &sections[0]) {
            // `unsupported` is what create answers: no plan, or a size the OpenCL model cannot plan (a status that no knob changes)
            mof_fft_config c;
            mof_fft_engine* e = nullptr;
            CHECK(mof_fft_config_reference(&c, 480, 120, 80.0) == MOF_OK);
            c.frame_width = c.frame_height = c.stride_x = c.stride_y = c.patch_size = n;
            c.grid_x = c.grid_y = 1;
            c.peak_model = model;
            const int rc = mof_fft_create(&c, &e);
            CHECK(want.ok ? (rc == MOF_OK || rc == MOF_ERR_NO_DEVICE) : (rc == MOF_ERR_UNSUPPORTED && e == nullptr));
            if (rc == MOF_OK) mof_fft_destroy(e);
            supported[model] += want.ok;
          }
          if (!want.ok) {
            CHECK(model == MOF_PEAK_OCL || !ok);
            continue;
          }
          CHECK(ok && std::strcmp(want.fam, families[r.family]) == 0 && r.m == want.m && r.half_m == want.half_m);
          CHECK(std::strcmp(want.video, videos[r.video]) == 0 && r.video_m == want.video_m);
          CHECK(r.large_tuned == (want.large_tuned != 0) && r.odd_tail == (want.odd_tail != 0) && r.large_video == (want.large_video != 0));
          CHECK(r.family == mof::FftRoute::TUNED || (plan.n == n && plan.m == want.m));
          // what the route carries for its users follows the route and the knobs
          const char* variant = r.half_m > 0 ? "planned-half" : r.family == mof::FftRoute::LARGE ? "planned-large" : r.family == mof::FftRoute::PLANNED ? "planned" : "stockham";
          CHECK(std::strcmp(r.variant, variant) == 0 && r.min_run == min_runs[r.video]);
          CHECK(r.seq_run == s.k.seq_run && r.large_pass == s.k.large_pass && r.planned_static == s.k.planned_static);
        }
    CHECK(supported[0] == 959 && supported[1] == 65);
    for (int n = 2; n <= 960; ++n) {
      mof::FftKnobs k;
      mof::PcPlan plan{};
      mof::FftRoute r;
      CHECK(mof::fft_route(n, MOF_PEAK_OPENCV, k, &plan, &r) && r.seq_run == 0 && r.large_pass == 0 && r.planned_static);
      k.seq_run = 7;
      k.large_pass = 5;
      k.planned_static = false;
      CHECK(mof::fft_route(n, MOF_PEAK_OPENCV, k, &plan, &r) && r.seq_run == 7 && r.large_pass == 5 && !r.planned_static);
    }
    // the half-tile kernel's two size lists, whoever is asked
    int pair = 0, video = 0, planned = 0;
    for (int m = 2; m <= 1000; ++m) {
      const bool p = mof::pc_half_supported(m), v = mof::pc_half_sequence_supported(m), w = mof::pc_half_workgroups_per_cu(m) > 0;
      CHECK(w == (p || v) && (p || !v || m == 50 || m == 54 || m == 108) && (v || !p || m == 162));
      pair += p;
      video += v;
      planned += w;
    }
    CHECK(pair == 14 && video == 16 && planned == 17);
  }
  // ---- the block matchers' route, decided without a device: every (knob setting, geometry) of the recorded table, every field ----
  {
    std::FILE* f = std::fopen(MOF_GOLDEN_DIR "/bm_route_table.txt", "r");
    CHECK(f != nullptr);
    auto project = [](const mof::BmRoute& r, bool quality, int out[4]) {
      const mof::BmRoute::Form& p = quality ? r.q : r.plain;
      if (r.scan16) out[0] = 1, out[1] = r.bpw, out[2] = 64, out[3] = (int)r.lds + (quality ? 256 : 0);
      else out[0] = 0, out[1] = p.bpw, out[2] = p.threads, out[3] = (int)p.lds;
    };
    mof::BmKnobs k;
    bool is_default = false;
    int sections = 0, rows = 0, kinds[4] = {0, 0, 0, 0};
    char line[256];
    while (std::fgets(line, sizeof line, f)) {
      if (line[0] == '#') continue;
      if (std::strncmp(line, "knobs ", 6) == 0) {
        const std::string label(line + 6, std::strcspn(line + 6, "\n"));
        const size_t eq = label.find('=');
        const int v = eq == std::string::npos ? 0 : std::atoi(label.c_str() + eq + 1);
        k = mof::BmKnobs{};
        is_default = label == "default";
        if (is_default) {}
        else if (label.rfind("MOF_BM_GENERIC=", 0) == 0) k.generic = true;
        else if (label.rfind("MOF_BM_XB=", 0) == 0) k.xb = v;
        else if (label.rfind("MOF_BM_BPW=", 0) == 0) k.bpw = v;
        else if (label.rfind("MOF_BM_G=", 0) == 0) k.g = v;
        else CHECK(!"a knob the driver does not know");
        ++sections;
        continue;
      }
      int b, s, r, gx, at = 0;
      char kind;
      CHECK(sections > 0 && std::sscanf(line, "%d %d %d %d %c%n", &b, &s, &r, &gx, &kind, &at) == 5);
      const char* rest = line + at;
      mof::BmRoute rt;
      const bool ok = mof::bm_route(b, s, r, gx, k, &rt);
      int plain[4] = {-1, -1, -1, -1}, q[4] = {-1, -1, -1, -1};
      if (ok) project(rt, false, plain), project(rt, true, q);
      if (kind == 'N') {
        CHECK(!ok);
        ++kinds[0];
      } else if (kind == 'S') {
        int bpw, wpr, sd;
        size_t lds, ldsq;
        CHECK(std::sscanf(rest, "%d %d %d %zu %zu", &bpw, &wpr, &sd, &lds, &ldsq) == 5);
        CHECK(ok && rt.scan16 && gx > 0 && rt.bpw == bpw && rt.waves_per_row == wpr && rt.strip_dwords == sd && rt.lds == lds && ldsq == lds + 256);
        CHECK(q[3] == (int)ldsq && !k.generic);
        ++kinds[1];
      } else if (kind == 'G') {
        int xb, G, bpw, wpd, slot, thr, grid, bpwq, thrq, gridq;
        size_t lds, ldsq;
        char cost[32], mine[32];
        CHECK(std::sscanf(rest, "%d %d %d %d %d %d %zu %d %31s %d %d %zu %d", &xb, &G, &bpw, &wpd, &slot, &thr, &lds, &grid, cost, &bpwq, &thrq, &ldsq, &gridq) == 13);
        CHECK(ok && !rt.scan16 && rt.xb == xb && (rt.g == 6 || rt.g == 7 || rt.g == 10 ? rt.g : 8) == G && (k.g == 0 || rt.g == k.g));
        CHECK(rt.plain.bpw == bpw && rt.plain.wpd == wpd && rt.plain.slot_dwords == slot && rt.plain.threads == thr && rt.plain.lds == lds);
        CHECK(rt.q.bpw == bpwq && rt.q.wpd == wpd && rt.q.slot_dwords == slot && rt.q.threads == thrq && rt.q.lds == ldsq && rt.q.cost == rt.plain.cost);
        CHECK((gx + bpw - 1) / bpw == grid && (gx + bpwq - 1) / bpwq == gridq);
        std::snprintf(mine, sizeof mine, "%.9g", rt.plain.cost);
        CHECK(std::strcmp(mine, cost) == 0);
        ++kinds[2];
      } else {
        int o[4], oq[4];
        CHECK(kind == 'P' && gx == 0 && std::sscanf(rest, "%d %d %d %d %d %d %d %d", &o[0], &o[1], &o[2], &o[3], &oq[0], &oq[1], &oq[2], &oq[3]) == 8);
        CHECK(ok && !rt.scan16 && std::memcmp(o, plain, sizeof o) == 0 && std::memcmp(oq, q, sizeof oq) == 0);
        ++kinds[3];
      }
      CHECK(rt.verbose == false);
      if (is_default) {
        // what mof_bm_scan_plan reports is the route's projection (this process runs with no MOF_BM_* set); no plan: create's refusal
        int got[4] = {-1, -1, -1, -1};
        const int rc = mof_bm_scan_plan(b, s, r, gx, 0, got);
        CHECK(ok ? (rc == MOF_OK && std::memcmp(got, plain, sizeof got) == 0) : rc == MOF_ERR_BAD_ARG);
        CHECK(mof_bm_scan_plan(b, s, r, gx, 1, got) == rc && (!ok || std::memcmp(got, q, sizeof got) == 0));
      }
      ++rows;
    }
    std::fclose(f);
    CHECK(sections == 9 && rows == 2845 && kinds[0] == 160 && kinds[1] == 247 && kinds[2] == 2422 && kinds[3] == 16);
    // the one plan family that fills the LDS: with two groups of x-shifts per lane 7 blocks take 163 828 bytes, the quality form takes 6
    for (int gx : {7, 13, 14, 28}) {
      mof::BmKnobs k2;
      k2.xb = 2;
      mof::BmRoute rt;
      CHECK(mof::bm_route(100, 0, 4, gx, k2, &rt) && !rt.scan16 && rt.xb == 2);
      CHECK(rt.plain.bpw == 7 && rt.plain.threads == 128 && rt.plain.lds == 163828 && rt.plain.lds + 4 * 7 > 160 * 1024);
      CHECK(rt.q.bpw == 6 && rt.q.threads == 128 && rt.q.lds == (163828 - 12 * 7) / 7 * 6 + 16 * 6 && rt.q.lds <= 160 * 1024);
    }
    mof::BmKnobs kv;
    kv.verbose = true;
    mof::BmRoute rv;
    CHECK(mof::bm_route(32, 0, 8, 8, kv, &rv) && rv.verbose);
  }
  // ---- the log-polar remap's route and plan, decided without a device: every row of the recorded table ----
  {
    std::FILE* f = std::fopen(MOF_GOLDEN_DIR "/sr_lp_route_table.txt", "r");
    CHECK(f != nullptr);
    static const char* const forms[] = {"PIXEL", "TABLE", "WAVE", "SUPER"};
    static const int ns[] = {1, 3, 4, 5, 15, 16, 63, 64, 127, 128, 1024};
    mof::SrKnobs k;
    bool is_default = false;
    int sections = 0, rows = 0, boxes_checked = 0;
    char line[256];
    while (std::fgets(line, sizeof line, f)) {
      if (line[0] == '#') continue;
      if (std::strncmp(line, "knobs ", 6) == 0) {
        // the knobs of a label, by the rules sr_knobs() reads the environment with
        const std::string label(line + 6, std::strcspn(line + 6, "\n"));
        const size_t eq = label.find('=');
        const int v = eq == std::string::npos ? 0 : std::atoi(label.c_str() + eq + 1);
        k = mof::SrKnobs{};
        is_default = label == "default";
        if (is_default) {}
        else if (label.rfind("MOF_SR_LP_GLOBAL=", 0) == 0) k.lp_global = v != 0;
        else if (label.rfind("MOF_SR_LP_STAGED=", 0) == 0) k.lp_staged = v != 0;
        else if (label.rfind("MOF_SR_LP_SUPER=", 0) == 0) k.lp_super = v != 0;
        else if (label.rfind("MOF_SR_LP_RING=", 0) == 0) k.lp_long_ring = v == 16;
        else if (label.rfind("MOF_SR_LP_XCD=", 0) == 0) k.lp_xcd = v != 0;
        else if (label.rfind("MOF_SR_LP_IPW=", 0) == 0) k.lp_ipw = v;
        else CHECK(!"a knob the driver does not know");
        ++sections;
        continue;
      }
      int res, interp, boxdw, sboxdw, has_sb, ring;
      double M;
      size_t lds;
      char form[16];
      unsigned long long want = 0;
      CHECK(sections > 0 && std::sscanf(line, "%d %lf %d %d %d %d %15s %d %zu %llx", &res, &M, &interp, &boxdw, &sboxdw, &has_sb, form, &ring, &lds, &want) == 10);
      if (is_default && (res <= 64 || res == 240 || res == 480)) {
        // the recorded box sizes are what create computes
        int bytes = 0;
        const std::vector<mof::SrMapEntry> map = mof::sr_logpolar_map(res, M, 0);
        mof::sr_tile_boxes(map, res, interp == 2 ? 4 : 8, &bytes, 8);
        CHECK(bytes / 4 == boxdw && has_sb == (res % 16 == 0));
        if (has_sb) {
          mof::sr_tile_boxes(map, res, interp == 2 ? 4 : 8, &bytes, 16);
          CHECK(bytes / 4 == sboxdw);
        }
        ++boxes_checked;
      }
      const mof::SrLpRoute r = mof::sr_lp_route(res, boxdw, sboxdw, has_sb != 0, interp, k);
      CHECK(std::strcmp(forms[r.form], form) == 0 && r.ring == ring && r.lds == lds && r.res == res && r.interp == interp);
      CHECK(r.ipw == k.lp_ipw && r.xcd == k.lp_xcd);
      const unsigned pixel_grid = (unsigned)(((res + 31) / 32) * ((res + 7) / 8));
      std::string text;
      for (int n : ns)
        for (int aligned = 1; aligned >= 0; --aligned) {
          const mof::SrLpPlan p = mof::sr_lp_plan(r, n, aligned != 0);
          char buf[160];
          std::snprintf(buf, sizeof buf, "n%d a%d:", n, aligned);
          text += buf;
          if (p.form == mof::SrLpRoute::SUPER || p.form == mof::SrLpRoute::WAVE) {
            CHECK(p.form == r.form && p.n_st == (aligned ? n : n - 1) && p.last_pixel == !aligned);
            std::snprintf(buf, sizeof buf, " %c%d g%u l%zu n%d i%d x%d", p.form == mof::SrLpRoute::SUPER ? 'S' : 'W', r.ring, (unsigned)p.grid, r.lds, p.n_st, p.ipw,
                          p.xcd_groups);
            text += buf;
            if (p.last_pixel) {
              std::snprintf(buf, sizeof buf, " P g%u,1 s%d", pixel_grid, p.n_st);
              text += buf;
            }
          } else if (p.form == mof::SrLpRoute::TABLE) {
            CHECK(p.n_st == n && !p.last_pixel);
            std::snprintf(buf, sizeof buf, " T g%u n%d", (unsigned)(p.grid < 256 ? p.grid : 256), n);  // (recorded with 256 CUs)
            text += buf;
          } else {
            CHECK(p.n_st == n && !p.last_pixel && p.grid == (long)pixel_grid);
            std::snprintf(buf, sizeof buf, " P g%u,%d s0", pixel_grid, n);
            text += buf;
          }
          text += ";";
        }
      unsigned long long h = 1469598103934665603ull;
      for (unsigned char c : text) h = (h ^ c) * 1099511628211ull;
      if (h != want) std::fprintf(stderr, "remap plan of res %d M %g interp %d differs from the record: %s\n", res, M, interp, text.c_str());
      CHECK(h == want);
      ++rows;
    }
    std::fclose(f);
    CHECK(sections == 7 && rows == 2836 && boxes_checked > 100);
  }
  // ---- geometry tail, host forms ----
  {
    const mof_geom_camera cam{340, 338.5, 376, 240, -0.28, 0.07, 0.0004, -0.0003, -0.006};
    const oracle_camera ocam{340, 338.5, 376, 240, -0.28, 0.07, 0.0004, -0.0003, -0.006};
    mof_geom_layout L;
    CHECK(mof_geom_layout_reference(&L, 480, 120) == MOF_OK && L.grid_x == 4);
    CHECK(mof_geom_layout_reference(&L, 100, 120) == MOF_ERR_BAD_ARG);
    CHECK(mof_geom_layout_reference(&L, 480, 120) == MOF_OK);
    const oracle_geom_layout OL{4, 4, 0, 0, 120, 120, 120};
    double shifts[32], out[7], wout[7], H[9], o6[6], w6[6];
    uint8_t mask[16];
    for (int i = 0; i < 16; ++i) { shifts[2 * i] = 3.0 + 0.01 * (i % 4); shifts[2 * i + 1] = -2.0 + 0.02 * (i / 4); }
    shifts[10] = NAN;
    shifts[14] = 55.0;
    mof_geom_rt_params p{2.5, 0.02, 136.0, {0, 0, 0, 1}, {0, 0, 0, 1}, {0, 0, 0}};
    oracle_rt_params op{2.5, 0.02, 136.0, {0, 0, 0, 1}, {0, 0, 0, 1}, {0, 0, 0}};
    oracle_quat_from_rpy(0.01, -0.02, 0.3, p.ang_rate_q);
    std::memcpy(op.ang_rate_q, p.ang_rate_q, sizeof(op.ang_rate_q));
    int status = -1;
    for (int thr = -1; thr <= 17; thr += 3) {
      CHECK(mof_geom_get_rt(shifts, &L, &cam, &p, thr, out, &status, mask, H) == MOF_OK);
      CHECK(status == oracle_get_rt(shifts, &OL, &ocam, &op, thr, wout, nullptr, nullptr));
      for (int k = 0; k < 7; ++k) CHECK(std::fabs(out[k] - wout[k]) <= 1e-9);
    }
    CHECK(mof_geom_get_rt(shifts, &L, &cam, &p, 8, out, &status, nullptr, nullptr) == MOF_OK);
    CHECK(mof_geom_get_rt(nullptr, &L, &cam, &p, 8, out, &status, nullptr, nullptr) == MOF_ERR_BAD_ARG);
    mof_geom_layout big = L;
    big.grid_x = 64; big.grid_y = 32;
    CHECK(mof_geom_get_rt(shifts, &big, &cam, &p, 8, out, &status, nullptr, nullptr) == MOF_ERR_BAD_ARG);
    const mof_geom_2dt_params p2{2.0, 0.02, 0.1, -0.2, 1.0};
    const oracle_2dt_params op2{2.0, 0.02, 0.1, -0.2, 1.0};
    CHECK(mof_geom_get_2dt(shifts, &L, &cam, &p2, o6, &status) == MOF_OK && status == oracle_get_2dt(shifts, &OL, &ocam, &op2, w6));
    CHECK(std::memcmp(o6, w6, sizeof(o6)) == 0);
    double pts[6] = {0, 0, 240, 240, 479, 479}, und[6];
    CHECK(mof_geom_undistort_points(&cam, 136.0, pts, 3, und) == MOF_OK && mof_geom_undistort_points(&cam, 0, nullptr, 0, nullptr) == MOF_OK);
    double R[36], t[12], nn[12];
    int nsol = -1;
    const double Hid[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    CHECK(mof_geom_decompose_homography(Hid, R, t, nn, &nsol) == MOF_OK && nsol == 1);
    int found = -1;
    double a[8] = {0, 0, 1, 0, 1, 1, 0, 1}, b[8] = {0.1, 0, 1.1, 0.05, 1.2, 1.1, 0, 0.9};
    CHECK(mof_geom_find_homography(a, b, 4, H, mask, &found) == MOF_OK && found == 1);
    CHECK(mof_geom_find_homography(a, b, 3, H, mask, &found) == MOF_OK && found == 0);
    CHECK(mof_geom_find_homography(a, b, -1, H, mask, &found) == MOF_ERR_BAD_ARG);
    // the batched forms refuse null device pointers before any launch
    CHECK(mof_geom_get_rt_batch_device(nullptr, &L, &cam, nullptr, 3, 8, nullptr, nullptr) == MOF_ERR_BAD_ARG);
    CHECK(mof_geom_get_2dt_batch_device(nullptr, &L, &cam, nullptr, 3, nullptr, nullptr) == MOF_ERR_BAD_ARG);
    CHECK(mof_geom_get_rt_batch_device(nullptr, &L, &cam, nullptr, 0, 8, nullptr, nullptr) == MOF_OK);
  }
  // ---- the engines' owners and the one growth guard (dev_mem.hpp, capi_graph.hpp) ----
  {
    static_assert(!std::is_copy_constructible<mof::DevMem<float>>::value && !std::is_copy_assignable<mof::PinnedMem<double>>::value &&
                  !std::is_copy_constructible<mof::Stream>::value && !std::is_copy_constructible<mof::Event>::value, "owners are move-only");
    const int live0 = mof_live_buffers();
    {
      mof::DevMem<float> d, d2;
      mof::PinnedMem<double> h;
      mof::Stream s;
      mof::Event ev;
      d.reset();  // empty owners: reset and the destructors do nothing
      const bool device = mof_device_count() > 0;
      CHECK((d.alloc(64) == hipSuccess) == device && (d.get() != nullptr) == device);
      CHECK((h.alloc(64) == hipSuccess) == device && (h.get() != nullptr) == device);
      CHECK((s.create() == hipSuccess) == device && (ev.create() == hipSuccess) == device && (s.get() != nullptr) == device);
      CHECK(mof_live_buffers() == live0 + (device ? 2 : 0));
      float* raw = d.get();
      d2 = std::move(d);  // the source is left empty, nothing is released
      CHECK(d.get() == nullptr && d2.get() == raw && mof_live_buffers() == live0 + (device ? 2 : 0));
      mof::DevMem<float> d3(std::move(d2));
      CHECK(d2.get() == nullptr && d3.get() == raw);
      CHECK((mof::upload(d, std::vector<float>(16, 2.f), s) == hipSuccess) == device);
      d3.reset();
      d3.reset();
      CHECK(d3.get() == nullptr);
    }
    CHECK(mof_live_buffers() == live0);
    mof::ScratchFence fence;
    std::vector<long> asked;
    auto realloc = [&asked](long n) { asked.push_back(n); return n == 1 ? hipSuccess : hipErrorOutOfMemory; };
    CHECK(mof::grow_scratch(true, fence, {}, true, "scratch", 4, 4, 1, realloc) == MOF_OK && asked.empty());
    CHECK(mof::grow_scratch(true, fence, {}, false, "scratch", 4, 8, 1, realloc) == MOF_ERR_BUSY && std::strstr(mof_last_error(), "graph") && asked.empty());
    CHECK(mof::grow_scratch(false, fence, {}, true, "scratch", 4, 8, 1, realloc) == MOF_ERR_BAD_ARG && std::strstr(mof_last_error(), "graph") && asked.empty());
    CHECK(mof::grow_scratch(false, fence, {}, false, "scratch", 4, 8, 1, realloc) == MOF_ERR_NO_MEMORY && asked == std::vector<long>({8, 1}));
    CHECK(mof::grow_scratch(false, fence, {}, false, "scratch", 0, 1, 1, realloc) == MOF_OK && asked == std::vector<long>({8, 1, 1}));
  }
  std::printf("C-ABI sanitizer driver: ok\n");
  return 0;
}
