// Host-side C++ test driver for the window-offset methods of mof::FftMethod (include/mof/processors.hpp): reservePred,
// processBatchDevicePred, processCoarseToFineBatchDevice, processImageCoarseToFine. Reads raw u8 frames (all current frames, then all
// previous ones), predicts (px, py) for every patch, runs each method and the C ABI entry it mirrors (on a second engine) and compares
// their bytes; every value is printed with 17 digits, tests/test_gpu_cpp_pred.py compares them with the Python binding's bits.
//   usage: test_pred <frame_size> <patch_size> <max_px_speed> <px> <py> <npairs> <file>
//   prints: pred k  then per patch <x> <y> <response> <peak> <ax> <ay>
//           c2f k   then per patch <x> <y> <ax> <ay>
//           coarse k then per long-range patch <x> <y>
//           image k invalid <n> then per patch <x> <y>
//           abi <same | what differs>
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "mof/processors.hpp"

static void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  explicit DevBuf(size_t count) : n(count) { hip_check(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)), "hipMalloc"); }
  ~DevBuf() { (void)hipFree(p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  void up(const T* src) { hip_check(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice), "upload"); }
  std::vector<T> down() const {
    std::vector<T> v(n);
    hip_check(hipDeviceSynchronize(), "sync");
    hip_check(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost), "download");
    return v;
  }
};

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

int main(int argc, char** argv) {
  if (argc < 8) {
    std::fprintf(stderr, "usage: test_pred <frame_size> <patch_size> <max_px_speed> <px> <py> <npairs> <file>\n");
    return 2;
  }
  try {
    const int fs = std::atoi(argv[1]), n = std::atoi(argv[2]), px = std::atoi(argv[4]), py = std::atoi(argv[5]), pairs = std::atoi(argv[6]);
    const double speed = std::atof(argv[3]);
    const size_t fb = (size_t)fs * fs;
    std::vector<uint8_t> frames(fb * 2 * pairs);
    FILE* f = std::fopen(argv[7], "rb");
    if (!f || std::fread(frames.data(), 1, frames.size(), f) != frames.size()) throw std::runtime_error("cannot read the frames");
    std::fclose(f);
    mof::FftMethod fm(fs, n, speed);
    const mof_fft_config cfg = fm.config();
    const size_t patches = (size_t)cfg.grid_x * cfg.grid_y, total = patches * pairs;
    const int n_lr = mof_fft_long_range_patches(fm.handle());
    if (n_lr < 1) throw std::runtime_error("the geometry has no long-range form");
    mof_fft_engine* abi = nullptr;  // the C ABI's side of every comparison runs on an engine of its own
    if (mof_fft_create(&cfg, &abi) != MOF_OK) throw std::runtime_error(mof_last_error());
    std::string differs;

    DevBuf<uint8_t> d_cur(fb * pairs), d_prev(fb * pairs);
    d_cur.up(frames.data());
    d_prev.up(frames.data() + fb * pairs);
    std::vector<int32_t> pred(2 * total);
    for (size_t i = 0; i < total; ++i) {
      pred[2 * i] = px;
      pred[2 * i + 1] = py;
    }
    DevBuf<int32_t> d_pred(2 * total), d_applied(2 * total), d_applied2(2 * total);
    d_pred.up(pred.data());
    DevBuf<double> d_out(2 * total), d_q(2 * total), d_coarse(2 * (size_t)n_lr * pairs), d_out2(2 * total), d_q2(2 * total),
        d_coarse2(2 * (size_t)n_lr * pairs);

    fm.reservePred(pairs);
    fm.processBatchDevicePred(d_cur.p, fb, d_prev.p, fb, (size_t)fs, pairs, d_pred.p, d_out.p, d_q.p, d_applied.p);
    if (mof_fft_process_batch_device_pred(abi, d_cur.p, fb, d_prev.p, fb, (size_t)fs, pairs, d_pred.p, d_out2.p, d_q2.p, d_applied2.p, nullptr) != MOF_OK)
      throw std::runtime_error(mof_last_error());
    {
      const std::vector<double> out = d_out.down(), q = d_q.down();
      const std::vector<int32_t> a = d_applied.down();
      if (!same(out, d_out2.down()) || !same(q, d_q2.down()) || !same(a, d_applied2.down())) differs += " processBatchDevicePred";
      for (int k = 0; k < pairs; ++k) {
        std::printf("pred %d", k);
        for (size_t p = k * patches; p < (k + 1) * patches; ++p)
          std::printf(" %.17g %.17g %.17g %.17g %d %d", out[2 * p], out[2 * p + 1], q[2 * p], q[2 * p + 1], a[2 * p], a[2 * p + 1]);
        std::printf("\n");
      }
    }

    fm.processCoarseToFineBatchDevice(d_cur.p, fb, d_prev.p, fb, (size_t)fs, pairs, d_out.p, nullptr, d_applied.p, d_coarse.p);
    if (mof_fft_process_coarse_to_fine_batch_device(abi, d_cur.p, fb, d_prev.p, fb, (size_t)fs, pairs, d_out2.p, nullptr, d_applied2.p, d_coarse2.p,
                                                    nullptr) != MOF_OK)
      throw std::runtime_error(mof_last_error());
    {
      const std::vector<double> out = d_out.down(), coarse = d_coarse.down();
      const std::vector<int32_t> a = d_applied.down();
      if (!same(out, d_out2.down()) || !same(coarse, d_coarse2.down()) || !same(a, d_applied2.down())) differs += " processCoarseToFineBatchDevice";
      for (int k = 0; k < pairs; ++k) {
        std::printf("c2f %d", k);
        for (size_t p = k * patches; p < (k + 1) * patches; ++p) std::printf(" %.17g %.17g %d %d", out[2 * p], out[2 * p + 1], a[2 * p], a[2 * p + 1]);
        std::printf("\ncoarse %d", k);
        for (size_t p = (size_t)k * n_lr; p < (size_t)(k + 1) * n_lr; ++p) std::printf(" %.17g %.17g", coarse[2 * p], coarse[2 * p + 1]);
        std::printf("\n");
      }
    }

    // the stateful method: previous, then current, of every pair -- the chain runs through all of them
    for (int k = 0; k < pairs; ++k) {
      std::vector<double> want(2 * patches), first(2 * patches);
      int want_invalid = -1;
      const uint8_t* prev = frames.data() + fb * (pairs + k);
      const uint8_t* cur = frames.data() + fb * k;
      fm.processImageCoarseToFine(mof::ImageView{prev, fs, fs, (size_t)fs});
      const std::vector<mof::Point2d> s = fm.processImageCoarseToFine(mof::ImageView{cur, fs, fs, (size_t)fs});
      if (mof_fft_process_coarse_to_fine(abi, prev, (size_t)fs, first.data(), nullptr, nullptr) != MOF_OK ||
          mof_fft_process_coarse_to_fine(abi, cur, (size_t)fs, want.data(), nullptr, &want_invalid) != MOF_OK)
        throw std::runtime_error(mof_last_error());
      if (s.size() != patches || std::memcmp(s.data(), want.data(), want.size() * sizeof(double)) != 0 || fm.invalidPatches() != want_invalid ||
          fm.lastQuality().size() != patches)
        differs += " processImageCoarseToFine";
      std::printf("image %d invalid %d", k, fm.invalidPatches());
      for (size_t p = 0; p < s.size(); ++p) std::printf(" %.17g %.17g", s[p].x, s[p].y);
      std::printf("\n");
    }
    mof_fft_destroy(abi);
    std::printf("abi %s\n", differs.empty() ? "same" : differs.c_str());
    return differs.empty() ? 0 : 4;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
