// Host-side C++ test driver for the fused window-offset route of mof::FftMethod (include/mof/processors.hpp): setPredRoute, predRoute,
// processBatchDevicePredBgr -- and processBatchDevicePred on that route. Reads raw gray u8 frames (all current frames, then all previous
// ones), predicts (px, py) for every patch, runs each method and the C ABI entry it mirrors (on a second engine) and compares their
// bytes; every value is printed with 17 digits, tests/test_gpu_cpp_pred_fused.py compares them with the Python binding's bits.
// The BGR8 frames are made here from the gray ones, channel by channel: f, (f + 85) mod 256, 255 - f (tests/pred_fused_cases.py, bgr_of).
//   usage: test_pred_fused <frame_size> <patch_size> <max_px_speed> <px> <py> <npairs> <file>
//   prints: pred k  then per patch <x> <y> <response> <peak> <ax> <ay>      (gray frames, fused route)
//           bgr k   the same on the BGR8 frames
//           refused <what the wrappers refused, in order>
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

template <class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const std::exception&) {
    return true;
  }
  return false;
}

int main(int argc, char** argv) {
  if (argc < 8) {
    std::fprintf(stderr, "usage: test_pred_fused <frame_size> <patch_size> <max_px_speed> <px> <py> <npairs> <file>\n");
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
    std::vector<uint8_t> bgr(3 * frames.size());
    for (size_t i = 0; i < frames.size(); ++i) {
      bgr[3 * i] = frames[i];
      bgr[3 * i + 1] = (uint8_t)(frames[i] + 85);
      bgr[3 * i + 2] = (uint8_t)(255 - frames[i]);
    }
    mof::FftMethod fm(fs, n, speed);
    const mof_fft_config cfg = fm.config();
    const size_t patches = (size_t)cfg.grid_x * cfg.grid_y, total = patches * pairs;
    mof_fft_engine* abi = nullptr;  // the C ABI's side of every comparison runs on an engine of its own
    if (mof_fft_create(&cfg, &abi) != MOF_OK) throw std::runtime_error(mof_last_error());
    std::string differs, refused;

    DevBuf<uint8_t> d_cur(fb * pairs), d_prev(fb * pairs), d_cur3(3 * fb * pairs), d_prev3(3 * fb * pairs);
    d_cur.up(frames.data());
    d_prev.up(frames.data() + fb * pairs);
    d_cur3.up(bgr.data());
    d_prev3.up(bgr.data() + 3 * fb * pairs);
    std::vector<int32_t> pred(2 * total);
    for (size_t i = 0; i < total; ++i) {
      pred[2 * i] = px;
      pred[2 * i + 1] = py;
    }
    DevBuf<int32_t> d_pred(2 * total), d_applied(2 * total), d_applied2(2 * total);
    d_pred.up(pred.data());
    DevBuf<double> d_out(2 * total), d_q(2 * total), d_out2(2 * total), d_q2(2 * total);

    // the default route: the gather, which takes no BGR8 frames; an unknown route is refused and changes nothing
    if (fm.predRoute() != MOF_PRED_ROUTE_GATHER || mof_fft_pred_route(abi) != MOF_PRED_ROUTE_GATHER) differs += " predRoute(default)";
    if (throws([&] { fm.processBatchDevicePredBgr(d_cur3.p, 3 * fb, d_prev3.p, 3 * fb, 3 * (size_t)fs, pairs, d_pred.p, d_out.p); })) refused += " bgr-on-gather";
    if (throws([&] { fm.setPredRoute(2); })) refused += " route-2";
    if (fm.predRoute() != MOF_PRED_ROUTE_GATHER) differs += " predRoute(after a refusal)";
    fm.setPredRoute(MOF_PRED_ROUTE_FUSED);
    if (mof_fft_set_pred_route(abi, MOF_PRED_ROUTE_FUSED) != MOF_OK) throw std::runtime_error(mof_last_error());
    if (fm.predRoute() != MOF_PRED_ROUTE_FUSED) differs += " predRoute(fused)";

    auto print = [&](const char* tag, const std::vector<double>& out, const std::vector<double>& q, const std::vector<int32_t>& a) {
      for (int k = 0; k < pairs; ++k) {
        std::printf("%s %d", tag, k);
        for (size_t p = k * patches; p < (k + 1) * patches; ++p)
          std::printf(" %.17g %.17g %.17g %.17g %d %d", out[2 * p], out[2 * p + 1], q[2 * p], q[2 * p + 1], a[2 * p], a[2 * p + 1]);
        std::printf("\n");
      }
    };
    fm.reservePred(pairs);
    fm.processBatchDevicePred(d_cur.p, fb, d_prev.p, fb, (size_t)fs, pairs, d_pred.p, d_out.p, d_q.p, d_applied.p);
    if (mof_fft_process_batch_device_pred(abi, d_cur.p, fb, d_prev.p, fb, (size_t)fs, pairs, d_pred.p, d_out2.p, d_q2.p, d_applied2.p, nullptr) != MOF_OK)
      throw std::runtime_error(mof_last_error());
    {
      const std::vector<double> out = d_out.down(), q = d_q.down();
      const std::vector<int32_t> a = d_applied.down();
      if (!same(out, d_out2.down()) || !same(q, d_q2.down()) || !same(a, d_applied2.down())) differs += " processBatchDevicePred";
      print("pred", out, q, a);
    }
    fm.processBatchDevicePredBgr(d_cur3.p, 3 * fb, d_prev3.p, 3 * fb, 3 * (size_t)fs, pairs, d_pred.p, d_out.p, d_q.p, d_applied.p);
    if (mof_fft_process_batch_device_pred_bgr(abi, d_cur3.p, 3 * fb, d_prev3.p, 3 * fb, 3 * (size_t)fs, pairs, d_pred.p, d_out2.p, d_q2.p, d_applied2.p,
                                              nullptr) != MOF_OK)
      throw std::runtime_error(mof_last_error());
    {
      const std::vector<double> out = d_out.down(), q = d_q.down();
      const std::vector<int32_t> a = d_applied.down();
      if (!same(out, d_out2.down()) || !same(q, d_q2.down()) || !same(a, d_applied2.down())) differs += " processBatchDevicePredBgr";
      print("bgr", out, q, a);
    }
    mof_fft_destroy(abi);
    std::printf("refused%s\n", refused.c_str());
    std::printf("abi %s\n", differs.empty() ? "same" : differs.c_str());
    return differs.empty() ? 0 : 4;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
