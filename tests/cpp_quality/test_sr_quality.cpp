// Host-side C++ test driver for the estimator's correlation quality in include/mof/processors.hpp: lastQuality(), setMinResponse(),
// processSequenceDeviceQ and processVideoQ of mof::scaleRotationEstimator. Reads a raw u8 video, prints every value with 17 digits;
// tests/test_gpu_sr_quality.py compares them with the Python binding's bits.
//   usage: test_sr_quality <res> <M> <min_response> <nframes> <file>
//   prints: gated <device> <host>
//           frame t stateful <scale> <rot> <response> <peak> device <scale> <rot> <pt.x> <pt.y> <response> <peak> host <the same six>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime_api.h>  // device buffers for the video (the mirror itself needs no HIP)

#include "mof/processors.hpp"

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: test_sr_quality <res> <M> <min_response> <nframes> <file>\n");
    return 2;
  }
  try {
    const int res = std::atoi(argv[1]), n = std::atoi(argv[4]);
    const double M = std::atof(argv[2]), min_response = std::atof(argv[3]);
    const size_t fb = (size_t)res * res;
    std::vector<uint8_t> frames(fb * n);
    FILE* f = std::fopen(argv[5], "rb");
    if (!f || std::fread(frames.data(), 1, frames.size(), f) != frames.size()) throw std::runtime_error("cannot read the video");
    std::fclose(f);
    mof::scaleRotationEstimator one(res, M), dev(res, M), host(res, M);
    for (mof::scaleRotationEstimator* e : {&one, &dev, &host}) {
      e->setMinResponse(min_response);
      if (e->minResponse() != min_response) throw std::runtime_error("minResponse() does not return what setMinResponse() took");
    }
    uint8_t* d_frames = nullptr;
    double* d_res = nullptr;  // [n][4] results | [n][2] quality
    if (hipMalloc((void**)&d_frames, frames.size()) != hipSuccess || hipMalloc((void**)&d_res, (size_t)n * 6 * sizeof(double)) != hipSuccess ||
        hipMemcpy(d_frames, frames.data(), frames.size(), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("device buffers");
    const int gated_dev = dev.processSequenceDeviceQ(d_frames, fb, (size_t)res, n, d_res, d_res + (size_t)n * 4);
    std::vector<double> dres((size_t)n * 6), hres((size_t)n * 6);
    if (hipMemcpy(dres.data(), d_res, dres.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("read-back");
    const int gated_host = host.processVideoQ(frames.data(), fb, (size_t)res, n, hres.data(), hres.data() + (size_t)n * 4);
    std::vector<mof::Point2d> p((size_t)n);
    std::vector<mof::PatchQuality> q((size_t)n);
    for (int t = 0; t < n; ++t) {
      p[t] = one.processImage(mof::ImageView{frames.data() + fb * t, res, res, (size_t)res}, false, false);
      q[t] = one.lastQuality();
    }
    std::printf("gated %d %d\n", gated_dev, gated_host);
    for (int t = 0; t < n; ++t) {
      std::printf("frame %d stateful %.17g %.17g %.17g %.17g", t, p[t].x, p[t].y, q[t].response, q[t].peak);
      for (const std::vector<double>* r : {&dres, &hres}) {
        const double* o = r->data() + 4 * (size_t)t;
        const double* qq = r->data() + (size_t)n * 4 + 2 * (size_t)t;
        std::printf(" %s %.17g %.17g %.17g %.17g %.17g %.17g", r == &dres ? "device" : "host", o[0], o[1], o[2], o[3], qq[0], qq[1]);
      }
      std::printf("\n");
    }
    (void)hipFree(d_frames);
    (void)hipFree(d_res);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
