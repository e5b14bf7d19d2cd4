// Host-side C++ test driver for the response gate of the drop-in adapter `MofFftMethod : OpticFlowCalc` (include/mof/processors.hpp):
// setMinResponse() / minResponse() pass through to the engine. Compiled like tests/cpp/test_adapter.cpp against the reference's own
// interface header (on the include path via -I, read-only) with tests/stubs/ standing in for the OpenCV headers; built by
// oracle/gate_adapter.mk into oracle/_ref/. Reads raw u8 frame pairs (all current frames, then all previous ones), runs every pair
// through two processImage calls (previous, current) on an armed adapter -- through the abstract interface, as the node calls it -- and
// prints every vector with 17 digits; tests/test_gpu_fft_gate.py compares them with the Python binding's armed output.
//   usage: test_gate_adapter <frame_size> <patch_size> <max_px_speed> <min_response> <npairs> <file>
//   prints: setter <ok | what failed>
//           pair k n <vectors> then per patch <x> <y>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "mof/processors.hpp"

#if !(defined(__has_include) && __has_include(<OpticFlowCalc.h>))
#error "test_gate_adapter needs the reference's include directory (OpticFlowCalc.h) and tests/stubs on the include path"
#endif

int main(int argc, char** argv) {
  if (argc < 7) {
    std::fprintf(stderr, "usage: test_gate_adapter <frame_size> <patch_size> <max_px_speed> <min_response> <npairs> <file>\n");
    return 2;
  }
  try {
    const int fs = std::atoi(argv[1]), n = std::atoi(argv[2]), pairs = std::atoi(argv[5]);
    const double speed = std::atof(argv[3]), v = std::atof(argv[4]);
    const size_t fb = (size_t)fs * fs;
    std::vector<unsigned char> frames(fb * 2 * pairs);
    FILE* f = std::fopen(argv[6], "rb");
    if (!f || std::fread(frames.data(), 1, frames.size(), f) != frames.size()) throw std::runtime_error("cannot read the frames");
    std::fclose(f);
    std::string video_path = "", cl_file = "unused.cl";
    MofFftMethod adapter(fs, n, speed, false, false, false, false, &video_path, 30, cl_file, false);
    const char* what = nullptr;
    if (adapter.minResponse() != 0.0) what = "a fresh adapter is not disarmed";
    for (double bad : {-1.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()}) {
      bool threw = false;
      try {
        adapter.setMinResponse(bad);
      } catch (const std::runtime_error&) {
        threw = true;
      }
      if (!what && (!threw || adapter.minResponse() != 0.0)) what = "a value that is not finite and >= 0 was accepted";
    }
    adapter.setMinResponse(v);
    if (!what && adapter.minResponse() != v) what = "minResponse() does not return what setMinResponse() took";
    std::printf("setter %s\n", what ? what : "ok");
    OpticFlowCalc* processClass = &adapter;
    std::vector<cv::Point2d> raw;
    const cv::Point2i mid(fs / 2, fs / 2);
    for (int k = 0; k < pairs; ++k) {
      // (the previous frame goes in through processImage: after a bare setImPrev the engine's first call would still correlate the
      // frame with itself, FftMethod.cpp:1791-1793)
      cv::Mat prev(fs, fs, CV_8UC1, frames.data() + fb * (pairs + k)), cur(fs, fs, CV_8UC1, frames.data() + fb * k);
      processClass->processImage(prev, false, false, mid, 0.0, cv::Point(0, 0), raw, 300, 300);
      const std::vector<cv::Point2d> s = processClass->processImage(cur, false, false, mid, 0.0, cv::Point(0, 0), raw, 300, 300);
      std::printf("pair %d n %zu", k, s.size());
      for (const cv::Point2d& p : s) std::printf(" %.17g %.17g", p.x, p.y);
      std::printf("\n");
    }
    return what ? 4 : 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
