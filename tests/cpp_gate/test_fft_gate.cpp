// Host-side C++ test driver for the FFT engine's response gate in include/mof/processors.hpp: setMinResponse() / minResponse() of
// mof::FftMethod and mof::ShardedFftMethod. Reads raw u8 frame pairs (all current frames, then all previous ones), runs every pair through
// two processImage calls (previous, current) on an armed engine and prints every value with 17 digits; tests/test_gpu_fft_gate.py
// compares them with the Python binding's bits.
//   usage: test_fft_gate <frame_size> <patch_size> <max_px_speed> <min_response> <npairs> <file>
//   prints: setter <ok | what failed>
//           pair k invalid <n> then per patch <x> <y> <response> <peak>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "mof/processors.hpp"

template <class T>
static const char* setter_contract(T& m, double v) {
  if (m.minResponse() != 0.0) return "a fresh object is not disarmed";
  for (double bad : {-1.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()}) {
    bool threw = false;
    try {
      m.setMinResponse(bad);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw || m.minResponse() != 0.0) return "a value that is not finite and >= 0 was accepted";
  }
  m.setMinResponse(v);
  if (m.minResponse() != v) return "minResponse() does not return what setMinResponse() took";
  return nullptr;
}

int main(int argc, char** argv) {
  if (argc < 7) {
    std::fprintf(stderr, "usage: test_fft_gate <frame_size> <patch_size> <max_px_speed> <min_response> <npairs> <file>\n");
    return 2;
  }
  try {
    const int fs = std::atoi(argv[1]), n = std::atoi(argv[2]), pairs = std::atoi(argv[5]);
    const double speed = std::atof(argv[3]), v = std::atof(argv[4]);
    const size_t fb = (size_t)fs * fs;
    std::vector<uint8_t> frames(fb * 2 * pairs);
    FILE* f = std::fopen(argv[6], "rb");
    if (!f || std::fread(frames.data(), 1, frames.size(), f) != frames.size()) throw std::runtime_error("cannot read the frames");
    std::fclose(f);
    mof::FftMethod fm(fs, n, speed);
    mof::ShardedFftMethod group(fm.config(), 1);
    const char* what = setter_contract(fm, v);
    if (!what) what = setter_contract(group, v);
    std::printf("setter %s\n", what ? what : "ok");
    std::vector<mof::Point2d> raw;
    for (int k = 0; k < pairs; ++k) {
      // (the previous frame goes in through processImage: after a bare setImPrev the engine's first call would still correlate the
      // frame with itself, FftMethod.cpp:1791-1793)
      fm.processImage(mof::ImageView{frames.data() + fb * (pairs + k), fs, fs, (size_t)fs}, false, false, mof::Point2i{fs / 2, fs / 2}, 0.0,
                      mof::Point2d{0, 0}, raw);
      const std::vector<mof::Point2d> s = fm.processImage(mof::ImageView{frames.data() + fb * k, fs, fs, (size_t)fs}, false, false,
                                                          mof::Point2i{fs / 2, fs / 2}, 0.0, mof::Point2d{0, 0}, raw);
      const std::vector<mof::PatchQuality>& q = fm.lastQuality();
      std::printf("pair %d invalid %d", k, fm.invalidPatches());
      for (size_t p = 0; p < s.size(); ++p) std::printf(" %.17g %.17g %.17g %.17g", s[p].x, s[p].y, q[p].response, q[p].peak);
      std::printf("\n");
    }
    return what ? 4 : 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
