// Host-side C++ test driver for the block matchers' match quality and gate in include/mof/processors.hpp: BlockMatcherBase::setGate /
// gate / lastQuality / invalidBlocks / processBatchDeviceQ and ShardedBlockMatcher::setGate. Reads raw u8 frame pairs (all current
// frames, then all previous ones), runs every pair through setImPrev + processImage on an armed FastSpacedBMMethod, then all of them
// through one processBatchDeviceQ, and prints every integer; tests/test_gpu_bm_quality.py compares them with the CPU oracle's.
//   usage: test_bm_quality <block> <radius> <step> <width> <height> <max_min_sad> <min_sad_range> <npairs> <file>
//   prints: setter <ok | what failed>
//           stateful k invalid <n> vectors <count> then per block <dx> <dy> <min_sad> <zero_sad> <max_sad>
//           batch k invalid <n> mode <8 values> then per block <dx> <dy> <min_sad> <zero_sad> <max_sad>
#include <hip/hip_runtime_api.h>  // device buffers for the batch (the mirror itself needs no HIP)

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "mof/processors.hpp"

template <class T>
static const char* setter_contract(T& m, uint32_t a, uint32_t b) {
  uint32_t ga = 0, gb = 1;
  m.gate(&ga, &gb);
  if (ga != std::numeric_limits<uint32_t>::max() || gb != 0) return "a fresh object is not disarmed";
  m.setGate(a, b);
  m.gate(&ga, &gb);
  if (ga != a || gb != b) return "gate() does not return what setGate() took";
  return nullptr;
}

int main(int argc, char** argv) {
  if (argc < 10) {
    std::fprintf(stderr, "usage: test_bm_quality <block> <radius> <step> <width> <height> <max_min_sad> <min_sad_range> <npairs> <file>\n");
    return 2;
  }
  try {
    const int block = std::atoi(argv[1]), radius = std::atoi(argv[2]), step = std::atoi(argv[3]), w = std::atoi(argv[4]), h = std::atoi(argv[5]);
    const uint32_t a = (uint32_t)std::strtoul(argv[6], nullptr, 10), b = (uint32_t)std::strtoul(argv[7], nullptr, 10);
    const int pairs = std::atoi(argv[8]);
    const size_t fb = (size_t)w * h;
    std::vector<uint8_t> frames(fb * 2 * pairs);
    FILE* f = std::fopen(argv[9], "rb");
    if (!f || std::fread(frames.data(), 1, frames.size(), f) != frames.size()) throw std::runtime_error("cannot read the frames");
    std::fclose(f);
    mof::FastSpacedBMMethod bm(block, radius, step, w, h);
    mof::ShardedBlockMatcher group(bm.config(), 1);
    const char* what = setter_contract(bm, a, b);
    if (!what) what = setter_contract(group, a, b);
    std::printf("setter %s\n", what ? what : "ok");
    const size_t nb = (size_t)bm.config().grid_x * bm.config().grid_y;
    for (int k = 0; k < pairs; ++k) {
      bm.setImPrev(mof::ImageView{frames.data() + fb * (pairs + k), h, w, (size_t)w});
      const std::vector<mof::Point2f> v = bm.processImage(mof::ImageView{frames.data() + fb * k, h, w, (size_t)w}, false, false,
                                                          mof::Point2i{w / 2, h / 2}, 0.0, mof::Point2d{0, 0});
      const std::vector<mof::BlockQuality>& q = bm.lastQuality();
      std::printf("stateful %d invalid %d vectors %d", k, bm.invalidBlocks(), (int)v.size());
      for (size_t p = 0; p < nb; ++p) std::printf(" %d %d %u %u %u", bm.flowX()[p], bm.flowY()[p], q[p].min_sad, q[p].zero_sad, q[p].max_sad);
      std::printf("\n");
    }
    uint8_t* d_frames = nullptr;
    int8_t* d_res = nullptr;  // dx | dy | mode
    uint32_t* d_q = nullptr;  // quality | n_invalid
    const size_t res = (size_t)pairs * (2 * nb + 8), nq = (size_t)pairs * (3 * nb + 1);
    if (hipMalloc((void**)&d_frames, frames.size()) != hipSuccess || hipMalloc((void**)&d_res, res) != hipSuccess ||
        hipMalloc((void**)&d_q, nq * sizeof(uint32_t)) != hipSuccess ||
        hipMemcpy(d_frames, frames.data(), frames.size(), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("device buffers");
    bm.processBatchDeviceQ(d_frames, fb, d_frames + fb * pairs, fb, (size_t)w, pairs, d_res, d_res + pairs * nb, d_res + 2 * pairs * nb, d_q,
                           reinterpret_cast<int32_t*>(d_q + 3 * pairs * nb), nullptr);
    std::vector<int8_t> r(res);
    std::vector<uint32_t> q(nq);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(r.data(), d_res, res, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(q.data(), d_q, nq * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("read-back");
    for (int k = 0; k < pairs; ++k) {
      std::printf("batch %d invalid %d mode", k, (int)q[3 * pairs * nb + k]);
      for (int i = 0; i < 8; ++i) std::printf(" %d", r[2 * pairs * nb + 8 * k + i]);
      for (size_t p = 0; p < nb; ++p)
        std::printf(" %d %d %u %u %u", r[k * nb + p], r[pairs * nb + k * nb + p], q[3 * (k * nb + p)], q[3 * (k * nb + p) + 1], q[3 * (k * nb + p) + 2]);
      std::printf("\n");
    }
    (void)hipFree(d_frames);
    (void)hipFree(d_res);
    (void)hipFree(d_q);
    return what ? 4 : 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
