// mof_frontend.hip -- C ABI of the camera front end (include/mof.h, mof_frontend_*): the node's rectangle, the argument checks
// and the launch of csrc/fe_kernel.hip. Stateless: no engine, no allocation, the caller's current device and stream.

#include "mof.h"

#include <hip/hip_runtime.h>

#include <cmath>

#include "capi_graph.hpp"
#include "mof_kernels.h"

namespace {

constexpr auto& fail = mof::capi_fail;

int check_config(const mof_frontend_config* c) {
  if (!c) return fail(MOF_ERR_BAD_ARG, "null front-end config");
  if (c->src_width < 1 || c->src_height < 1) return fail(MOF_ERR_BAD_ARG, "camera frame %d x %d", c->src_width, c->src_height);
  if (c->channels != 1 && c->channels != 3) return fail(MOF_ERR_BAD_ARG, "channels %d: 1 (mono8) or 3 (BGR8)", c->channels);
  if (c->scale < 1) return fail(MOF_ERR_BAD_ARG, "scale %d: an integer scale_factor >= 1", c->scale);
  if (c->src_width % c->scale || c->src_height % c->scale)
    return fail(MOF_ERR_UNSUPPORTED, "%d x %d by %d is not an exact ratio: OpenCV's general bilinear path is not restated",
                c->src_width, c->src_height, c->scale);
  const long long w = c->src_width / c->scale, h = c->src_height / c->scale;
  if (c->crop_width < 1 || c->crop_height < 1 || c->crop_x < 0 || c->crop_y < 0 || c->crop_x + (long long)c->crop_width > w ||
      c->crop_y + (long long)c->crop_height > h)
    return fail(MOF_ERR_BAD_ARG, "crop (%d, %d, %d, %d) leaves the %lld x %lld downscaled image", c->crop_x, c->crop_y, c->crop_width,
                c->crop_height, w, h);
  return MOF_OK;
}

// one past the last byte of n frames of `rows` rows, `row_bytes` used per row; false on overflow
bool span(size_t n, size_t stride, size_t rows, size_t pitch, size_t row_bytes, size_t* out) {
  size_t a = 0, b = 0, c = 0;
  if (__builtin_mul_overflow(n - 1, stride, &a) || __builtin_mul_overflow(rows - 1, pitch, &b) || __builtin_add_overflow(a, b, &c) ||
      __builtin_add_overflow(c, row_bytes, out))
    return false;
  return true;
}

}  // namespace

extern "C" {

int mof_frontend_config_reference(mof_frontend_config* cfg, int cam_width, int cam_height, int channels, int scale_factor,
                                  int frame_size, double cx) {
  if (!cfg) return fail(MOF_ERR_BAD_ARG, "null front-end config");
  if (cam_width < 1 || cam_height < 1 || scale_factor < 1 || frame_size < 1 || (channels != 1 && channels != 3))
    return fail(MOF_ERR_BAD_ARG, "bad reference front end: camera %d x %d, %d channels, scale_factor %d, frame_size %d", cam_width,
                cam_height, channels, scale_factor, frame_size);
  if (!(std::fabs(cx) < 2147483648.0)) return fail(MOF_ERR_BAD_ARG, "cx %g is not a pixel coordinate", cx);
  cfg->src_width = cam_width;
  cfg->src_height = cam_height;
  cfg->channels = channels;
  cfg->scale = scale_factor;
  if (cam_width % scale_factor || cam_height % scale_factor)
    return fail(MOF_ERR_UNSUPPORTED, "%d x %d by scale_factor %d is not an exact ratio: OpenCV's general bilinear path is not restated",
                cam_width, cam_height, scale_factor);
  const int fs = frame_size / scale_factor;                // _frame_size_ / _scale_factor_ (optic_flow.cpp:867-869)
  const int w = cam_width / scale_factor, h = cam_height / scale_factor;  // dsize (:1604)
  cfg->crop_x = (int)cx - fs / 2;                           // int image_center_x = cx_; xi (:1611-1613)
  cfg->crop_y = h / 2 - fs / 2;                             // yi (:1612-1614)
  cfg->crop_width = cfg->crop_height = fs;
  if (fs < 1 || cfg->crop_x < 0 || cfg->crop_y < 0 || cfg->crop_x + (long long)fs > w || cfg->crop_y + (long long)fs > h)
    return fail(MOF_ERR_BAD_ARG,
                "the node's crop (%d, %d, %d, %d) leaves the %d x %d scaled image, where cv::Mat(roi) throws: it is centred on the "
                "UNSCALED principal point cx_ = %g (optic_flow.cpp:1611); pass an explicit crop, e.g. centred on cx_ / %d",
                cfg->crop_x, cfg->crop_y, fs, fs, w, h, cx, scale_factor);
  return MOF_OK;
}

int mof_frontend_validate(const mof_frontend_config* cfg) { return check_config(cfg); }

int mof_frontend_batch_device(const mof_frontend_config* cfg, const uint8_t* d_src, size_t src_stride, size_t src_pitch, int n,
                              uint8_t* d_dst, size_t dst_stride, size_t dst_pitch, void* stream) {
  int rc = check_config(cfg);
  if (rc) return rc;
  if (n < 0) return fail(MOF_ERR_BAD_ARG, "n = %d frames", n);
  if (n == 0) return MOF_OK;
  if (!d_src || !d_dst) return fail(MOF_ERR_BAD_ARG, "null frames or crops");
  const size_t src_row = (size_t)cfg->channels * (size_t)cfg->src_width, dst_row = (size_t)cfg->crop_width;
  if (src_pitch < src_row) return fail(MOF_ERR_BAD_ARG, "src_pitch %zu < %zu bytes of a camera row", src_pitch, src_row);
  if (dst_pitch < dst_row) return fail(MOF_ERR_BAD_ARG, "dst_pitch %zu < crop_width %zu", dst_pitch, dst_row);
  size_t crop_bytes = 0, src_end = 0, dst_end = 0;
  span(1, 0, (size_t)cfg->crop_height, dst_pitch, dst_row, &crop_bytes);
  if (n > 1 && dst_stride < crop_bytes) return fail(MOF_ERR_BAD_ARG, "dst_stride %zu: the output crops (%zu bytes) would overlap", dst_stride, crop_bytes);
  if (!span((size_t)n, src_stride, (size_t)cfg->src_height, src_pitch, src_row, &src_end) ||
      !span((size_t)n, dst_stride, (size_t)cfg->crop_height, dst_pitch, dst_row, &dst_end) ||
      (uintptr_t)d_src > UINTPTR_MAX - src_end || (uintptr_t)d_dst > UINTPTR_MAX - dst_end)
    return fail(MOF_ERR_BAD_ARG, "the batch does not fit the address space");
  const uintptr_t s0 = (uintptr_t)d_src, s1 = s0 + src_end, t0 = (uintptr_t)d_dst, t1 = t0 + dst_end;
  if (s0 < t1 && t0 < s1) return fail(MOF_ERR_BAD_ARG, "source and destination ranges overlap");
  const int P = mof::frontend_run_pixels(cfg->channels, cfg->scale);
  if ((unsigned long long)cfg->crop_height * (unsigned long long)((cfg->crop_width + P - 1) / P) > (1ull << 31))
    return fail(MOF_ERR_BAD_ARG, "crop %d x %d is too large for one launch", cfg->crop_width, cfg->crop_height);
  int devices = 0;
  rc = mof::require_device(&devices);  // (the stream's device is the caller's: nothing is selected here)
  if (rc) return rc;
  mof::FeArgs a{};
  a.src = d_src;
  a.src_stride = src_stride;
  a.src_pitch = src_pitch;
  a.dst = d_dst;
  a.dst_stride = dst_stride;
  a.dst_pitch = dst_pitch;
  a.scale = cfg->scale;
  a.crop_x = cfg->crop_x;
  a.crop_y = cfg->crop_y;
  a.crop_w = cfg->crop_width;
  a.crop_h = cfg->crop_height;
  const hipError_t e = mof::launch_frontend(a, cfg->channels, n, (hipStream_t)stream);
  if (e != hipSuccess) return fail(MOF_ERR_HIP, "front-end launch: %s", hipGetErrorString(e));
  return MOF_OK;
}

}  // extern "C"
