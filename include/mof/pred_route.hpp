// pred_route.hpp -- the C ABI of include/mof_pred_route.h as processors.hpp's FftMethod calls it (setPredRoute, predRoute,
// processBatchDevicePredBgr): one inline forwarder per entry. Included by processors.hpp; not meant to be included on its own.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../mof_pred_route.h"

namespace mof {
namespace detail {
inline int fftSetPredRoute(mof_fft_engine* e, int route) { return mof_fft_set_pred_route(e, route); }
inline int fftPredRoute(const mof_fft_engine* e) { return mof_fft_pred_route(e); }
inline int fftProcessBatchDevicePredBgr(mof_fft_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev, size_t prev_stride,
                                        size_t pitch, int n_pairs, const int32_t* d_pred_xy, double* d_out_xy, double* d_quality,
                                        int32_t* d_applied_xy, void* stream) {
  return mof_fft_process_batch_device_pred_bgr(e, d_cur, cur_stride, d_prev, prev_stride, pitch, n_pairs, d_pred_xy, d_out_xy, d_quality,
                                               d_applied_xy, stream);
}
}  // namespace detail
}  // namespace mof
