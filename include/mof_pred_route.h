/* mof_pred_route.h -- the routes of the FFT engine's window-offset entries: MOF_PRED_ROUTE_GATHER (every engine's default) and
 * MOF_PRED_ROUTE_FUSED, and the BGR8 entry that exists on the fused route. Part of include/mof.h, which includes this file at its end and
 * holds the whole description ("Predicted-shift window offsets": the FUSED route); including either header gives both. */
#ifndef MOF_PRED_ROUTE_H
#define MOF_PRED_ROUTE_H

#include "mof.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MOF_PRED_ROUTE_GATHER 0
#define MOF_PRED_ROUTE_FUSED 1
int mof_fft_set_pred_route(mof_fft_engine* e, int route);
int mof_fft_pred_route(const mof_fft_engine* e);
int mof_fft_pred_route_supported(const mof_fft_config* cfg, int route);
int mof_fft_process_batch_device_pred_bgr(mof_fft_engine* e, const uint8_t* d_cur, size_t cur_stride, const uint8_t* d_prev,
                                          size_t prev_stride, size_t pitch, int n_pairs, const int32_t* d_pred_xy, double* d_out_xy,
                                          double* d_quality, int32_t* d_applied_xy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOF_PRED_ROUTE_H */
