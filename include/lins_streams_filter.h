/*
 * lins_streams_filter.h — the filter of the device-resident streams (lins_host.h: lins_streams_*) held on the device.
 * Implemented in liblins_ieskf.so (csrc/lins_capi_filter.hip, csrc/lins_capi_frontend.hip; kernels:
 * csrc/filter_kernels.hip).  The CPU restatement of the step's finish is lins_filter_finish (lins_host.h).
 */
#ifndef LINS_STREAMS_FILTER_H_
#define LINS_STREAMS_FILTER_H_

#include "lins_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the streams' filter on the device -------------------------------------------------------------------------
 * What StateEstimator keeps between two scans besides the clouds — the StatePredictor (a lins_filter) and globalState_ —
 * held per stream in HBM, so that a running stream needs no host filter call: processImu -> lins_streams_filter_predict,
 * processScan -> lins_streams_step_imu(_raw).  The two-scan bootstrap (SE:331-425) stays host code: a stream's first scan
 * goes through lins_streams_step(_raw), and lins_streams_filter_set hands the bootstrapped filter and globalState_ over.
 * lins_streams_step(_raw) never touch the device filter; both kinds may be mixed on one context.                     */
#define LINS_STREAMS_IMU_MAX 64 /* IMU rows per stream and call */
#define LINS_STREAMS_GATED 1    /* out[k].reserved[0]: the scan had too few features (SE:436-440), see below */
/* load / read one stream's filter and globalState_ (19 doubles); _get synchronises (either output may be NULL) */
int lins_streams_filter_set(lins_ctx* ctx, int stream, const lins_filter* f, const double* global_state);
int lins_streams_filter_get(lins_ctx* ctx, int stream, lins_filter* f, double* global_state);
/* StatePredictor::predict (KF:125-186) of every stream over its own rows: imu[k] = n_imu[k] rows (dt, acc, gyr) of 7
 * doubles, 0 <= n_imu[k] <= LINS_STREAMS_IMU_MAX (LINS_E_CAPACITY beyond); a stream with no rows stays bit for bit as it
 * is.  One kernel launch for all streams.  LINS_E_STATE when a stream has no filter.                                */
int lins_streams_filter_predict(lins_ctx* ctx, const int32_t* n_imu, const double* const* imu);
/* lins_streams_step / _raw with the prior taken from the device filter: the stream's IMU rows since the last call are
 * propagated, the update starts from the predicted (state, covariance) where they lie, and behind it (and the ICP
 * fallback) the finish kernel does on the device what lins_filter_finish does: the filter is left reset, globalState_
 * advanced.  out[k] holds the posterior BEFORE reset(1), as lins_streams_step returns it; global_state_out (optional):
 * n x 19.  A diverged stream hands the ICP pose with the prior covariance to the filter; one that could not take the
 * device fallback (out[k].reserved[0] = LINS_E_UNSUPPORTED) keeps the whole predicted prior.
 * The reference's gate (SE:436-440): a stream whose new scan has <= 5 less-sharp or <= 10 less-flat points gets no
 * update, no integration, no reset — its filter stays as predicted (returned in out[k], iters = 0), out[k].reserved[0] =
 * LINS_STREAMS_GATED, and its resident targets stay the OLD scan's clouds (scan_last_); the other streams advance.
 * LINS_E_STATE (nothing run) when a stream has no filter or no resident last scan.                                   */
int lins_streams_step_imu(lins_ctx* ctx, const lins_segmented_scan* scans, const int32_t* n_imu, const double* const* imu,
                          double scan_period, lins_result* out, int32_t* feature_counts, double* global_state_out);
int lins_streams_step_imu_raw(lins_ctx* ctx, const lins_point* const* raw, const int32_t* n_raw, const int32_t* n_imu,
                              const double* const* imu, double scan_period, lins_result* out, int32_t* feature_counts,
                              double* global_state_out);
/* HIP-event times (ms) of the last predict and finish kernels */
int lins_streams_filter_stats(lins_ctx* ctx, float* predict_ms, float* finish_ms);

#ifdef __cplusplus
}
#endif
#endif
