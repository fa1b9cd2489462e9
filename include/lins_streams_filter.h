/*
 * lins_streams_filter.h — the filter of the device-resident streams (lins_host.h: lins_streams_*) held on the device.
 * Implemented in liblins_ieskf.so (csrc/lins_capi_filter.hip, csrc/lins_capi_boot.hip, csrc/lins_capi_frontend.hip;
 * kernels: csrc/filter_kernels.hip, csrc/boot_kernels.hip).  The CPU restatement of the step's finish is
 * lins_filter_finish, that of the two-scan bootstrap lins_host_preintegrate / lins_host_boot_first / _second (lins_host.h).
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
 * processScan -> lins_streams_step_imu(_raw).  A stream is started either by hand — its first scan through
 * lins_streams_step(_raw), a filter bootstrapped elsewhere through lins_streams_filter_set — or by the state machine
 * below (lins_streams_machine_init, lins_streams_process*), which runs the two-scan bootstrap (SE:331-425) on the device.
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

/* ---- the streams' state machine: StateEstimator's INIT -> FIRST_SCAN -> RUNNING (SE:242-425) on the device ---------
 * With lins_streams_machine_init every stream carries the reference's status_ (SE:177-183), and one call per scan does
 * processImu over the stream's rows and processPCL, whatever the stream's status; streams in different states share a
 * batch.  Without that call every entry point above behaves as if this section did not exist.                         */
#define LINS_STREAM_INIT 0
#define LINS_STREAM_FIRST_SCAN 1
#define LINS_STREAM_RUNNING 3
#define LINS_STREAMS_FIRST 2  /* out[k].reserved[0]: the scan was accepted as the stream's first (processFirstScan) */
#define LINS_STREAMS_BOOTED 3 /* ... as its second: the filter and globalState_ are initialised (processSecondScan) */
/* lins_boot_params, lins_preintegration: lins_host.h */
void lins_boot_default_params(lins_boot_params* p);
/* after lins_streams_init: every stream to LINS_STREAM_INIT — resident scans and filters dropped —, the covariance /
 * noise template of a new filter (lins_filter_init's) uploaded.  A second call starts anew.                         */
int lins_streams_machine_init(lins_ctx* ctx, const lins_boot_params* prm);
/* processImu over each stream's rows (as lins_streams_filter_predict takes them), then processPCL of its scan:
 *   INIT        rows dropped; a scan with >= 10 less-sharp and >= 100 less-flat points becomes the resident first scan,
 *               as extracted (SE:331-375): out[k] = the zero-initialised filter, iters = 0, reserved[0] =
 *               LINS_STREAMS_FIRST.  Fewer: LINS_STREAMS_GATED, the stream stays INIT.
 *   FIRST_SCAN  rows pre-integrated (IB:53-81); the same gate, failing it -> INIT (the resident first scan stays until a
 *               new one replaces it).  Else estimateTransform from the pre-integrated pose — ONE batched launch of the
 *               device ICP for all such streams —, estimateInitialState, the filter's initialisation and globalState_
 *               (SE:379-425): out[k].state / cov = the filter after initialisation, iters / converged = the ICP's rounds /
 *               stop flag, reserved[0] = LINS_STREAMS_BOOTED.  Clouds the device ICP cannot take (or icp_freq != 1):
 *               reserved[0] = LINS_E_UNSUPPORTED, the stream stays FIRST_SCAN with its pre-integration (this call's rows
 *               included) and resident scan; bootstrap it on the host and hand it over with lins_streams_filter_set.
 *   RUNNING     what lins_streams_step_imu(_raw) does and returns, bit for bit.
 * scan_imu: n x 6, the imu_last_ handed to processPCL (acc, gyr: the newest IMU sample, EC:164-169), or NULL = the last
 * row of the stream's rows in this call, else the last row the stream has been given; a stream that is not RUNNING and
 * has none: LINS_E_ARG, nothing run.  scan_time: n doubles (the filter's time_ at initialisation).  status_out
 * (optional): each stream's status after the call.  A RUNNING stream without a resident last scan: LINS_E_STATE.    */
int lins_streams_process(lins_ctx* ctx, const lins_segmented_scan* scans, const int32_t* n_imu, const double* const* imu,
                         const double* scan_imu, const double* scan_time, double scan_period, lins_result* out,
                         int32_t* feature_counts, double* global_state_out, int32_t* status_out);
int lins_streams_process_raw(lins_ctx* ctx, const lins_point* const* raw, const int32_t* n_raw, const int32_t* n_imu,
                             const double* const* imu, const double* scan_imu, const double* scan_time, double scan_period,
                             lins_result* out, int32_t* feature_counts, double* global_state_out, int32_t* status_out);
/* In machine mode lins_streams_filter_predict dispatches per status (drop / pre-integrate / predict),
 * lins_streams_filter_set sets its stream RUNNING, lins_streams_step_imu* still need every stream RUNNING.          */
int lins_streams_status(lins_ctx* ctx, int32_t* status /* n */);
/* one stream's pre-integration record; LINS_E_STATE outside FIRST_SCAN.  Synchronises. */
int lins_streams_preintegration_get(lins_ctx* ctx, int stream, lins_preintegration* out);
/* linState_ of every stream (n x 19) as the last step's re-projection read it: the posterior of a RUNNING stream, the
 * identity of a first scan, the ICP's pose of a second.  Synchronises.                                              */
int lins_streams_lin_state(lins_ctx* ctx, double* lin_state);
/* HIP-event times (ms) of the last call's pre-integration kernel, of its bootstrap ICP (index of the first scans'
 * clouds, start rows, the batched ICP launch) and of the bootstrap's finish kernel                                  */
int lins_streams_boot_stats(lins_ctx* ctx, float* preintegrate_ms, float* icp_ms, float* finish_ms);

#ifdef __cplusplus
}
#endif
#endif
