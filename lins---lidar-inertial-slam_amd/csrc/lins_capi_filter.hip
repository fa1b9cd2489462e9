// lins_capi_filter.hip — the streams' device-resident filter in the C ABI (include/lins_streams_filter.h): loading and reading one
// stream's filter, the IMU propagation between scans, and what lins_streams_step_imu(_raw) (lins_capi_streams.hip)
// queues around the update.  Kernels: filter_kernels.hip.
#include "filter_math.h"
#include "lins_ctx.h"

using namespace lins;
using namespace lins_filt;

namespace lins {

void streams_filter_free(lins_ctx* ctx) { ctx->st.f = lins_ctx::Streams::Filter{}; }

int streams_filter_alloc(lins_ctx* ctx) {
  auto& t = ctx->st;
  auto& f = t.f;
  if (f.d_state) return LINS_OK;
  const size_t n = (size_t)t.n;
  BUF_TRY(ctx, f.d_state.grow(n * 19));
  BUF_TRY(ctx, f.d_cov.grow(n * 324));
  BUF_TRY(ctx, f.d_noise.grow(n * 144));
  BUF_TRY(ctx, f.d_aux.grow(n * kAux));
  BUF_TRY(ctx, f.d_gstate.grow(n * 19));
  BUF_TRY(ctx, f.d_imu.grow(n * LINS_STREAMS_IMU_MAX * 7));
  BUF_TRY(ctx, f.h_imu.grow(n * LINS_STREAMS_IMU_MAX * 7));
  BUF_TRY(ctx, f.d_ints.grow(n * 3));
  BUF_TRY(ctx, f.h_ints.grow(n * 3));
  for (Event& e : f.ev) BUF_TRY(ctx, e.create());
  f.set.assign(n, 0);
  f.prm.assign(n, lins_filter_params{});
  return LINS_OK;
}

int streams_filter_check(lins_ctx* ctx, const int32_t* n_imu, const double* const* imu) {
  auto& t = ctx->st;
  if (!n_imu || !imu) return LINS_E_ARG;
  if (!t.f.d_state) return LINS_E_STATE;
  for (int k = 0; k < t.n; ++k) {
    if (n_imu[k] < 0 || (n_imu[k] && !imu[k])) return LINS_E_ARG;
    if (n_imu[k] > LINS_STREAMS_IMU_MAX) return LINS_E_CAPACITY;
    if (!t.f.set[k]) return LINS_E_STATE;
  }
  return LINS_OK;
}

int streams_filter_predict_queue(lins_ctx* ctx, const int32_t* n_imu, const double* const* imu) {
  auto& t = ctx->st;
  auto& f = t.f;
  const int n = t.n;
  if (f.predict_timed) HIP_TRY(ctx, hipEventSynchronize(f.ev[1]));  // (the staging of the call before has been read)
  size_t rows = 0;
  for (int k = 0; k < n; ++k) {
    f.h_ints[k] = n_imu[k], f.h_ints[n + k] = (int)rows;
    if (n_imu[k]) std::memcpy(f.h_imu + rows * 7, imu[k], (size_t)n_imu[k] * 7 * 8);
    rows += (size_t)n_imu[k];
  }
  HIP_TRY(ctx, hipMemcpyAsync(f.d_ints, f.h_ints, (size_t)n * 2 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  if (rows) HIP_TRY(ctx, hipMemcpyAsync(f.d_imu, f.h_imu, rows * 7 * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(f.ev[0], ctx->stream));
  launch_filter_predict(ctx->stream, n, f.d_ints, f.d_ints + n, f.d_imu, f.d_state, f.d_cov, f.d_noise, f.d_aux);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(f.ev[1], ctx->stream));
  f.predict_timed = true;
  return LINS_OK;
}

int streams_filter_finish_queue(lins_ctx* ctx, const int* mode) {
  auto& t = ctx->st;
  auto& f = t.f;
  const int n = t.n;
  if (f.finish_timed) HIP_TRY(ctx, hipEventSynchronize(f.ev[3]));
  std::memcpy(f.h_ints + 2 * n, mode, (size_t)n * sizeof(int));
  HIP_TRY(ctx, hipMemcpyAsync(f.d_ints + 2 * n, f.h_ints + 2 * n, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(f.ev[2], ctx->stream));
  launch_filter_finish(ctx->stream, n, f.d_ints + 2 * n, ctx->d_state_out, ctx->d_cov_out, f.d_state, f.d_cov, f.d_aux, f.d_gstate);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(f.ev[3], ctx->stream));
  f.finish_timed = true;
  return LINS_OK;
}

}  // namespace lins

extern "C" {

int lins_streams_filter_set(lins_ctx* ctx, int stream, const lins_filter* filt, const double* global_state) {
  if (!ctx || !filt || !global_state) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;
  if (stream < 0 || stream >= t.n) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = streams_filter_alloc(ctx)) return rc;
  auto& f = t.f;
  double aux[kAux] = {};
  for (int i = 0; i < 3; ++i) {
    aux[kAuxAcc + i] = filt->acc_last[i], aux[kAuxGyr + i] = filt->gyr_last[i];
    aux[kAuxPosVar + i] = filt->prm.init_pos_std[i] * filt->prm.init_pos_std[i];
    const double a = filt->prm.init_att_std[i] * kDeg;
    aux[kAuxAttVar + i] = a * a;
  }
  aux[kAuxTime] = filt->time, aux[kAuxHasImu] = filt->has_imu ? 1.0 : 0.0;
  const size_t k = (size_t)stream;
  // (pageable sources: each copy has left the caller's memory when the call returns; in order on the context's stream)
  HIP_TRY(ctx, hipMemcpyAsync(f.d_state + k * 19, filt->state, 19 * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(f.d_cov + k * 324, filt->cov, 324 * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(f.d_noise + k * 144, filt->noise, 144 * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(f.d_aux + k * kAux, aux, sizeof aux, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(f.d_gstate + k * 19, global_state, 19 * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  f.set[k] = 1, f.prm[k] = filt->prm;
  if (t.b.on) t.b.status[k] = LINS_STREAM_RUNNING;  // (machine mode: a filter bootstrapped elsewhere)
  return LINS_OK;
}

int lins_streams_filter_get(lins_ctx* ctx, int stream, lins_filter* filt, double* global_state) {
  if (!ctx || (!filt && !global_state)) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;
  if (stream < 0 || stream >= t.n) return LINS_E_ARG;
  auto& f = t.f;
  if (!f.d_state || !f.set[stream]) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t k = (size_t)stream;
  double aux[kAux];
  if (filt) {
    std::memset(filt, 0, sizeof *filt);
    HIP_TRY(ctx, hipMemcpyAsync(filt->state, f.d_state + k * 19, 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(filt->cov, f.d_cov + k * 324, 324 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(filt->noise, f.d_noise + k * 144, 144 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(aux, f.d_aux + k * kAux, sizeof aux, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (global_state) HIP_TRY(ctx, hipMemcpyAsync(global_state, f.d_gstate + k * 19, 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (filt) {
    for (int i = 0; i < 3; ++i) filt->acc_last[i] = aux[kAuxAcc + i], filt->gyr_last[i] = aux[kAuxGyr + i];
    filt->time = aux[kAuxTime], filt->has_imu = aux[kAuxHasImu] != 0.0;
    filt->prm = f.prm[k];
  }
  return LINS_OK;
}

int lins_streams_filter_predict(lins_ctx* ctx, const int32_t* n_imu, const double* const* imu) {
  if (!ctx) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;
  if (t.b.on) {  // machine mode, processImu by status (SE:242-257): INIT drops, FIRST_SCAN pre-integrates, RUNNING predicts
    if (int rc = streams_boot_check(ctx, n_imu, imu)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rcs = split_join(ctx)) return rcs;
    std::vector<int32_t> n_run((size_t)t.n);
    for (int k = 0; k < t.n; ++k) n_run[k] = t.b.status[k] == LINS_STREAM_RUNNING ? n_imu[k] : 0;
    if (int rc = streams_filter_predict_queue(ctx, n_run.data(), imu)) return rc;
    if (int rc = streams_boot_preintegrate_queue(ctx, n_imu, imu)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < t.n; ++k)
      if (n_imu[k]) std::memcpy(&t.b.imu_last[(size_t)k * 6], imu[k] + (size_t)(n_imu[k] - 1) * 7 + 1, 6 * 8), t.b.imu_seen[k] = 1;
    return LINS_OK;
  }
  if (int rc = streams_filter_check(ctx, n_imu, imu)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  if (int rc = streams_filter_predict_queue(ctx, n_imu, imu)) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LINS_OK;
}

int lins_streams_filter_stats(lins_ctx* ctx, float* predict_ms, float* finish_ms) {
  if (!ctx) return LINS_E_ARG;
  auto& f = ctx->st.f;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (f.predict_timed) {
    HIP_TRY(ctx, hipEventSynchronize(f.ev[1]));
    HIP_TRY(ctx, hipEventElapsedTime(&f.predict_ms, f.ev[0], f.ev[1]));
  }
  if (f.finish_timed) {
    HIP_TRY(ctx, hipEventSynchronize(f.ev[3]));
    HIP_TRY(ctx, hipEventElapsedTime(&f.finish_ms, f.ev[2], f.ev[3]));
  }
  if (predict_ms) *predict_ms = f.predict_ms;
  if (finish_ms) *finish_ms = f.finish_ms;
  return LINS_OK;
}

}  // extern "C"
