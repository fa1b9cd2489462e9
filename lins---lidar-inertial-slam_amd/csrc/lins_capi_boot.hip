// lins_capi_boot.hip — the streams' state machine in the C ABI (include/lins_streams_filter.h: lins_streams_machine_init,
// lins_streams_process*, ...): the reference's status_ per stream and the two-scan bootstrap (SE:331-425) around the step of
// lins_capi_streams.hip.  Kernels: boot_kernels.hip; the bootstrap's ICP is the device ICP of the divergence fallback
// (launch_lds_mr_icp), one launch over the compact list of the streams taking their second scan.
#include "boot_math.h"
#include "filter_init.h"
#include "lins_ctx.h"

using namespace lins;
using namespace lins_boot;
using lins_filt::kAux;

namespace lins {

void streams_boot_free(lins_ctx* ctx) { ctx->st.b = lins_ctx::Streams::Boot{}; }

int streams_boot_check(lins_ctx* ctx, const int32_t* n_imu, const double* const* imu) {
  auto& t = ctx->st;
  if (!n_imu || !imu) return LINS_E_ARG;
  for (int k = 0; k < t.n; ++k) {
    if (n_imu[k] < 0 || (n_imu[k] && !imu[k])) return LINS_E_ARG;
    if (n_imu[k] > LINS_STREAMS_IMU_MAX) return LINS_E_CAPACITY;
  }
  return LINS_OK;
}

int streams_boot_preintegrate_queue(lins_ctx* ctx, const int32_t* n_imu, const double* const* imu) {
  auto& t = ctx->st;
  auto& b = t.b;
  const int n = t.n;
  if (b.pre_timed) HIP_TRY(ctx, hipEventSynchronize(b.ev[1]));  // (the staging of the call before has been read)
  int max_rows = 0;
  for (int k = 0; k < n; ++k) {
    const int cnt = b.status[k] == LINS_STREAM_FIRST_SCAN ? n_imu[k] : 0;
    b.h_ints[k] = cnt;
    max_rows = std::max(max_rows, cnt);
  }
  for (int k = 0; k < n; ++k)  // component-major: (row, component, stream); a stream's missing rows are never read
    for (int it = 0; it < b.h_ints[k]; ++it)
      for (int j = 0; j < 7; ++j) b.h_rows[((size_t)it * 7 + j) * n + k] = imu[k][it * 7 + j];
  HIP_TRY(ctx, hipMemcpyAsync(b.d_ints, b.h_ints, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  if (max_rows) HIP_TRY(ctx, hipMemcpyAsync(b.d_rows, b.h_rows, (size_t)max_rows * 7 * n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(b.ev[0], ctx->stream));
  if (max_rows) launch_boot_preintegrate(ctx->stream, n, b.d_ints, b.d_rows, b.d_tmpl, b.d_pre, t.f.d_aux);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(b.ev[1], ctx->stream));
  b.pre_timed = true;
  return LINS_OK;
}

int streams_boot_finish(lins_ctx* ctx, const int* mode, const std::vector<ScanDesc>& descs, const StepMachine& mach, lins_result* out) {
  auto& t = ctx->st;
  auto& b = t.b;
  auto& f = t.f;
  const int n = t.n, m = (int)descs.size();
  // (every step ends synchronised: the staging of the call before has been read; the times are those of this call)
  b.icp_timed = b.finish_timed = false, b.icp_ms = b.finish_ms = 0.f;
  bool any = false;
  for (int k = 0; k < n; ++k) any = any || mode[k] != 0;
  if (!any) return LINS_OK;
  int* h_mode = b.h_ints + n;
  int* h_slot = b.h_ints + 2 * n;
  int* h_list = b.h_ints + 3 * n;
  int i = 0;
  for (int k = 0; k < n; ++k) {
    h_mode[k] = mode[k], h_slot[k] = 0;
    if (mode[k] == 2) h_slot[k] = i, h_list[i++] = k;
    for (int j = 0; j < 6; ++j) b.h_scan[(size_t)k * 8 + j] = mode[k] ? mach.scan_imu[(size_t)k * 6 + j] : 0.0;
    b.h_scan[(size_t)k * 8 + 6] = mach.scan_time[k], b.h_scan[(size_t)k * 8 + 7] = 0.0;
  }
  if (i != m) return LINS_E_ARG;
  HIP_TRY(ctx, hipMemcpyAsync(b.d_ints + n, b.h_ints + n, (size_t)n * 3 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(b.d_scan, b.h_scan, (size_t)n * 8 * 8, hipMemcpyHostToDevice, ctx->stream));
  if (m) {
    // (pageable source: the copy has left `descs` when the call returns)
    HIP_TRY(ctx, hipMemcpyAsync(b.d_desc, descs.data(), (size_t)m * sizeof(ScanDesc), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(b.ev[2], ctx->stream));
    // the search index of the first scans' clouds (kd-tree setInputCloud of SE:363-364), the start rows, estimateTransform
    launch_grid_index(ctx->stream, m, b.d_desc, t.d_arena, t.d_gsorted, b.d_tab);
    launch_boot_start(ctx->stream, m, b.d_ints + 3 * n, b.d_pre, b.d_icp_in);
    launch_lds_mr_icp(ctx->stream, m, ctx->dprm, b.d_desc, t.d_arena, t.d_gsorted, b.d_tab, b.d_icp_in, b.d_icp_out, b.d_out, ctx->d_idx);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(b.ev[3], ctx->stream));
    b.icp_timed = true;
    HIP_TRY(ctx, hipMemcpyAsync(b.h_out, b.d_out, (size_t)m * sizeof(OutRec), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipEventRecord(b.ev[4], ctx->stream));
  launch_boot_finish(ctx->stream, n, b.d_ints + n, b.d_ints + 2 * n, b.d_icp_out, b.d_scan, b.d_tmpl, b.d_pre, f.d_state, f.d_cov, f.d_noise,
                     f.d_aux, f.d_gstate, ctx->d_state_out);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(b.ev[5], ctx->stream));
  b.finish_timed = true;
  for (int k = 0; k < n; ++k) {
    if (!mode[k]) continue;
    lins_result& r = out[k];
    std::memset(&r, 0, sizeof r);
    HIP_TRY(ctx, hipMemcpyAsync(r.state, f.d_state + (size_t)k * 19, 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
    std::memcpy(r.cov, b.h_tmpl.data() + kTmplCov, 324 * 8);
    r.reserved[0] = mode[k] == 1 ? LINS_STREAMS_FIRST : LINS_STREAMS_BOOTED;
    f.set[k] = 1, f.prm[k] = b.prm.filter;
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int j = 0; j < m; ++j) {
    lins_result& r = out[h_list[j]];
    const OutRec& o = b.h_out[j];
    r.residual_norm = o.residual_norm, r.update_norm = o.update_norm;
    r.iters = o.iters, r.converged = o.converged, r.m_surf = o.m_surf, r.m_corner = o.m_corner;
  }
  return LINS_OK;
}

}  // namespace lins

extern "C" {

int lins_streams_machine_init(lins_ctx* ctx, const lins_boot_params* prm) {
  if (!ctx || !prm) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (int rc = streams_filter_alloc(ctx)) return rc;
  streams_boot_free(ctx);
  auto& b = t.b;
  const size_t n = (size_t)t.n;
  BUF_TRY(ctx, b.d_tmpl.grow(kTmpl));
  BUF_TRY(ctx, b.d_pre.grow(n * kPre));
  BUF_TRY(ctx, b.d_rows.grow(n * LINS_STREAMS_IMU_MAX * 7));
  BUF_TRY(ctx, b.h_rows.grow(n * LINS_STREAMS_IMU_MAX * 7));
  BUF_TRY(ctx, b.d_scan.grow(n * 8));
  BUF_TRY(ctx, b.h_scan.grow(n * 8));
  BUF_TRY(ctx, b.d_ints.grow(n * 4));
  BUF_TRY(ctx, b.h_ints.grow(n * 4));
  BUF_TRY(ctx, b.d_desc.grow(n));
  BUF_TRY(ctx, b.d_tab.grow(n));
  BUF_TRY(ctx, b.d_icp_in.grow(n * 19));
  BUF_TRY(ctx, b.d_icp_out.grow(n * 19));
  BUF_TRY(ctx, b.d_out.grow(n));
  BUF_TRY(ctx, b.h_out.grow(n));
  for (Event& e : b.ev) BUF_TRY(ctx, e.create());
  b.prm = *prm;
  // the template: what lins_filter_init forms, and the variances reset(1) re-installs (as lins_streams_filter_set)
  b.h_tmpl.assign(kTmpl, 0.0);
  lins_filt_init::cov_noise(&prm->filter, b.h_tmpl.data() + kTmplCov, b.h_tmpl.data() + kTmplNoise);
  for (int i = 0; i < 3; ++i) {
    b.h_tmpl[kTmplPosVar + i] = prm->filter.init_pos_std[i] * prm->filter.init_pos_std[i];
    const double a = prm->filter.init_att_std[i] * lins_filt::kDeg;
    b.h_tmpl[kTmplAttVar + i] = a * a;
    b.h_tmpl[kTmplBa + i] = prm->init_ba[i], b.h_tmpl[kTmplBw + i] = prm->init_bw[i];
  }
  HIP_TRY(ctx, hipMemcpy(b.d_tmpl, b.h_tmpl.data(), kTmpl * 8, hipMemcpyHostToDevice));
  // every stream: no filter, no resident scan; defined rows where the kernels read before a bootstrap has written
  // (the update kernel copies the prior row of a stream without queries; globalState_ starts as the identity, SE:213)
  std::vector<double> rows(n * 19), zeros(n * 324, 0.0);
  for (size_t k = 0; k < n; ++k) lins_filt::store(identity_state(), rows.data() + k * 19);
  auto& f = t.f;
  HIP_TRY(ctx, hipMemcpy(f.d_state, rows.data(), n * 19 * 8, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(f.d_gstate, rows.data(), n * 19 * 8, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(f.d_cov, zeros.data(), n * 324 * 8, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(f.d_noise, zeros.data(), n * 144 * 8, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(f.d_aux, zeros.data(), n * kAux * 8, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(b.d_pre, zeros.data(), n * kPre * 8, hipMemcpyHostToDevice));
  f.set.assign(n, 0);
  b.status.assign(n, LINS_STREAM_INIT);
  b.imu_seen.assign(n, 0), b.imu_last.assign(n * 6, 0.0);
  t.cur.assign(n, 0), t.last_counts.assign(n * 2, -1);
  t.outl_counts.assign(n * 2, 0), t.outl_put.assign(n, 0), t.outl_pending = false;
  t.index_ready = false;
  streams_slam_reset(ctx);
  b.on = true;
  return LINS_OK;
}

// imu_last_ of every stream for this call (EC:164-169): the caller's, else the last row given now, else the last one seen
static int resolve_imu_last(lins_ctx* ctx, const int32_t* n_imu, const double* const* imu, const double* scan_imu, std::vector<double>& last,
                            std::vector<char>& seen) {
  auto& t = ctx->st;
  last = t.b.imu_last, seen = t.b.imu_seen;
  for (int k = 0; k < t.n; ++k) {
    const double* src = scan_imu ? scan_imu + (size_t)k * 6 : (n_imu[k] ? imu[k] + (size_t)(n_imu[k] - 1) * 7 + 1 : nullptr);
    if (src) std::memcpy(&last[(size_t)k * 6], src, 6 * 8), seen[k] = 1;
    if (!seen[k] && t.b.status[k] != LINS_STREAM_RUNNING) return LINS_E_ARG;
  }
  return LINS_OK;
}

static int process_impl(lins_ctx* ctx, const lins_segmented_scan* scans, const lins_point* const* raw, const int32_t* n_raw, const int32_t* n_imu,
                        const double* const* imu, const double* scan_imu, const double* scan_time, double scan_period, lins_result* out,
                        int32_t* feature_counts, double* global_state_out, int32_t* status_out) {
  if (!ctx || !out || !scan_time) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed || !t.b.on) return LINS_E_STATE;
  if (int rc = streams_boot_check(ctx, n_imu, imu)) return rc;
  for (int k = 0; k < t.n; ++k)
    if (t.b.status[k] == LINS_STREAM_RUNNING && (t.last_counts[(size_t)k * 2] < 0 || !t.f.set[k])) return LINS_E_STATE;
  std::vector<double> last;
  std::vector<char> seen;
  if (int rc = resolve_imu_last(ctx, n_imu, imu, scan_imu, last, seen)) return rc;
  const StepImu si{n_imu, imu, global_state_out};
  const StepMachine sm{last.data(), scan_time, seen.data(), status_out};
  const int rc = streams_step_impl(ctx, StepScans{scans, raw, n_raw, scan_period}, StepPrior{nullptr, nullptr, &si, &sm}, out, feature_counts);
  if (rc == LINS_OK) t.b.imu_last = last, t.b.imu_seen = seen;
  return rc;
}

int lins_streams_process(lins_ctx* ctx, const lins_segmented_scan* scans, const int32_t* n_imu, const double* const* imu, const double* scan_imu,
                         const double* scan_time, double scan_period, lins_result* out, int32_t* feature_counts, double* global_state_out,
                         int32_t* status_out) {
  if (!scans) return LINS_E_ARG;
  return process_impl(ctx, scans, nullptr, nullptr, n_imu, imu, scan_imu, scan_time, scan_period, out, feature_counts, global_state_out, status_out);
}

int lins_streams_process_raw(lins_ctx* ctx, const lins_point* const* raw, const int32_t* n_raw, const int32_t* n_imu, const double* const* imu,
                             const double* scan_imu, const double* scan_time, double scan_period, lins_result* out, int32_t* feature_counts,
                             double* global_state_out, int32_t* status_out) {
  if (!raw || !n_raw) return LINS_E_ARG;
  return process_impl(ctx, nullptr, raw, n_raw, n_imu, imu, scan_imu, scan_time, scan_period, out, feature_counts, global_state_out, status_out);
}

int lins_streams_status(lins_ctx* ctx, int32_t* status) {
  if (!ctx || !status) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed || !t.b.on) return LINS_E_STATE;
  for (int k = 0; k < t.n; ++k) status[k] = t.b.status[k];
  return LINS_OK;
}

int lins_streams_preintegration_get(lins_ctx* ctx, int stream, lins_preintegration* out) {
  if (!ctx || !out) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed || !t.b.on) return LINS_E_STATE;
  if (stream < 0 || stream >= t.n) return LINS_E_ARG;
  if (t.b.status[stream] != LINS_STREAM_FIRST_SCAN) return LINS_E_STATE;
  static_assert(sizeof(lins_preintegration) == kPre * 8, "lins_preintegration layout");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpyAsync(out, t.b.d_pre + (size_t)stream * kPre, kPre * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LINS_OK;
}

int lins_streams_lin_state(lins_ctx* ctx, double* lin_state) {
  if (!ctx || !lin_state) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpyAsync(lin_state, ctx->d_state_out, (size_t)t.n * 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LINS_OK;
}

int lins_streams_boot_stats(lins_ctx* ctx, float* preintegrate_ms, float* icp_ms, float* finish_ms) {
  if (!ctx) return LINS_E_ARG;
  auto& b = ctx->st.b;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (b.pre_timed) {
    HIP_TRY(ctx, hipEventSynchronize(b.ev[1]));
    HIP_TRY(ctx, hipEventElapsedTime(&b.pre_ms, b.ev[0], b.ev[1]));
  }
  if (b.icp_timed) {
    HIP_TRY(ctx, hipEventSynchronize(b.ev[3]));
    HIP_TRY(ctx, hipEventElapsedTime(&b.icp_ms, b.ev[2], b.ev[3]));
  }
  if (b.finish_timed) {
    HIP_TRY(ctx, hipEventSynchronize(b.ev[5]));
    HIP_TRY(ctx, hipEventElapsedTime(&b.finish_ms, b.ev[4], b.ev[5]));
  }
  if (preintegrate_ms) *preintegrate_ms = b.pre_ms;
  if (icp_ms) *icp_ms = b.icp_ms;
  if (finish_ms) *finish_ms = b.finish_ms;
  return LINS_OK;
}

}  // extern "C"
