// lins_streams_slam_capi.hip — streams end to end in the C ABI (include/lins_streams_slam.h): the odometry records derived
// from the streams' resident globalState_ (lins_capi_filter.hip d_gstate), the mapping step that reads transformSum from
// them (the body is lins_streams_map_capi.hip streams_map_step_run), the transform fusion node, and the one call per scan
// that runs the state machine's step, the records, the mapping step and the fusion.  Kernels: odom_kernels.hip.
#include "lins_ctx.h"
#include "local_map.h"

using namespace lins;

namespace lins {

void streams_slam_free(lins_ctx* ctx) { ctx->st.s = lins_ctx::Streams::Slam{}; }

// the records of an earlier run are not this run's: lins_streams_machine_init and lins_streams_map_init call this
void streams_slam_reset(lins_ctx* ctx) { ctx->st.s.have = false; }

namespace {

int slam_alloc(lins_ctx* ctx) {
  auto& t = ctx->st;
  auto& s = t.s;
  if (s.d_odom) return LINS_OK;
  const size_t n = (size_t)t.n;
  BUF_TRY(ctx, s.d_odom.grow(n));
  BUF_TRY(ctx, s.h_odom.grow(n));
  BUF_TRY(ctx, s.d_ints.grow(n * 2));
  BUF_TRY(ctx, s.h_ints.grow(n * 2));
  BUF_TRY(ctx, s.d_fused.grow(n));
  BUF_TRY(ctx, s.h_fused.grow(n));
  return LINS_OK;
}

// every stream's record from globalState_ as it lies; the host copy follows (one kernel, one download, one synchronisation)
int records_refresh(lins_ctx* ctx) {
  auto& t = ctx->st;
  auto& s = t.s;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = split_join(ctx)) return rc;
  if (int rc = slam_alloc(ctx)) return rc;
  const int n = t.n;
  if (!t.f.d_gstate) {  // no stream has been given a filter: no globalState_ anywhere
    HIP_TRY(ctx, hipMemsetAsync(s.d_odom, 0, (size_t)n * sizeof(lins_stream_odom), ctx->stream));
  } else {
    // (machine mode: a first scan loads the zero-initialised filter, globalState_ comes with the second — SE:379-425)
    for (int k = 0; k < n; ++k) s.h_ints[k] = t.f.set[k] && (!t.b.on || t.b.status[k] == LINS_STREAM_RUNNING) ? 1 : 0;
    HIP_TRY(ctx, hipMemcpyAsync(s.d_ints, s.h_ints, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    launch_odom_records(ctx->stream, n, t.f.d_gstate, s.d_ints, s.d_odom);
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, hipMemcpyAsync(s.h_odom, s.d_odom, (size_t)n * sizeof(lins_stream_odom), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  s.have = true;
  return LINS_OK;
}

// the fusion kernel for the n streams named (checked by the caller: in range, records valid), into the pinned staging
int fuse_run(lins_ctx* ctx, int n, const int32_t* streams) {
  auto& s = ctx->st.s;
  const MapPoseRec* d_poses = streams_map_poses(ctx);
  if (!d_poses) return LINS_E_STATE;
  const int ns = ctx->st.n;
  for (int k = 0; k < n; ++k) s.h_ints[ns + k] = streams[k];
  HIP_TRY(ctx, hipMemcpyAsync(s.d_ints + ns, s.h_ints + ns, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  launch_odom_fuse(ctx->stream, n, s.d_ints + ns, d_poses, s.d_odom, s.d_fused);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(s.h_fused, s.d_fused, (size_t)n * sizeof(lins_fused_pose), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LINS_OK;
}

lins_map_step_result step_skipped() {
  lins_map_step_result r{};
  r.status = LINS_MAP_STEP_SKIPPED, r.ring_age = -1, r.archive_id = -1;
  return r;
}

}  // namespace
}  // namespace lins

extern "C" {

int lins_streams_odometry(lins_ctx* ctx, lins_stream_odom* out) {
  if (!ctx) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;
  if (int rc = records_refresh(ctx)) return rc;
  if (out) std::memcpy(out, t.s.h_odom, (size_t)t.n * sizeof(lins_stream_odom));
  return LINS_OK;
}

int lins_streams_map_step_resident(lins_ctx* ctx, int n, const int32_t* streams, const double* time, const lins_slam_imu* imu,
                                   lins_map_step_result* out) {
  if (!ctx || n < 0 || (n && (!streams || !time || !out))) return LINS_E_ARG;
  auto& t = ctx->st;
  const int nm = streams_map_streams(ctx);
  if (!nm || t.n <= 0 || t.failed || nm > t.n) return LINS_E_STATE;  // (nm > t.n: lins_streams_init since, with fewer streams)
  if (n > nm) return LINS_E_ARG;  // (the other refusals: streams_map_step_run, before anything of the step is queued)
  for (int k = 0; k < n; ++k)
    if (streams[k] < 0 || streams[k] >= nm) return LINS_E_ARG;
  if (int rc = records_refresh(ctx)) return rc;
  return streams_map_step_run(ctx, n, streams, MapStepIn{nullptr, t.s.d_odom, t.s.h_odom, time, imu}, out);
}

int lins_streams_fuse(lins_ctx* ctx, int n, const int32_t* streams, lins_fused_pose* out) {
  if (!ctx || n < 0 || (n && (!streams || !out))) return LINS_E_ARG;
  auto& t = ctx->st;
  const int nm = streams_map_streams(ctx);
  if (!nm || t.n <= 0 || t.failed || nm > t.n || !t.s.have) return LINS_E_STATE;
  if (n > nm) return LINS_E_ARG;
  for (int k = 0; k < n; ++k)
    if (streams[k] < 0 || streams[k] >= nm) return LINS_E_ARG;
  for (int k = 0; k < n; ++k)
    if (!t.s.h_odom[streams[k]].valid) return LINS_E_INPUT;
  if (n == 0) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = split_join(ctx)) return rc;
  if (int rc = fuse_run(ctx, n, streams)) return rc;
  std::memcpy(out, t.s.h_fused, (size_t)n * sizeof(lins_fused_pose));
  return LINS_OK;
}

int lins_streams_slam_step(lins_ctx* ctx, const lins_point* const* raw, const int32_t* n_raw, const int32_t* n_imu, const double* const* imu,
                           const double* scan_imu, const double* scan_time, double scan_period, const lins_slam_imu* imu_rp, lins_result* results,
                           int32_t* status, lins_map_step_result* map, lins_fused_pose* fused) {
  if (!ctx || !raw || !n_raw || !scan_time || !results || !status || !map || !fused) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed || !t.b.on || streams_map_streams(ctx) != t.n) return LINS_E_STATE;
  const int n = t.n;
  // processImu + processPCL of every stream, whatever its status
  if (int rc = lins_streams_process_raw(ctx, raw, n_raw, n_imu, imu, scan_imu, scan_time, scan_period, results, nullptr, nullptr, status)) return rc;
  // publishOdometryYZX + laserOdometryHandler
  if (int rc = records_refresh(ctx)) return rc;
  // the mapping node's run() for the streams the estimator publishes for
  std::vector<int32_t> run;
  std::vector<double> time;
  std::vector<lins_slam_imu> rp;
  for (int k = 0; k < n; ++k) {
    map[k] = step_skipped();
    fused[k] = lins_fused_pose{};
    if (status[k] != LINS_STREAM_RUNNING) continue;
    run.push_back(k), time.push_back(scan_time[k]);
    if (imu_rp) rp.push_back(imu_rp[k]);
  }
  const int nr = (int)run.size();
  if (nr == 0) return LINS_OK;
  std::vector<lins_map_step_result> res((size_t)nr);
  if (int rc = streams_map_step_run(ctx, nr, run.data(), MapStepIn{nullptr, t.s.d_odom, t.s.h_odom, time.data(), imu_rp ? rp.data() : nullptr},
                                    res.data()))
    return rc;
  for (int j = 0; j < nr; ++j) map[run[j]] = res[j];
  // the transform fusion node, behind the mapping step, for the same streams
  std::vector<int32_t> fz;
  for (int j = 0; j < nr; ++j)
    if (t.s.h_odom[run[j]].valid) fz.push_back(run[j]);
  if (fz.empty()) return LINS_OK;
  if (int rc = fuse_run(ctx, (int)fz.size(), fz.data())) return rc;
  for (size_t j = 0; j < fz.size(); ++j) fused[fz[j]] = t.s.h_fused[j];
  return LINS_OK;
}

}  // extern "C"
