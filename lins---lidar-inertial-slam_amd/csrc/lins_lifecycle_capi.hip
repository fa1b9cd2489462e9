// lins_lifecycle_capi.hip — ending streams in the C ABI (include/lins_lifecycle.h): the filter side's release — what
// lins_streams_init, the first lins_streams_filter_set and lins_streams_machine_init leave, for the streams named — and
// lins_streams_retire, which asks every initialised module first and then releases stream == slot in each of them
// (lifecycle.h: the modules' apply functions live in their own files).
#include "../../include/lins_lifecycle.h"
#include "boot_math.h"
#include "filter_init.h"
#include "lifecycle.h"
#include "lins_ctx.h"
#include "local_map.h"
#include "snapshot.h"

static_assert(lins_snap::kRowAux == lins_filt::kAux && lins_snap::kRowPre == lins_boot::kPre, "the rows of the snapshot's plan");

using namespace lins;
using namespace lins_boot;
using lins_filt::kAux;

namespace lins {

// Field for field what the init calls leave (lins_capi_streams.hip lins_streams_init, lins_capi_filter.hip
// streams_filter_alloc, lins_capi_boot.hip lins_streams_machine_init, lins_streams_slam_capi.hip records_refresh).  The
// filter's rows: machine mode starts them as the identity state (globalState_, SE:213) with zero covariance, noise,
// aux and pre-integration rows; without it the rows of a stream that has no filter are never read, and are zeroed.
int streams_release_apply(lins_ctx* ctx, int n, const int32_t* streams) {
  auto& t = ctx->st;
  if (n == 0) return LINS_OK;
  hipStream_t st = ctx->stream;
  double row[19] = {};
  if (t.b.on) lins_filt::store(identity_state(), row);
  for (int i = 0; i < n; ++i) {
    const size_t k = (size_t)streams[i];
    t.cur[k] = 0;
    t.last_counts[k * 2] = t.last_counts[k * 2 + 1] = -1;
    t.outl_counts[k * 2] = t.outl_counts[k * 2 + 1] = 0;
    t.outl_put[k] = 0;
    auto& f = t.f;
    if (f.d_state) {
      f.set[k] = 0, f.prm[k] = lins_filter_params{};
      HIP_TRY(ctx, hipMemcpyAsync(f.d_state + k * 19, row, sizeof row, hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, hipMemcpyAsync(f.d_gstate + k * 19, row, sizeof row, hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, hipMemsetAsync(f.d_cov + k * 324, 0, 324 * 8, st));
      HIP_TRY(ctx, hipMemsetAsync(f.d_noise + k * 144, 0, 144 * 8, st));
      HIP_TRY(ctx, hipMemsetAsync(f.d_aux + k * kAux, 0, kAux * 8, st));
    }
    auto& b = t.b;
    if (b.on) {
      b.status[k] = LINS_STREAM_INIT, b.imu_seen[k] = 0;
      std::fill(b.imu_last.begin() + k * 6, b.imu_last.begin() + k * 6 + 6, 0.0);
      HIP_TRY(ctx, hipMemsetAsync(b.d_pre + k * kPre, 0, kPre * 8, st));
    }
    auto& s = t.s;
    if (s.d_odom) {  // valid = 0 and zeros, as the records kernel writes for a stream without a globalState_
      std::memset(s.h_odom + k, 0, sizeof(lins_stream_odom));
      HIP_TRY(ctx, hipMemsetAsync(s.d_odom + k, 0, sizeof(lins_stream_odom), st));
    }
  }
  // the search index of the resident scans is rebuilt by the next step for every stream, as in a context whose streams
  // start together (the same bits as the index the step before left: tests/test_gpu_edge_cases.py)
  t.index_ready = false;
  HIP_TRY(ctx, hipStreamSynchronize(st));  // (row goes out of scope)
  return LINS_OK;
}

// ---- snapshot.h: the same fields, read into a blob and written from one.  The filter's rows travel when they can be
// read: in machine mode (the identity rows of a stream without a filter are read) or with a filter loaded.
void streams_snapshot_context(lins_ctx* ctx, SnapContext& c) {
  auto& t = ctx->st;
  c.modules |= LINS_SNAP_STREAM;
  c.facts.params = ctx->prm;
  c.facts.machine = t.b.on ? 1 : 0;
  if (t.b.on) c.facts.boot = t.b.prm, c.modules |= LINS_SNAP_BOOT;
  int64_t off[2], slot_points = 0;
  int32_t caps[2];
  streams_scan_place(0, 0, off, caps, &slot_points);
  c.base[LINS_SNAP_BUF_SCAN] = t.d_arena.get(), c.units[LINS_SNAP_BUF_SCAN] = 2 * slot_points * t.n;
  c.base[LINS_SNAP_BUF_OUTL] = t.d_outl.get(), c.units[LINS_SNAP_BUF_OUTL] = 2ll * LINS_OUTLIER_MAX * t.n;
  if (t.f.d_state) {
    c.modules |= LINS_SNAP_FILTER;
    double* rows[5] = {t.f.d_state.get(), t.f.d_cov.get(), t.f.d_noise.get(), t.f.d_aux.get(), t.f.d_gstate.get()};
    const int units[5] = {lins_snap::kRowState, lins_snap::kRowCov, lins_snap::kRowNoise, lins_snap::kRowAux, lins_snap::kRowState};
    for (int k = 0; k < 5; ++k) c.base[LINS_SNAP_BUF_F_STATE + k] = rows[k], c.units[LINS_SNAP_BUF_F_STATE + k] = (int64_t)units[k] * t.n;
  }
  if (t.b.on) c.base[LINS_SNAP_BUF_B_PRE] = t.b.d_pre.get(), c.units[LINS_SNAP_BUF_B_PRE] = (int64_t)lins_snap::kRowPre * t.n;
  if (t.s.d_odom) c.modules |= LINS_SNAP_ODOM, c.base[LINS_SNAP_BUF_ODOM] = t.s.d_odom.get(), c.units[LINS_SNAP_BUF_ODOM] = (int64_t)lins_snap::kRowOdom * t.n;
}

int streams_snapshot_describe(lins_ctx* ctx, int stream, SnapStream& s) {
  auto& t = ctx->st;
  const size_t k = (size_t)stream;
  const int last = t.cur[k] ^ 1;
  s.modules |= LINS_SNAP_STREAM;
  lins_snapshot_counts& c = s.counts;
  c.has_scan = t.last_counts[k * 2] >= 0;
  c.less_sharp = c.has_scan ? t.last_counts[k * 2] : 0, c.less_flat = c.has_scan ? t.last_counts[k * 2 + 1] : 0;
  c.outliers = c.has_scan ? t.outl_counts[k * 2 + last] : 0;
  int32_t caps[2];
  streams_scan_place(stream, last, s.place.scan_off, caps, nullptr);
  s.place.outl_off = (int64_t)(k * 2 + last) * LINS_OUTLIER_MAX, s.place.row = stream;
  lins_snapshot_stream_rec* r = s.host_section<lins_snapshot_stream_rec>(LINS_SNAP_SEC_STREAM_REC, 1);
  r->outl_put = t.outl_put[k];
  const bool rows = t.f.d_state && (t.b.on || t.f.set[k]);
  if (rows) s.modules |= LINS_SNAP_FILTER, r->filter_set = t.f.set[k] ? 1 : 0;
  if (rows && t.f.set[k]) r->filter_prm = t.f.prm[k];
  if (t.b.on) {
    s.modules |= LINS_SNAP_BOOT;
    r->status = t.b.status[k], r->imu_seen = t.b.imu_seen[k] ? 1 : 0;
    std::memcpy(r->imu_last, &t.b.imu_last[k * 6], sizeof r->imu_last);
  }
  if (t.s.d_odom && t.s.have) s.modules |= LINS_SNAP_ODOM;
  return LINS_OK;
}

int streams_restore_check(lins_ctx* ctx, int stream, lins_snapshot_limits& lim) {
  auto& t = ctx->st;
  const size_t k = (size_t)stream;
  if (t.cur[k] != 0 || t.last_counts[k * 2] != -1 || t.last_counts[k * 2 + 1] != -1 || t.outl_counts[k * 2] || t.outl_counts[k * 2 + 1] || t.outl_put[k])
    return LINS_E_STATE;
  if (t.f.d_state && t.f.set[k]) return LINS_E_STATE;
  if (t.b.on && (t.b.status[k] != LINS_STREAM_INIT || t.b.imu_seen[k])) return LINS_E_STATE;
  if (t.s.d_odom && t.s.have && t.s.h_odom[k].valid) return LINS_E_STATE;
  int64_t off[2];
  int32_t caps[2];
  streams_scan_place(stream, 1, off, caps, nullptr);
  lim.less_flat_max = caps[0], lim.less_sharp_max = caps[1], lim.outlier_max = LINS_OUTLIER_MAX;
  return LINS_OK;
}

int streams_restore_prepare(lins_ctx* ctx, uint32_t modules) {
  if (modules & LINS_SNAP_FILTER)
    if (int rc = streams_filter_alloc(ctx)) return rc;
  // (a context that has not derived its odometry records yet derives them now, for every stream: the blob's record
  // then replaces its stream's)
  if ((modules & LINS_SNAP_ODOM) && !(ctx->st.s.d_odom && ctx->st.s.have))
    if (int rc = lins_streams_odometry(ctx, nullptr)) return rc;
  return LINS_OK;
}

// the scan goes to feature slot 1 and the stream's next scan to slot 0: what a fresh stream's first step leaves, shifted
// by one scan — the results do not depend on the slot (the streams of a context alternate theirs independently)
void streams_restore_place(lins_ctx* ctx, int stream, const SnapView& v, SnapStream& s) {
  int32_t caps[2];
  streams_scan_place(stream, 1, s.place.scan_off, caps, nullptr);
  s.place.outl_off = (int64_t)(stream * 2 + 1) * LINS_OUTLIER_MAX, s.place.row = stream;
}

void streams_restore_apply(lins_ctx* ctx, int stream, const SnapView& v) {
  auto& t = ctx->st;
  const size_t k = (size_t)stream;
  const lins_snapshot_counts& c = v.info.counts;
  lins_snapshot_stream_rec r;
  std::memcpy(&r, v.sec(LINS_SNAP_SEC_STREAM_REC), sizeof r);
  t.cur[k] = 0;
  t.last_counts[k * 2] = c.has_scan ? c.less_sharp : -1, t.last_counts[k * 2 + 1] = c.has_scan ? c.less_flat : -1;
  t.outl_counts[k * 2] = 0, t.outl_counts[k * 2 + 1] = c.outliers;
  t.outl_put[k] = r.outl_put;
  if (v.info.modules & LINS_SNAP_FILTER) t.f.set[k] = (char)r.filter_set, t.f.prm[k] = r.filter_prm;
  if (v.info.modules & LINS_SNAP_BOOT) {
    t.b.status[k] = r.status, t.b.imu_seen[k] = (char)r.imu_seen;
    std::memcpy(&t.b.imu_last[k * 6], r.imu_last, sizeof r.imu_last);
  }
  if (v.info.modules & LINS_SNAP_ODOM) std::memcpy(t.s.h_odom + k, v.sec(LINS_SNAP_SEC_ODOM), sizeof(lins_stream_odom));
  t.index_ready = false;  // (as the release: the next step builds the search index of every resident scan anew)
}

}  // namespace lins

extern "C" {

int lins_streams_release(lins_ctx* ctx, int n, const int32_t* streams) {
  if (!ctx) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;
  if (int rc = release_list_check(n, streams, t.n)) return rc;
  if (int rc = ctx_quiesce(ctx)) return rc;
  return streams_release_apply(ctx, n, streams);
}

int lins_streams_retire(lins_ctx* ctx, int n, const int32_t* streams) {
  if (!ctx) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;
  // every initialised module is asked first: a stream is a slot of each of them
  const int sizes[5] = {t.n, streams_map_streams(ctx), local_map_slots(ctx), archive_slots(ctx), pose_graph_slots(ctx)};
  for (int limit : sizes)
    if (limit > 0)
      if (int rc = release_list_check(n, streams, limit)) return rc;
  if (n == 0) return LINS_OK;
  if (int rc = ctx_quiesce(ctx)) return rc;
  if (int rc = streams_release_apply(ctx, n, streams)) return rc;
  if (sizes[1])
    if (int rc = streams_map_release_apply(ctx, n, streams)) return rc;
  if (sizes[2])
    if (int rc = local_map_release_apply(ctx, n, streams)) return rc;
  if (sizes[3])
    if (int rc = archive_release_apply(ctx, n, streams, nullptr)) return rc;
  if (sizes[4])
    if (int rc = pose_graph_release_apply(ctx, n, streams)) return rc;
  return LINS_OK;
}

}  // extern "C"
