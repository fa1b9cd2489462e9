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
