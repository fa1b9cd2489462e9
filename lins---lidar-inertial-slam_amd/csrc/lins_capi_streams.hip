// lins_capi_streams.hip — the device-resident streams of the C ABI (include/lins_ieskf.h, lins_streams_filter.h):
// lins_streams_init, the step every lins_streams_step* / lins_streams_process* call ends in (front-end -> IESKF update ->
// re-projection without the clouds leaving HBM), and the calls that read what a step left (lins_streams_map_cloud,
// _stats, _peek; lins_streams_put_outliers).  The step is a sequence of named phases over one per-call record (StepPlan);
// its update goes out through the batch path's launcher, run_family() in lins_capi.hip.
#include "lins_ctx.h"
#include "snapshot.h"

using namespace lins;

namespace {
// slot layout (points): [flat 512 | sharp 256 | less flat LINS_CLOUD_MAX | less sharp 1920]; the less-sharp cloud
// follows the less-flat one so that the multi-resident kernel's sorted copy (positions 0 .. n_all) stays in the slot
constexpr long long kSlotFlat = 0, kSlotSharp = 512, kSlotLessFlat = 768, kSlotLessSharp = 768 + LINS_CLOUD_MAX;
constexpr long long kSlotSize = kSlotLessSharp + 1920;
inline long long slot_base(int stream, int slot) { return ((long long)stream * 2 + slot) * kSlotSize; }

// a stream's descriptor: queries (flat, sharp) in its slot `qs`, targets (less flat, less sharp) in its slot `ts`
ScanDesc stream_desc(int stream, int qs, int n_flat, int n_sharp, int ts, int n_less_flat, int n_less_sharp) {
  const long long bq = slot_base(stream, qs), bt = slot_base(stream, ts);
  ScanDesc d{};
  d.off_surf_q = (int)(bq + kSlotFlat), d.n_surf_q = n_flat;
  d.off_corner_q = (int)(bq + kSlotSharp), d.n_corner_q = n_sharp;
  d.off_surf_t = (int)(bt + kSlotLessFlat), d.n_surf_t = n_less_flat;
  d.off_corner_t = (int)(bt + kSlotLessSharp), d.n_corner_t = n_less_sharp;
  d.surf_sorted = d.corner_sorted = 1;  // the front-end emits ring-major clouds with ring ids < 16
  d.slot_base = stream * LINS_MAX_QUERY, d.pad = 0;
  return d;
}
}  // namespace

namespace lins {
void streams_free(lins_ctx* ctx) { ctx->st = lins_ctx::Streams{}; }  // (with its filter, state machine and odometry records)

int streams_count(lins_ctx* ctx) { return ctx->st.failed ? 0 : ctx->st.n; }

int streams_map_clouds(lins_ctx* ctx, int stream, StreamMapClouds* v) {
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;
  if (stream < 0 || stream >= t.n) return LINS_E_ARG;
  if (t.last_counts[(size_t)stream * 2] < 0) return LINS_E_STATE;
  const int last = t.cur[stream] ^ 1;  // the slot of the scan taken in last
  const long long b = slot_base(stream, last);
  v->src[0] = t.d_arena + b + kSlotLessSharp, v->n[0] = t.last_counts[(size_t)stream * 2];
  v->src[1] = t.d_arena + b + kSlotLessFlat, v->n[1] = t.last_counts[(size_t)stream * 2 + 1];
  v->src[2] = t.d_outl + (size_t)(stream * 2 + last) * LINS_OUTLIER_MAX, v->n[2] = t.outl_counts[(size_t)stream * 2 + last];
  return LINS_OK;
}

// (snapshot.h) the two clouds a later step reads of a resident scan — less flat, less sharp: the next update's targets
// and the mapping node's input — where they lie in feature slot `slot` of `stream`, and what they hold at most
void streams_scan_place(int stream, int slot, int64_t off[2], int32_t caps[2], int64_t* slot_points) {
  const long long b = slot_base(stream, slot);
  off[0] = b + kSlotLessFlat, off[1] = b + kSlotLessSharp;
  caps[0] = LINS_CLOUD_MAX, caps[1] = (int32_t)(kSlotSize - kSlotLessSharp);
  if (slot_points) *slot_points = kSlotSize;
}
}  // namespace lins

namespace {

// What one step knows about its streams, filled phase by phase.
struct StepPlan {
  int n = 0;
  std::vector<int> st_in;   // the status each stream enters the step with (machine mode; otherwise every stream counts as running)
  std::vector<int> counts;  // per stream: sharp, less sharp, flat, less flat of this scan
  std::vector<int> n_outl;  // ... and its outlier count
  // gated[k]: the scan is not kept.  boot_mode[k]: the stream's first (1) / second (2) scan is dealt with behind the update
  std::vector<char> gated, unsupported;
  std::vector<int> boot_mode;
  bool any_gated = false;
  RangeFlags fl;           // what this step's descriptors can take ...
  Family fam{};            // ... and the family its update ran
  UpdateIo io{};           // where that update read and wrote
  bool idx_ready = false;  // the search index of the resident last scans exists

  const int* count(int k) const { return &counts[(size_t)k * 4]; }
  // the stream's scan is matched against its resident last one
  bool has_last(const lins_ctx::Streams& t, int k) const {
    return t.last_counts[(size_t)k * 2] >= 0 && !gated[k] && st_in[k] == LINS_STREAM_RUNNING;
  }
};

// 1. feature front-end, straight into this scan's slots (a rejected input has advanced nothing: only this scan's own slots
//    were touched)
int step_frontend(lins_ctx* ctx, const StepScans& in, StepPlan& p) {
  auto& t = ctx->st;
  const int n = p.n;
  std::vector<long long> offs((size_t)n * 4);
  for (int k = 0; k < n; ++k) {
    long long* o = &offs[(size_t)k * 4];
    const long long b = slot_base(k, t.cur[k]);
    o[0] = b + kSlotSharp, o[1] = b + kSlotLessSharp, o[2] = b + kSlotFlat, o[3] = b + kSlotLessFlat;
  }
  const auto* offs4 = reinterpret_cast<const long long(*)[4]>(offs.data());
  // this scan's outlier cloud: slot cur of the stream, as its feature clouds (the count of a segmented step: what
  // lins_streams_put_outliers left, else none)
  p.n_outl.assign((size_t)n, 0);
  if (in.segmented) {
    if (t.outl_pending) p.n_outl = t.outl_put;
    if (int rc = fe_run(ctx, n, in.segmented, in.scan_period, t.d_arena, offs4, p.counts)) return rc;
  } else {  // raw clouds: the image_projection stage on the device feeds the front-end where its output lies
    std::vector<int> o_slots((size_t)n);
    for (int k = 0; k < n; ++k) o_slots[k] = k * 2 + t.cur[k];
    if (int rc = sg_run(ctx, n, in.raw, in.n_raw, offs4, t.d_outl, o_slots.data())) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(p.n_outl.data(), ctx->fe.d_outliers, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipEventElapsedTime(&ctx->fe.sg_ms, ctx->ev0, ctx->ev2));
    if (int rc = fe_launch(ctx, n, in.scan_period, t.d_arena, p.counts, 0)) return rc;
  }
  t.frontend_ms = ctx->fe.ms;
  return LINS_OK;
}

// 2. On the filter path the prior is first propagated over the stream's IMU rows (behind the front-end, so that a
//    rejected input has advanced nothing), and a scan with too few features is gated (SE:436-440): no update, the
//    stream's resident clouds and slot stay the old scan's.
//    The state machine (mach): processImu by status — predict, pre-integrate, drop —; the bootstrap's own gate
//    (SE:332-333, 380-381: strict bounds); a stream that is not RUNNING gets no update (zero queries), its first or
//    second scan is dealt with behind the update (boot_mode: 1 / 2).
int step_gates(lins_ctx* ctx, const StepPrior& prior, StepPlan& p) {
  auto& t = ctx->st;
  const int n = p.n;
  p.gated.assign((size_t)n, 0), p.unsupported.assign((size_t)n, 0), p.boot_mode.assign((size_t)n, 0);
  const StepImu* imu = prior.imu;
  if (!imu) return LINS_OK;
  if (prior.mach) {
    std::vector<int32_t> n_run((size_t)n);
    for (int k = 0; k < n; ++k) n_run[k] = p.st_in[k] == LINS_STREAM_RUNNING ? imu->n_imu[k] : 0;
    if (int rc = streams_filter_predict_queue(ctx, n_run.data(), imu->rows)) return rc;
    if (int rc = streams_boot_preintegrate_queue(ctx, imu->n_imu, imu->rows)) return rc;
  } else if (int rc = streams_filter_predict_queue(ctx, imu->n_imu, imu->rows))
    return rc;
  for (int k = 0; k < n; ++k) {
    const int* c = p.count(k);
    if (p.st_in[k] == LINS_STREAM_RUNNING)
      p.gated[k] = c[1] <= 5 || c[3] <= 10;
    else {
      p.gated[k] = c[1] < 10 || c[3] < 100;
      if (!p.gated[k]) p.boot_mode[k] = p.st_in[k] == LINS_STREAM_INIT ? 1 : 2;
      if (p.boot_mode[k] == 2) {  // estimateTransform needs the device ICP: its caps, ICP_FREQ 1 (as the divergence fallback)
        const int n_all = t.last_counts[(size_t)k * 2] + t.last_counts[(size_t)k * 2 + 1];
        if (t.last_counts[(size_t)k * 2] < 0 || n_all > lds_mr_np_cap() || n_all > kGridNpMax || ctx->prm.icp_freq != 1)
          p.boot_mode[k] = 0, p.gated[k] = 1, p.unsupported[k] = 1;
      }
    }
    p.any_gated = p.any_gated || p.gated[k];
  }
  return LINS_OK;
}

// 3. IESKF update of every stream against its resident last scan (a stream's first scan: an update with no rows, which
//    leaves the given state — the bootstrap pose — untouched): descriptors, priors, launch, download (synchronises)
int step_update(lins_ctx* ctx, const StepPrior& prior, StepPlan& p) {
  auto& t = ctx->st;
  const int n = p.n;
  for (int k = 0; k < n; ++k) {
    const int* c = p.count(k);  // sharp, less sharp, flat, less flat
    const bool m = p.has_last(t, k);
    ctx->h_desc[k] = stream_desc(k, t.cur[k], m ? c[2] : 0, m ? c[0] : 0, t.cur[k] ^ 1, m ? t.last_counts[(size_t)k * 2 + 1] : 0,
                                 m ? t.last_counts[(size_t)k * 2] : 0);
  }
  p.fl = range_flags(ctx->h_desc, n);
  HIP_TRY(ctx, hipMemcpyAsync(t.d_desc, ctx->h_desc, (size_t)n * sizeof(ScanDesc), hipMemcpyHostToDevice, ctx->stream));
  if (!prior.imu) {
    std::memcpy(ctx->h_state, prior.state, (size_t)n * 19 * 8);
    std::memcpy(ctx->h_cov, prior.cov, (size_t)n * 324 * 8);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_state_in, ctx->h_state, (size_t)n * 19 * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cov_in, ctx->h_cov, (size_t)n * 324 * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  UpdateIo& io = p.io;
  io.desc = t.d_desc, io.arena = t.d_arena, io.gsorted = t.d_gsorted, io.gridtab = t.d_gridtab, io.binned = t.d_sorted;
  io.state_in = prior.imu ? t.f.d_state : ctx->d_state_in, io.cov_in = prior.imu ? t.f.d_cov : ctx->d_cov_in;
  io.state_out = ctx->d_state_out, io.cov_out = ctx->d_cov_out, io.a6 = ctx->d_a6, io.out = ctx->d_out, io.relay_lane = ctx->d_relay_lane;
  io.poses = nullptr, io.scan_id_base = 0, io.prof = nullptr;
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  p.fam = pick_family(ctx, n, p.fl);
  if (p.fam.use_mr || p.fam.use_lds) {
    p.idx_ready = true;
    // the search index of the last scan's clouds: left by the step before, which re-projected and indexed them in one
    // kernel (step_reproject) — built here only when that step could not (its first scan, another search mode)
    if (!t.index_ready) launch_grid_index(ctx->stream, n, t.d_desc, t.d_arena, t.d_gsorted, t.d_gridtab);
  }
  // What stays the step's own of the batch kernel's launch: the launch order only where this step's priors are on the host
  // (h_state; the filter path's are on the device: natural order, same results), and the several-part updates (more
  // streams than workgroup slots) whatever the phase profile and the launch queues say.
  const int* order = nullptr;
  RelayArgs ra;
  const bool relay = p.fam.use_mr && n > ctx->queue_grid && ctx->prm.icp_freq == 1 && ctx->d_relay_hdr && ctx->relay_at != 0 &&
                     relay_max_parts(ctx->prm.num_iter, ctx->relay_at, ctx->relay_cuts) > 1;
  const bool ordered = p.fam.use_mr && ctx->use_order && n > ctx->queue_grid && !prior.imu;
  if (ordered) {
    launch_order(ctx, n);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_order, ctx->h_order, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    order = ctx->d_order;
  }
  if (relay) {
    if (int rc = relay_prepare(ctx, n, ordered, ra)) return rc;
    order = ctx->d_order + ctx->max_batch;
  }
  run_family(ctx, p.fam, ctx->stream, p.io, n, order, relay ? &ra : nullptr);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_state, ctx->d_state_out, (size_t)n * 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_cov, ctx->d_cov_out, (size_t)n * 324 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, (size_t)n * sizeof(OutRec), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (int rc = relay_check(ctx)) return rc;  // (the guard marks the streams context failed: no stale posterior is re-projected)
  HIP_TRY(ctx, hipEventElapsedTime(&t.update_ms, ctx->ev0, ctx->ev1));
  return LINS_OK;
}

// 4. the caller's results of the update, and the per-stream ICP fall-back
int step_results(lins_ctx* ctx, const StepPrior& prior, StepPlan& p, lins_result* out) {
  auto& t = ctx->st;
  for (int k = 0; k < p.n; ++k) {
    lins_result& r = out[k];
    std::memset(&r, 0, sizeof r);
    std::memcpy(r.state, ctx->h_state + (size_t)k * 19, sizeof r.state);
    std::memcpy(r.cov, ctx->h_cov + (size_t)k * 324, sizeof r.cov);
    const OutRec& o = ctx->h_out[k];
    const bool m = p.has_last(t, k);
    r.residual_norm = o.residual_norm, r.update_norm = o.update_norm;
    r.iters = m ? o.iters : 0, r.converged = m ? o.converged : 0, r.diverged = m ? o.diverged : 0;
    r.m_surf = o.m_surf, r.m_corner = o.m_corner;
    if (!m && !prior.imu) {  // a stream's first scan: the given state and covariance, bit for bit (also as re-projection pose)
      std::memcpy(r.state, prior.state + (size_t)k * 19, sizeof r.state);
      std::memcpy(r.cov, prior.cov + (size_t)k * 324, sizeof r.cov);
      HIP_TRY(ctx, hipMemcpyAsync(ctx->d_state_out + (size_t)k * 19, ctx->d_state_in + (size_t)k * 19, 19 * 8, hipMemcpyDeviceToDevice,
                                  ctx->stream));
    }
    if (p.st_in[k] != LINS_STREAM_RUNNING) {  // the state machine's other streams: filled in behind the bootstrap (step_finish)
      std::memset(&r, 0, sizeof r);
      r.reserved[0] = p.unsupported[k] ? LINS_E_UNSUPPORTED : (p.gated[k] ? LINS_STREAMS_GATED : 0);
      continue;
    }
    if (!m && prior.imu) {  // a gated scan: the filter as predicted
      r.reserved[0] = LINS_STREAMS_GATED;
      HIP_TRY(ctx, hipMemcpyAsync(r.state, t.f.d_state + (size_t)k * 19, 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(r.cov, t.f.d_cov + (size_t)k * 324, 324 * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  if (p.any_gated) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // diverged filters: the ICP fallback (SE:585-592) on the same resident clouds, pose into the state row
  for (int k = 0; k < p.n; ++k) {
    if (!out[k].diverged) continue;
    if (!p.fl.mr_ok || ctx->prm.icp_freq != 1) {
      // this stream's clouds cannot take the device fallback: it keeps the un-updated filter (what performIESKF
      // holds before SE:585), flagged per stream — the other streams' step is not thrown away
      out[k].reserved[0] = LINS_E_UNSUPPORTED;
      continue;
    }
    if (!p.idx_ready) {  // (the update ran on the any-size kernel: no index yet)
      launch_grid_index(ctx->stream, p.n, t.d_desc, t.d_arena, t.d_gsorted, t.d_gridtab);
      p.idx_ready = true;
    }
    launch_lds_mr_icp(ctx->stream, 1, ctx->dprm, t.d_desc + k, t.d_arena, t.d_gsorted, t.d_gridtab + k, p.io.state_in + (size_t)k * 19,
                      ctx->d_state_out + (size_t)k * 19, ctx->d_out + k, ctx->d_idx);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out[k].state, ctx->d_state_out + (size_t)k * 19, 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (prior.imu) HIP_TRY(ctx, hipMemcpyAsync(out[k].cov, p.io.cov_in + (size_t)k * 324, 324 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!prior.imu) std::memcpy(out[k].cov, prior.cov + (size_t)k * 324, 324 * 8);  // Pk_ un-updated
  }
  return LINS_OK;
}

// 5. the filter path: filter_->update, integrateTransformation, reset(1), correctRollPitch on the device
//    (filter_finish_kernel reads the posterior rows and leaves them: the re-projection reads linState_ there); then
//    the state machine's first and second scans: processFirstScan / processSecondScan on the device — the ICP of all
//    second scans in one launch over their compact descriptor list (queries: this scan's flat / sharp clouds, targets:
//    the resident first scan's, as extracted), then the finish kernel, which leaves linState_ in the rows the
//    re-projection reads (identity for a first scan: its clouds stay as extracted)
int step_finish(lins_ctx* ctx, const StepPrior& prior, const StepPlan& p, lins_result* out) {
  auto& t = ctx->st;
  const int n = p.n;
  if (!prior.imu) return LINS_OK;
  std::vector<int> mode((size_t)n);
  for (int k = 0; k < n; ++k)
    mode[k] = p.gated[k] || p.st_in[k] != LINS_STREAM_RUNNING || (out[k].diverged && out[k].reserved[0] == LINS_E_UNSUPPORTED) ? 0 : (out[k].diverged ? 2 : 1);
  if (int rc = streams_filter_finish_queue(ctx, mode.data())) return rc;
  if (prior.mach) {
    std::vector<ScanDesc> icp;
    for (int k = 0; k < n; ++k) {
      if (p.boot_mode[k] != 2) continue;
      const int* c = p.count(k);
      icp.push_back(stream_desc(k, t.cur[k], c[2], c[0], t.cur[k] ^ 1, t.last_counts[(size_t)k * 2 + 1], t.last_counts[(size_t)k * 2]));
    }
    if (int rc = streams_boot_finish(ctx, p.boot_mode.data(), icp, *prior.mach, out)) return rc;
  }
  if (prior.imu->global_state_out)
    HIP_TRY(ctx, hipMemcpyAsync(prior.imu->global_state_out, t.f.d_gstate, (size_t)n * 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
  return LINS_OK;
}

// 6. updatePointCloud: this scan's less-sharp / less-flat clouds to the scan end with the final pose (device-resident
//    state rows), in place — they are the next step's targets — and, when the next step's update will search through
//    the LDS grid, their search index in the same pass (grid_index_kernel<true>: one read of the new clouds for the
//    re-projected arena copy, the grid-sorted copy and the tables; SURVEY f-2 "re-projection + target binning build").
//    (a gated stream keeps its old targets and their index: the step then runs the two kernels, and the next step builds
//    the index of every stream's resident clouds anew — same bits either way, tests/test_gpu_edge_cases.py)
int step_reproject(lins_ctx* ctx, double scan_period, const StepPlan& p) {
  auto& t = ctx->st;
  const int n = p.n;
  bool fuse = ctx->streams_fuse && p.fam.search >= SEARCH_LDS && !p.any_gated;
  for (int k = 0; k < n && fuse; ++k) {
    const int n_all = p.count(k)[1] + p.count(k)[3];
    if (n_all > kGridNpMax || n_all > (p.fam.search == SEARCH_MR ? lds_mr_np_cap() : lds_np_cap())) fuse = false;
  }
  int max_n = 1;
  if (fuse) {
    for (int k = 0; k < n; ++k) {  // (the update's descriptors have been consumed: its kernel has finished)
      const ScanDesc& u = ctx->h_desc[k];
      ctx->h_desc[k] = stream_desc(k, t.cur[k], u.n_surf_q, u.n_corner_q, t.cur[k], p.count(k)[3], p.count(k)[1]);
    }
    HIP_TRY(ctx, hipMemcpyAsync(t.d_desc_next, ctx->h_desc, (size_t)n * sizeof(ScanDesc), hipMemcpyHostToDevice, ctx->stream));
  } else {
    std::vector<StreamCloud> jobs((size_t)n * 2);
    for (int k = 0; k < n; ++k) {
      const int* c = p.count(k);
      const long long b = slot_base(k, t.cur[k]);
      const bool keep = !p.gated[k];  // (a gated scan: nothing of it becomes a target)
      jobs[(size_t)k * 2] = StreamCloud{b + kSlotLessSharp, keep ? c[1] : 0, k};
      jobs[(size_t)k * 2 + 1] = StreamCloud{b + kSlotLessFlat, keep ? c[3] : 0, k};
      if (keep) max_n = std::max(max_n, std::max(c[1], c[3]));
    }
    HIP_TRY(ctx, hipMemcpyAsync(t.d_jobs, jobs.data(), jobs.size() * sizeof(StreamCloud), hipMemcpyHostToDevice, ctx->stream));
  }
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if (fuse)
    launch_reproject_and_index(ctx->stream, n, t.d_desc_next, t.d_arena, t.d_gsorted, t.d_gridtab, ctx->d_state_out, (double)(1.f / (float)scan_period));
  else
    launch_reproject_in_place(ctx->stream, 2 * n, max_n, t.d_jobs, ctx->d_state_out, t.d_arena, (double)(1.f / (float)scan_period));
  t.index_ready = fuse;
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipEventElapsedTime(&t.reproject_ms, ctx->ev0, ctx->ev2));
  return LINS_OK;
}

// 7. what the step leaves: the kept scans' counts, slot flips, status_ after processPCL (SE:294-307)
void step_commit(lins_ctx* ctx, const StepPrior& prior, const StepPlan& p, int32_t* feature_counts) {
  auto& t = ctx->st;
  for (int k = 0; k < p.n; ++k) {
    const int* c = p.count(k);
    if (feature_counts) std::memcpy(feature_counts + (size_t)k * 4, c, 4 * sizeof(int));
    if (p.gated[k]) continue;
    t.last_counts[(size_t)k * 2] = c[1], t.last_counts[(size_t)k * 2 + 1] = c[3];
    t.outl_counts[(size_t)k * 2 + t.cur[k]] = p.n_outl[k];
    t.cur[k] ^= 1;
  }
  t.outl_pending = false;
  if (!prior.mach) return;
  for (int k = 0; k < p.n; ++k) {
    if (p.st_in[k] == LINS_STREAM_INIT && p.boot_mode[k] == 1) t.b.status[k] = LINS_STREAM_FIRST_SCAN;
    if (p.st_in[k] == LINS_STREAM_FIRST_SCAN && !p.unsupported[k]) {
      t.b.status[k] = p.boot_mode[k] == 2 ? LINS_STREAM_RUNNING : LINS_STREAM_INIT;
      if (p.boot_mode[k] != 2) t.f.set[k] = 0;  // (back to INIT: the stream has no filter until its next first scan)
    }
    if (prior.mach->status_out) prior.mach->status_out[k] = t.b.status[k];
  }
}

}  // namespace

int lins::streams_step_impl(lins_ctx* ctx, const StepScans& scans, const StepPrior& prior, lins_result* out, int32_t* feature_counts) {
  if (!ctx || !out || (!prior.imu && (!prior.state || !prior.cov))) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;  // (after a failed step: lins_streams_init again)
  if (prior.imu && !prior.mach) {  // every stream runs from its device filter against its resident last scan, or nothing is run
    if (int rc = streams_filter_check(ctx, prior.imu->n_imu, prior.imu->rows)) return rc;
    for (int k = 0; k < t.n; ++k)
      if (t.last_counts[(size_t)k * 2] < 0 || (t.b.on && t.b.status[k] != LINS_STREAM_RUNNING)) return LINS_E_STATE;
  }
  StepPlan plan;
  plan.n = t.n;
  plan.st_in = prior.mach ? t.b.status : std::vector<int>((size_t)t.n, LINS_STREAM_RUNNING);
  // A step either completes for every stream — slots flipped, resident clouds re-projected — or marks the streams
  // context failed: no half-advanced state survives an early return.
  struct Guard {
    bool& failed;
    bool done = false;
    ~Guard() {
      if (!done) failed = true;
    }
  } guard{t.failed};
  const CallTrace trace;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = split_join(ctx)) return rc;
  ctx->n_uploaded = 0, ctx->ran = false;  // the batch buffers are reused below
  if (int rc = step_frontend(ctx, scans, plan)) {
    guard.done = rc != LINS_E_HIP;  // (a rejected input has advanced nothing)
    return rc;
  }
  trace.mark("front-end done (synced)");
  if (int rc = step_gates(ctx, prior, plan)) return rc;
  if (int rc = step_update(ctx, prior, plan)) return rc;
  trace.mark("update done (synced)");
  if (int rc = step_results(ctx, prior, plan, out)) return rc;
  if (int rc = step_finish(ctx, prior, plan, out)) return rc;
  if (int rc = step_reproject(ctx, scans.scan_period, plan)) return rc;
  trace.mark("re-projection done (synced)");
  step_commit(ctx, prior, plan, feature_counts);
  guard.done = true;
  return LINS_OK;
}

extern "C" {

int lins_streams_init(lins_ctx* ctx, int n_streams) {
  if (!ctx || n_streams < 1) return LINS_E_ARG;
  if (n_streams > ctx->max_batch) return LINS_E_CAPACITY;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  streams_free(ctx);
  auto& t = ctx->st;
  const size_t pts = (size_t)n_streams * 2 * kSlotSize;
  if (pts >= (1ull << 31)) return LINS_E_CAPACITY;  // ScanDesc offsets are ints
  BUF_TRY(ctx, t.d_arena.grow(pts));
  BUF_TRY(ctx, t.d_sorted.grow(pts));
  BUF_TRY(ctx, t.d_gsorted.grow(pts));
  BUF_TRY(ctx, t.d_gridtab.grow((size_t)n_streams));
  BUF_TRY(ctx, t.d_desc.grow((size_t)n_streams));
  BUF_TRY(ctx, t.d_desc_next.grow((size_t)n_streams));
  t.index_ready = false;
  BUF_TRY(ctx, t.d_jobs.grow((size_t)n_streams * 2));
  BUF_TRY(ctx, t.d_outl.grow((size_t)n_streams * 2 * LINS_OUTLIER_MAX));
  t.outl_counts.assign((size_t)n_streams * 2, 0), t.outl_put.assign((size_t)n_streams, 0), t.outl_pending = false;
  t.n = n_streams, t.cur.assign((size_t)n_streams, 0);
  t.last_counts.assign((size_t)n_streams * 2, -1);
  return LINS_OK;
}

int lins_streams_step_imu(lins_ctx* ctx, const lins_segmented_scan* scans, const int32_t* n_imu, const double* const* imu,
                          double scan_period, lins_result* out, int32_t* feature_counts, double* global_state_out) {
  if (!scans) return LINS_E_ARG;
  const StepImu si{n_imu, imu, global_state_out};
  return streams_step_impl(ctx, StepScans{scans, nullptr, nullptr, scan_period}, StepPrior{nullptr, nullptr, &si, nullptr}, out, feature_counts);
}

int lins_streams_step_imu_raw(lins_ctx* ctx, const lins_point* const* raw, const int32_t* n_raw, const int32_t* n_imu,
                              const double* const* imu, double scan_period, lins_result* out, int32_t* feature_counts,
                              double* global_state_out) {
  if (!raw || !n_raw) return LINS_E_ARG;
  const StepImu si{n_imu, imu, global_state_out};
  return streams_step_impl(ctx, StepScans{nullptr, raw, n_raw, scan_period}, StepPrior{nullptr, nullptr, &si, nullptr}, out, feature_counts);
}

int lins_streams_step(lins_ctx* ctx, const lins_segmented_scan* scans, const double* prior_state, const double* prior_cov,
                      double scan_period, lins_result* out, int32_t* feature_counts) {
  if (!scans) return LINS_E_ARG;
  return streams_step_impl(ctx, StepScans{scans, nullptr, nullptr, scan_period}, StepPrior{prior_state, prior_cov, nullptr, nullptr}, out, feature_counts);
}

int lins_streams_step_raw(lins_ctx* ctx, const lins_point* const* raw, const int32_t* n_raw, const double* prior_state,
                          const double* prior_cov, double scan_period, lins_result* out, int32_t* feature_counts) {
  if (!raw || !n_raw) return LINS_E_ARG;
  return streams_step_impl(ctx, StepScans{nullptr, raw, n_raw, scan_period}, StepPrior{prior_state, prior_cov, nullptr, nullptr}, out, feature_counts);
}

int lins_streams_put_outliers(lins_ctx* ctx, const lins_point* const* outlier, const int32_t* n_outlier) {
  if (!ctx || !outlier || !n_outlier) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;
  for (int k = 0; k < t.n; ++k) {
    if (n_outlier[k] < 0 || n_outlier[k] > LINS_OUTLIER_MAX || (n_outlier[k] && !outlier[k])) return LINS_E_ARG;
    for (int i = 0; i < n_outlier[k]; ++i) {
      const lins_point& p = outlier[k][i];
      if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z) || !std::isfinite(p.intensity)) return LINS_E_INPUT;
    }
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  for (int k = 0; k < t.n; ++k)  // into the slot the next scan's clouds go to
    if (n_outlier[k])
      HIP_TRY(ctx, hipMemcpyAsync(t.d_outl + (size_t)(k * 2 + t.cur[k]) * LINS_OUTLIER_MAX, outlier[k], (size_t)n_outlier[k] * sizeof(float4),
                                  hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the caller's clouds may go once this returns)
  t.outl_put.assign(n_outlier, n_outlier + t.n), t.outl_pending = true;
  return LINS_OK;
}

int lins_streams_map_cloud(lins_ctx* ctx, int stream, int which, lins_point* out, int cap) {
  if (!ctx || which < 0 || which > 2) return LINS_E_ARG;
  StreamMapClouds v;
  if (int rc = streams_map_clouds(ctx, stream, &v)) return rc;
  const int cnt = v.n[which];
  if (cnt > cap) return LINS_E_CAPACITY;
  if (!cnt) return 0;
  if (!out) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpy(out, v.src[which], (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost));
  for (int i = 0; i < cnt; ++i) {  // the mapping node's axes (SE:1128-1131): (x, y, z) <- (y, z, x)
    const lins_point p = out[i];
    out[i] = lins_point{p.y, p.z, p.x, p.intensity};
  }
  return cnt;
}

int lins_streams_stats(lins_ctx* ctx, float* frontend_ms, float* update_ms, float* reproject_ms) {
  if (!ctx) return LINS_E_ARG;
  if (frontend_ms) *frontend_ms = ctx->st.frontend_ms;
  if (update_ms) *update_ms = ctx->st.update_ms;
  if (reproject_ms) *reproject_ms = ctx->st.reproject_ms;
  return LINS_OK;
}

/* test aid: one resident cloud of a stream back to the host (which: 0 less sharp, 1 less flat of the LAST scan) */
int lins_streams_peek(lins_ctx* ctx, int stream, int which, lins_point* out, int cap) {
  if (!ctx || !out || stream < 0 || stream >= ctx->st.n || which < 0 || which > 1) return LINS_E_ARG;
  auto& t = ctx->st;
  const int cnt = t.last_counts[(size_t)stream * 2 + which];
  if (cnt < 0) return LINS_E_STATE;
  if (cnt > cap) return LINS_E_CAPACITY;
  const long long b = slot_base(stream, t.cur[stream] ^ 1) + (which ? kSlotLessFlat : kSlotLessSharp);
  HIP_TRY(ctx, hipMemcpy(out, t.d_arena + b, (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost));
  return cnt;
}

}  // extern "C"
