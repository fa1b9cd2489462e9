// lins_capi.hip — implementation of the C ABI in include/lins_ieskf.h.
//
// Owns: one HIP stream, the device arena (all four clouds of every uploaded scan
// pair, 64-byte aligned spans of float4), per-scan descriptors, prior / posterior
// state + covariance, and pinned host staging.  Caller owns every host buffer it
// passes in; nothing is retained after a call returns.

#include "lifecycle.h"
#include "lins_ctx.h"

using namespace lins;

namespace {

void pipe_free(lins_ctx* ctx) {
  auto& q = ctx->pipe;
  if (q.s_comm) (void)hipStreamSynchronize(q.s_comm), (void)hipStreamDestroy(q.s_comm);
  for (int k = 0; k < 2; ++k) {
    if (q.ev_comm[k]) (void)hipEventDestroy(q.ev_comm[k]);
  }
  q = lins_ctx::Pipe{};
}

// input contract: finite fields, int(intensity) in [0, LINS_MAX_RING) — the relative-time
// fraction may be slightly negative (SE:631-650 produces -0.025..0.125), and C truncation
// maps (-1, 0) to ring 0 exactly as the reference's int() does; reports ring-sortedness
// (packed 16-byte points: the arena's own layout — also what a strided cloud is checked as after it was gathered there)
int check_cloud(const lins_point* p, int n, bool* sorted) {
  int prev = -1;
  bool s = true;  // "grid-able": ring-sorted and every ring id < 16 (binned search precondition)
  for (int i = 0; i < n; ++i) {
    if (!std::isfinite(p[i].x) || !std::isfinite(p[i].y) || !std::isfinite(p[i].z) || !std::isfinite(p[i].intensity))
      return LINS_E_INPUT;
    if (p[i].intensity <= -1.f || p[i].intensity >= (float)LINS_MAX_RING) return LINS_E_INPUT;
    int r = (int)p[i].intensity;
    if (r < prev || r >= 16) s = false;
    prev = r;
  }
  if (sorted) *sorted = s;
  return LINS_OK;
}

void make_dev_params(const lins_params& p, int search, DevParams& d) {
  d.num_iter = p.num_iter;
  d.icp_freq = p.icp_freq;
  d.fixed_iters = p.fixed_iters;
  d.search = search;
  d.r2 = p.lidar_std * p.lidar_std;
  d.lidar_scale = p.lidar_scale;
  d.inv_period = (double)(1.f / p.scan_period);  // (1.f / SCAN_PERIOD), SE:1067
  d.nearest = p.nearest_sq_dist;
  d.nearest_f = (float)p.nearest_sq_dist;
  d.pad = 0;
  d.margin_cold = 0.20f;  // (metres; swept on the batch workload after the late iterations got cheaper: 0.10 / 0.04 -> 0.789 ms, 0.20 / 0.08 -> 0.771 ms)
  d.margin_warm = 0.08f;
  d.reseed_drift = 0.15f;  // (metres; any value gives the same results: it only picks between two bounds of an exact search)
  d.pad2 = 0;
  // Tuning / profiling knobs, honoured only when LINS_ENABLE_DEBUG_KNOBS=1 is set as well: a stray variable in a
  // production environment changes nothing.  The margins only trade search work for certificate hits (any value
  // >= 0 gives the same results); LINS_DEBUG_SKIP deliberately breaks the searches (profiling aid).
  const char* gate = std::getenv("LINS_ENABLE_DEBUG_KNOBS");
  if (gate && gate[0] == '1') {
    if (const char* e = std::getenv("LINS_MARGIN_COLD")) d.margin_cold = std::max(0.f, (float)std::atof(e));
    if (const char* e = std::getenv("LINS_MARGIN_WARM")) d.margin_warm = std::max(0.f, (float)std::atof(e));
    if (const char* e = std::getenv("LINS_RESEED_DRIFT")) d.reseed_drift = std::max(0.f, (float)std::atof(e));
    if (const char* e = std::getenv("LINS_DEBUG_SKIP")) d.pad = std::atoi(e);  // 1 = skip walks, 2 = skip search, 8 = verify
  }
}

// pass 1 (serial, cheap): argument checks and the arena layout of the whole batch
int layout_batch(lins_ctx* ctx, int n, const lins_scan_pair* in, size_t* arena_used, size_t* slots_used, uint64_t* bytes_iter) {
  if (!ctx || !in || n < 0) return LINS_E_ARG;
  if (n > ctx->max_batch) return LINS_E_CAPACITY;
  size_t off = 0, slots = 0;
  uint64_t bytes = 0;
  for (int s = 0; s < n; ++s) {
    const lins_scan_pair& p = in[s];
    if (p.n_surf_flat < 0 || p.n_corner_sharp < 0 || p.n_surf_last < 0 || p.n_corner_last < 0) return LINS_E_ARG;
    if (p.point_stride_bytes != 0 && p.point_stride_bytes != 16 && p.point_stride_bytes != 32) return LINS_E_ARG;
    if ((p.n_surf_flat && !p.surf_flat) || (p.n_corner_sharp && !p.corner_sharp) ||
        (p.n_surf_last && !p.surf_less_flat_last) || (p.n_corner_last && !p.corner_less_sharp_last))
      return LINS_E_ARG;
    if (p.n_surf_flat > LINS_MAX_QUERY || p.n_corner_sharp > LINS_MAX_QUERY) return LINS_E_CAPACITY;
    if (p.n_surf_last > ctx->max_targets || p.n_corner_last > ctx->max_targets) return LINS_E_CAPACITY;
    ScanDesc& d = ctx->h_desc[s];
    const int cnt[4] = {p.n_surf_flat, p.n_corner_sharp, p.n_surf_last, p.n_corner_last};
    int offs[4];
    for (int c = 0; c < 4; ++c) {
      if (off + align4(cnt[c]) > ctx->arena_cap) return LINS_E_CAPACITY;
      offs[c] = (int)off;
      off += align4(cnt[c]);
    }
    d.off_surf_q = offs[0], d.n_surf_q = cnt[0];
    d.off_corner_q = offs[1], d.n_corner_q = cnt[1];
    d.off_surf_t = offs[2], d.n_surf_t = cnt[2];
    d.off_corner_t = offs[3], d.n_corner_t = cnt[3];
    d.slot_base = (int)slots;
    d.pad = 0;
    slots += cnt[0] + cnt[1];
    if (slots > ctx->slot_cap) return LINS_E_CAPACITY;
    bytes += 16ull * (cnt[0] + cnt[1] + cnt[2] + cnt[3]) + 8 * 19 + 8 * 28;
  }
  *arena_used = off, *slots_used = slots, *bytes_iter = bytes;
  return LINS_OK;
}

// pass 2 for one scan: input contract + packing into the pinned staging arena
int pack_one(lins_ctx* ctx, const lins_scan_pair* in, int s) {
  const lins_scan_pair& p = in[s];
  ScanDesc& d = ctx->h_desc[s];
  bool ss = true, cs = true;
  int r;
  // The clouds go to the pinned staging arena first — a copy for packed points, a gather of the 16 payload bytes for
  // pcl::PointXYZI arrays (point_stride_bytes 32), nothing at all for clouds the caller already wrote there
  // (lins_batch_map) — and are validated where they then lie.
  const lins_point* src[4] = {p.surf_flat, p.corner_sharp, p.surf_less_flat_last, p.corner_less_sharp_last};
  const int cnt[4] = {d.n_surf_q, d.n_corner_q, d.n_surf_t, d.n_corner_t};
  const int offs[4] = {d.off_surf_q, d.off_corner_q, d.off_surf_t, d.off_corner_t};
  for (int c = 0; c < 4; ++c) {
    lins_point* dst = reinterpret_cast<lins_point*>(ctx->h_arena + offs[c]);
    // (a cloud that lies in the staging arena but not where THIS layout wants it was mapped for another batch shape:
    // moving it would race with the packing of its neighbours — refused, lins_batch_map's contract is same n, same sizes)
    if (cnt[c] && src[c] != dst && reinterpret_cast<const float4*>(src[c]) >= ctx->h_arena &&
        reinterpret_cast<const float4*>(src[c]) < ctx->h_arena + ctx->arena_cap)
      return LINS_E_ARG;
    // (a cloud that already lies at its arena slot is packed 16-byte points by construction — lins_batch_map hands out
    // lins_point arrays; a pair that claims the 32-byte stride for it would be misread in silence: refused)
    if (cnt[c] && src[c] == dst && p.point_stride_bytes == 32) return LINS_E_ARG;
    if (cnt[c] && src[c] != dst) {
      if (p.point_stride_bytes == 32)
        for (int i = 0; i < cnt[c]; ++i) dst[i] = lins_point_load(src[c], 32, i);
      else
        std::memcpy(dst, src[c], sizeof(lins_point) * cnt[c]);
    }
    for (size_t k2 = cnt[c]; k2 < align4(cnt[c]); ++k2) ctx->h_arena[offs[c] + k2] = make_float4(0, 0, 0, 0);
  }
  const lins_point* at[4];
  for (int c = 0; c < 4; ++c) at[c] = reinterpret_cast<const lins_point*>(ctx->h_arena + offs[c]);
  if ((r = check_cloud(at[0], cnt[0], nullptr))) return r;
  if ((r = check_cloud(at[1], cnt[1], nullptr))) return r;
  if ((r = check_cloud(at[2], cnt[2], &ss))) return r;
  if ((r = check_cloud(at[3], cnt[3], &cs))) return r;
  d.surf_sorted = ss, d.corner_sorted = cs;
  std::memcpy(ctx->h_state + (size_t)s * 19, p.state, sizeof p.state);
  std::memcpy(ctx->h_cov + (size_t)s * 324, p.cov, sizeof p.cov);
  return 0;
}

// search index of scans [lo, lo + cnt) of the uploaded descriptors, on the context's stream (grid kernels only: scans
// that cannot take them run the any-size kernel, which bins for itself)
int build_index_range(lins_ctx* ctx, int lo, int cnt, const RangeFlags& fl) {
  if (cnt <= 0 || !(fl.lds_ok || fl.mr_ok)) return LINS_OK;
  launch_grid_index(ctx->stream, cnt, ctx->d_desc + lo, ctx->d_arena, ctx->d_gsorted, ctx->d_gridtab + lo);
  HIP_TRY(ctx, hipGetLastError());
  return LINS_OK;
}

// host -> device of scans [lo, hi) (their arena slice is contiguous), asynchronous on `st`
int h2d_range(lins_ctx* ctx, int lo, int hi, size_t arena_end, hipStream_t st) {
  if (hi <= lo) return LINS_OK;
  const size_t a0 = (size_t)ctx->h_desc[lo].off_surf_q;
  if (arena_end > a0)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_arena + a0, ctx->h_arena + a0, (arena_end - a0) * sizeof(float4), hipMemcpyHostToDevice, st));
  if (lo == 0 && hi == ctx->max_batch) {  // the whole context: priors and descriptors are one block (lins_ctx::h_meta)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_meta_in, ctx->h_meta, ctx->meta_in_bytes, hipMemcpyHostToDevice, st));
    return LINS_OK;
  }
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_desc + lo, ctx->h_desc + lo, (size_t)(hi - lo) * sizeof(ScanDesc), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_state_in + (size_t)lo * 19, ctx->h_state + (size_t)lo * 19, (size_t)(hi - lo) * 19 * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cov_in + (size_t)lo * 324, ctx->h_cov + (size_t)lo * 324, (size_t)(hi - lo) * 324 * 8, hipMemcpyHostToDevice, st));
  return LINS_OK;
}

// The second launch queue of a context (lins_set_launch_queues): created when a batch beyond the workgroup slots is uploaded —
// not inside the first run that uses it, where the stream and its 2 x 64 timing events cost that run a millisecond or more
// (round 6: the bench's queued stop-rule figure read 1.12 instead of 0.89 ms for it) — and, as a fallback, by that run.
int split_prepare(lins_ctx* ctx) {
  if (ctx->stream2) return LINS_OK;
  // A priority of its own: HIP multiplexes the streams of a process onto a handful of hardware queues (four by default) in
  // creation order, and two streams that share one are served in order — measured: a context whose two streams collided
  // ran its queued steps at 0.646 instead of 0.50 ms, depending on how many other contexts the process had created
  // (gpurun r06w).  Streams of different priority never share a hardware queue.  LOW, so that the work a caller puts on
  // streams of his own is not pushed back by it.
  int pr_least = 0, pr_greatest = 0;
  HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
  HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, pr_least));
  HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
  for (int k = 0; k < lins_ctx::kHist; ++k) {
    HIP_TRY(ctx, hipEventCreate(&ctx->hist0b[k]));
    HIP_TRY(ctx, hipEventCreate(&ctx->hist1b[k]));
  }
  return LINS_OK;
}

void set_batch_state(lins_ctx* ctx, int n, const RangeFlags& fl, size_t slots, uint64_t bytes) {
  ctx->n_uploaded = n;
  ctx->fl = fl;
  ctx->slots_uploaded = slots;
  ctx->ran = false;
  ctx->bytes_per_iter = bytes;
}

size_t queue_ints(const lins_ctx* ctx) {  // counters, one flag per scan, the debug trace (8 ints per workgroup, <= 15 per scan)
  return (size_t)lds_mr_queue_flags_offset() + (size_t)ctx->max_batch * (1 + 15 * 8);
}

// (wait = false: the caller synchronises the stream itself before it returns to its own caller — the single-call entry
// points, whose download waits anyway: one host wait per call instead of two)
int upload(lins_ctx* ctx, int n, const lins_scan_pair* in, bool wait = true) {
  {  // (pipelined mode: the side streams may still read the inputs this call replaces)
    int rcj = pipe_join(ctx);
    if (rcj) return rcj;
  }
  const CallTrace tr;  // (stage times on stderr: LINS_ENABLE_DEBUG_KNOBS=1 LINS_BATCH_TRACE=1)
  size_t off = 0, slots = 0;
  uint64_t bytes = 0;
  int rc = layout_batch(ctx, n, in, &off, &slots, &bytes);
  if (rc) return rc;
  tr.mark("upload: layout");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if ((rc = parallel_scans(n, [&](int s) { return pack_one(ctx, in, s); }))) return rc;
  tr.mark("upload: validate + pack");
  const RangeFlags fl = range_flags(ctx->h_desc, n);
  tr.mark("upload: range flags");
  if ((rc = h2d_range(ctx, 0, n, off, ctx->stream))) return rc;
  tr.mark("upload: copies queued");
  // the target clouds have arrived: their search index (the reference builds its kd-trees where it produces the
  // clouds, SE:1156-1160, not in performIESKF)
  // (timed by its own events for lins_last_index_ms — at the staged lins_batch_upload only: in the single-call entry points,
  // which a live filter waits for, two event records are ~10 us of in-order latency on the stream, tools/experiments/graph_latency.hip)
  if (wait) HIP_TRY(ctx, hipEventRecord(ctx->ev_idx0, ctx->stream));
  if ((rc = build_index_range(ctx, 0, n, fl))) return rc;
  if (wait) HIP_TRY(ctx, hipEventRecord(ctx->ev_idx1, ctx->stream));
  ctx->idx_timed = wait;
  tr.mark("upload: index queued");
  launch_order(ctx, n);
  if (ctx->max_batch > 1)  // (a one-scan context: the order is [0], which is what the array holds since lins_create)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_order, ctx->h_order, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  if (wait) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->split_mode && n > ctx->queue_grid)  // (a batch whose queued runs go out on two launch queues: the second one exists before the first run)
    if (int rcq = split_prepare(ctx)) return rcq;
  set_batch_state(ctx, n, fl, slots, bytes);
  return LINS_OK;
}

// where the update of scans [lo, ...) of the uploaded batch reads and writes; `poses` / `scan_id_base`: of scan 0 of the batch
UpdateIo batch_io(const lins_ctx* ctx, int lo, lins_pose_record* poses, int32_t scan_id_base, long long* prof) {
  UpdateIo io;
  io.desc = ctx->d_desc + lo, io.arena = ctx->d_arena, io.gsorted = ctx->d_gsorted, io.gridtab = ctx->d_gridtab + lo, io.binned = ctx->d_binned;
  io.state_in = ctx->d_state_in + (size_t)lo * 19, io.cov_in = ctx->d_cov_in + (size_t)lo * 324;
  io.state_out = ctx->d_state_out + (size_t)lo * 19, io.cov_out = ctx->d_cov_out + (size_t)lo * 324, io.a6 = ctx->d_a6 + (size_t)lo * 21;
  io.out = ctx->d_out + lo, io.relay_lane = ctx->d_relay_lane + (size_t)lo * kRelayLaneInts;
  io.poses = poses ? poses + lo : nullptr, io.scan_id_base = scan_id_base + lo, io.prof = prof;
  return io;
}

// The kernels of scans [lo, lo + cnt) of the uploaded batch on the context's stream (no events, no state)
int run_range(lins_ctx* ctx, int lo, int cnt, int n_total, const RangeFlags& fl, lins_pose_record* poses, int32_t scan_id_base,
              hipStream_t st = nullptr) {
  if (!st) st = ctx->stream;
  const Family fam = pick_family(ctx, n_total, fl);
  ctx->last_search = fam.ran;
  run_family(ctx, fam, st, batch_io(ctx, lo, poses, scan_id_base, nullptr), cnt, nullptr, nullptr);
  HIP_TRY(ctx, hipGetLastError());
  return LINS_OK;
}

}  // namespace

namespace lins {

hipStream_t ctx_stream(lins_ctx* ctx) { return ctx->stream; }
int ctx_device(lins_ctx* ctx) { return ctx->device; }
int ctx_fail_hip(lins_ctx* ctx, hipError_t e, const char* what) {
  if (ctx) ctx->hip_err = std::string(what) + ": " + hipGetErrorString(e);
  return LINS_E_HIP;
}
void** ctx_map_slot(lins_ctx* ctx, void (*free_fn)(void*)) {
  ctx->map_state_free = free_fn;
  return &ctx->map_state;
}
void ctx_events(lins_ctx* ctx, hipEvent_t* a, hipEvent_t* b) { *a = ctx->ev0, *b = ctx->ev2; }
const lins_params* ctx_params(const lins_ctx* ctx) { return &ctx->prm; }

// Everything the side streams of the pipelined mode still have in flight is ordered before what is enqueued on the
// main stream next (no host wait).  Called by every staged entry point that touches buffers the side streams read.
// Order the context's stream behind whatever the second launch queue still runs, and mark that queue as behind the
// context's stream (the next split run forks again).  Called by every entry point that enqueues on ctx->stream or reads
// what the update kernels wrote; lins_batch_run() itself does not join (see lins_ctx::stream2).
int split_join(lins_ctx* ctx) {
  ctx->split_dirty = true;
  if (ctx->split_pending) {
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->hist1b[ctx->split_h], 0));
    ctx->split_pending = false;
  }
  return LINS_OK;
}

// (lifecycle.h) what every release call does before it touches state: nothing of the context is still running
int ctx_quiesce(lins_ctx* ctx) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = split_join(ctx)) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LINS_OK;
}

int pipe_join(lins_ctx* ctx) {
  if (int rc = split_join(ctx)) return rc;
  auto& q = ctx->pipe;
  for (int k = 0; k < 2; ++k) {
    if (q.comm_pending[k]) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, q.ev_comm[k], 0));
    q.comm_pending[k] = false;
  }
  return LINS_OK;
}

// Which kernel family a batch runs.  "auto": one workgroup per CU is all a small batch can use — the 1024-thread kernel
// gives each scan the shortest critical path; beyond that the multi-resident kernel keeps two scans per CU.
// The 3-lane shape is the single-round kernel: query sets beyond its kLds3QueryMax slots (more than a VLP-16
// front-end can emit) take the 1-lane shapes, whose several-rounds path is the tested one.
// (`n_total`: the batch a range belongs to — "auto" picks the family by the batch, so that a scan's bits do not depend
// on how the batch was cut; `fl`: what the scans to launch can take)
Family pick_family(const lins_ctx* ctx, int n_total, const RangeFlags& fl) {
  int s = ctx->dprm.search;
  if (s == SEARCH_AUTO) s = n_total > ctx->n_cu ? (int)SEARCH_MR : (int)SEARCH_LDS3;
  if (s == SEARCH_LDS3 && !fl.lds3_ok) s = SEARCH_LDS;
  const bool want_lds = s >= SEARCH_LDS, want_mr = s == SEARCH_MR;
  const bool use_mr = want_mr && fl.mr_ok, use_lds = want_lds && !want_mr && fl.lds_ok;
  return Family{s, use_mr, use_lds, use_mr ? (int)SEARCH_MR : (use_lds ? s : (want_lds ? (int)SEARCH_BINNED : s))};
}

// kernel eligibility of the n scans the (host) descriptors describe
RangeFlags range_flags(const ScanDesc* desc, int n) {
  RangeFlags fl{true, true, true};
  for (int s = 0; s < n; ++s) {
    const ScanDesc& d = desc[s];
    const bool grid = d.surf_sorted && d.corner_sorted;
    if (!grid || d.n_surf_t + d.n_corner_t > lds_np_cap()) fl.lds_ok = false;
    if (!grid || d.n_surf_t + d.n_corner_t > lds_mr_np_cap()) fl.mr_ok = false;
    if (d.n_surf_q + d.n_corner_q > kLds3QueryMax) fl.lds3_ok = false;
  }
  return fl;
}

// The update kernels of `cnt` scans on `st`, by the family picked for them, reading and writing where `io` says (no events, no
// state besides the launch number): the one launch site of an update, for the batch calls and the streams step alike.
// `order` / `relay`: launch order and several-part updates of the batch kernel (null: index order, whole updates).
void run_family(lins_ctx* ctx, const Family& fam, hipStream_t st, const UpdateIo& io, int cnt, const int* order, const RelayArgs* relay) {
  if (fam.use_mr) {
    launch_lds_mr(st, cnt, ctx->dprm, io.desc, order, io.arena, io.gsorted, io.gridtab, io.state_in, io.cov_in, io.state_out, io.a6, io.cov_out, io.out, ctx->d_idx,
                  io.poses, io.scan_id_base, io.prof, relay, ctx->d_walk_cache, next_run_gen(ctx), io.relay_lane);
  } else if (fam.use_lds) {
    launch_lds(st, cnt, ctx->dprm, fam.search == SEARCH_LDS3 ? 3 : 1, io.desc, io.arena, io.gsorted, io.gridtab, io.state_in, io.cov_in, io.state_out, io.a6, io.cov_out,
               io.out, ctx->d_idx, io.poses, io.scan_id_base, io.prof, io.relay_lane);  // (the Joseph update is the kernels' epilogue)
  } else {
    DevParams dp = ctx->dprm;
    dp.search = fam.ran;  // a scan does not fit LDS: global-memory grid
    launch_persistent(st, cnt, dp, io.desc, io.arena, io.state_in, io.cov_in, io.state_out, io.cov_out, io.a6, io.out, ctx->d_idx, io.poses, io.scan_id_base,
                      io.binned, io.prof);
  }
}

// Launch order of a batch on the multi-resident kernel: 1024 workgroups on 512 slots is two "rounds", and the dispatcher
// hands workgroups out in index order — so the launch ends when the slowest pairing of an early and a late workgroup
// does.  Listing the scans longest-expected-first (LPT) lets the short ones fill the end.  What the host knows before
// the launch: cloud sizes (R^2 = 0.004 against measured workgroup times — useless) and the prior; the prior's
// translation |p| (= how far the clouds are apart before the first iteration, hence how many re-searches the first
// iterations need) correlates 0.40.  Measured on the batch workload (tools/wg_cost_model.py, list-scheduling model on
// measured per-workgroup times: as submitted 843 us, by |p| 731 us, by the true durations 726 us, perfectly divisible
// work 583 us).  Results do not depend on the order (one workgroup per scan, no cross-scan state).
void launch_order(lins_ctx* ctx, int n) {
  std::vector<std::pair<double, int>> key(n);
  for (int s = 0; s < n; ++s) {
    const double* st = ctx->h_state + (size_t)s * 19;
    double k2 = -(st[0] * st[0] + st[1] * st[1] + st[2] * st[2]);
    if (!(k2 == k2)) k2 = 0.0;  // (a NaN prior is the caller's business, not a reason to hand std::sort an unordered key)
    key[s] = {k2, s};
  }
  std::sort(key.begin(), key.end());
  for (int s = 0; s < n; ++s) ctx->h_order[s] = key[s].second;
  ctx->relay_list_parts = 0;  // (the item list of the several-part updates is rebuilt by the next run that needs it)
}

// The number of the next launch of an update kernel.  It tags the entries of the walk cache (16 bits of it: an entry of
// any earlier launch — other clouds, other priors — never matches), so the cache is cleared when those 16 bits come round
// again, not per upload or per step (the per-step clear of lins_streams_step was 33 MB per 1024 streams).
int next_run_gen(lins_ctx* ctx) {
  ++ctx->run_gen;
  if ((ctx->run_gen & 0xFFFF) == 0 && ctx->d_walk_cache) (void)hipMemsetAsync(ctx->d_walk_cache, 0xFF, ctx->slot_cap * 32, ctx->stream);
  return ctx->run_gen;
}

// Several-part updates of a launch of n scans on the batch kernel: the cuts, the launch's number, the list of its
// (scan, part) items on the device — every part 0 in launch order, then every part 1, ... — and the ticket counters and
// flags (RelayArgs; ieskf_lds_impl.h "work items").  `listed`: the launch order of these n scans is on the device.
int relay_prepare(lins_ctx* ctx, int n, bool ordered, RelayArgs& ra) {
  ra.at = ctx->relay_at, ra.cuts = ctx->relay_cuts;
  ra.parts = relay_max_parts(ctx->prm.num_iter, ra.at, ra.cuts);
  if (ctx->relay_gen >= (1 << 26)) {  // (flags are 16 gen + part: start over long before the int runs out)
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_queue, 0, queue_ints(ctx) * sizeof(int), ctx->stream));
    ctx->relay_gen = 0;
  }
  if (ctx->relay_list_parts != ra.parts || ctx->relay_list_n != n) {
    int* list = ctx->h_order + ctx->max_batch;
    for (int p = 0; p < ra.parts; ++p)
      for (int k = 0; k < n; ++k) list[p * n + k] = (ordered ? ctx->h_order[k] : k) | (p << 27);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_order + ctx->max_batch, list, (size_t)ra.parts * n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ctx->relay_list_parts = ra.parts, ctx->relay_list_n = n;
  }
  ra.gen = ++ctx->relay_gen, ra.spins = ctx->relay_spins, ra.cap = ctx->max_batch, ra.slots = ctx->queue_grid;
  ra.hdr = ctx->d_relay_hdr, ra.lane = ctx->d_relay_lane, ra.queue = ctx->d_queue, ra.err = ctx->h_relay_err;
  return LINS_OK;
}

// After a host wait that follows a launch of the batch kernel: did a part of a several-part update give up waiting for its
// hand-over (KernelArgs::relay_err)?  Nothing was written for that scan then — its result buffers hold an earlier launch's
// values — so EVERY call that hands results to the caller after a wait checks here (lins_sync, lins_batch_download, the
// streams steps, the single-call updates), not only lins_sync.  The word is cleared: the error is reported once,
// by the call whose launch it belongs to.
int relay_check(lins_ctx* ctx) {
  if (!ctx->h_relay_err || !*ctx->h_relay_err) return LINS_OK;
  ctx->hip_err = "several-part update: a part's wait for its hand-over ran out (a workgroup of the launch was lost)";
  ctx->queue_timeouts += *ctx->h_relay_err;
  *ctx->h_relay_err = 0;
  (void)hipMemset(ctx->d_queue, 0, queue_ints(ctx) * sizeof(int));  // (counters and flags start over)
  ctx->relay_gen = 0;
  return LINS_E_HIP;
}

}  // namespace lins

extern "C" {

const char* lins_strerror(int code) {
  switch (code) {
    case LINS_OK: return "ok";
    case LINS_E_ARG: return "bad argument";
    case LINS_E_HIP: return "HIP runtime error (see lins_last_hip_error)";
    case LINS_E_CAPACITY: return "batch or cloud exceeds the context capacity";
    case LINS_E_INPUT: return "cloud violates the input contract (non-finite value or ring id out of range)";
    case LINS_E_NODEVICE: return "no usable gfx950 device";
    case LINS_E_STATE: return "call sequence error";
    case LINS_E_UNSUPPORTED: return "input cannot take the requested device path";
    default: return "unknown error";
  }
}

const char* lins_last_hip_error(const lins_ctx* ctx) { return ctx ? ctx->hip_err.c_str() : ""; }

int lins_create(const lins_params* params, int device, int max_batch, int max_targets, lins_ctx** out) {
  if (!params || !out || max_batch < 1 || max_targets < 1) return LINS_E_ARG;
  if (params->num_iter < 1 || params->icp_freq < 1 || !(params->scan_period > 0)) return LINS_E_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0) return LINS_E_NODEVICE;
  lins_ctx* ctx = new (std::nothrow) lins_ctx();
  if (!ctx) return LINS_E_ARG;
  ctx->device = device;
  ctx->prm = *params;
  make_dev_params(*params, SEARCH_AUTO, ctx->dprm);  // (ineligible clouds fall back to the exact exhaustive paths)
  if (const char* g = std::getenv("LINS_ENABLE_DEBUG_KNOBS"))
    if (g[0] == '1') {
      if (const char* e = std::getenv("LINS_LAUNCH_ORDER")) ctx->use_order = e[0] != '0';
      if (const char* e = std::getenv("LINS_COMM_PRIO")) ctx->comm_default_prio = std::atoi(e) == 0;
      if (const char* e = std::getenv("LINS_SPLIT_STREAMS")) ctx->split_mode = std::atoi(e) == 0 ? 0 : (std::atoi(e) >= 2 ? 3 : 1);  // (0: one launch; 1: when runs are queued; 2: always)
      if (std::getenv("LINS_RELAY_AT") || std::getenv("LINS_RELAY_MASK") || std::getenv("LINS_RELAY_CUTS")) ctx->split_mode = 0;  // (the one-launch form's knobs)
      if (const char* e = std::getenv("LINS_RELAY_AT")) ctx->relay_at = std::max(0, std::atoi(e));  // (0: whole updates)
      if (const char* e = std::getenv("LINS_RELAY_CUTS")) ctx->relay_cuts = std::max(1, std::min(14, std::atoi(e)));
      if (const char* e = std::getenv("LINS_RELAY_MASK")) {  // (cuts that are not evenly spaced: bit i = a part ends before iteration i)
        const long m = std::strtol(e, nullptr, 0) & 0x7FFFFFFEl;
        if (m && __builtin_popcountl(m) <= 14) ctx->relay_at = -1, ctx->relay_cuts = (int)m;
      }
      if (const char* e = std::getenv("LINS_RELAY_SPINS")) ctx->relay_spins = std::max(0, std::atoi(e));
      if (const char* e = std::getenv("LINS_QUEUE_GRID")) ctx->queue_grid = std::max(1, std::atoi(e));  // (batches beyond this many scans are cut)
      if (const char* e = std::getenv("LINS_STREAMS_FUSE")) ctx->streams_fuse = e[0] != '0';  // (0: re-projection and index build as two kernels)
      if (const char* e = std::getenv("LINS_RUN_GEN0")) ctx->run_gen = std::atoi(e);  // (test aid: the walk cache's 16-bit wrap on a chosen launch)
    }
  ctx->max_batch = max_batch;
  ctx->max_targets = max_targets;
  ctx->arena_cap = (size_t)max_batch * (2 * align4(max_targets) + 2 * LINS_MAX_QUERY);
  ctx->slot_cap = (size_t)max_batch * LINS_MAX_QUERY;
  if (ctx->arena_cap >= (size_t)1 << 31 || ctx->slot_cap >= (size_t)1 << 31) {  // ScanDesc offsets are 32-bit
    delete ctx;
    return LINS_E_CAPACITY;
  }
#define CREATE_TRY(expr)                             \
  do {                                               \
    hipError_t e__ = (expr);                         \
    if (e__ != hipSuccess) {                         \
      fprintf(stderr, "lins_create: %s: %s\n", #expr, hipGetErrorString(e__)); \
      lins_destroy(ctx);                             \
      return LINS_E_HIP;                             \
    }                                                \
  } while (0)
  CREATE_TRY(hipSetDevice(device));
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) ctx->n_cu = ncu;
  }
  CREATE_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  CREATE_TRY(hipEventCreate(&ctx->ev0));
  CREATE_TRY(hipEventCreate(&ctx->ev1));
  CREATE_TRY(hipEventCreate(&ctx->ev2));
  for (int k = 0; k < lins_ctx::kHist; ++k) {
    CREATE_TRY(hipEventCreate(&ctx->hist0[k]));
    CREATE_TRY(hipEventCreate(&ctx->hist1[k]));
  }
  const size_t nb = (size_t)max_batch;
  CREATE_TRY(hipHostMalloc((void**)&ctx->h_arena, ctx->arena_cap * sizeof(float4)));
  const auto up64 = [](size_t v) { return (v + 63) & ~(size_t)63; };
  const size_t m_cov = up64(nb * 19 * 8), m_out = m_cov + up64(nb * 324 * 8), m_desc = m_out + up64(nb * sizeof(OutRec));
  ctx->meta_out_bytes = m_desc, ctx->meta_in_bytes = m_desc + up64(nb * sizeof(ScanDesc));
  CREATE_TRY(hipHostMalloc((void**)&ctx->h_meta, ctx->meta_in_bytes));
  ctx->h_state = (double*)ctx->h_meta, ctx->h_cov = (double*)(ctx->h_meta + m_cov);
  ctx->h_out = (OutRec*)(ctx->h_meta + m_out), ctx->h_desc = (ScanDesc*)(ctx->h_meta + m_desc);
  CREATE_TRY(hipHostMalloc((void**)&ctx->h_order, 16 * nb * sizeof(int)));  // (n entries: launch order; from max_batch on: parts x n items)
  CREATE_TRY(hipMalloc((void**)&ctx->d_order, 16 * nb * sizeof(int)));
  CREATE_TRY(hipMemsetAsync(ctx->d_order, 0, 16 * nb * sizeof(int), ctx->stream));
  CREATE_TRY(hipMalloc((void**)&ctx->d_arena, ctx->arena_cap * sizeof(float4)));
  CREATE_TRY(hipMalloc((void**)&ctx->d_binned, ctx->arena_cap * sizeof(float4)));
  CREATE_TRY(hipMalloc((void**)&ctx->d_gsorted, ctx->arena_cap * sizeof(float4)));
  CREATE_TRY(hipMalloc((void**)&ctx->d_gridtab, (size_t)ctx->max_batch * sizeof(GridTables)));
  if (ctx->queue_grid <= 0) ctx->queue_grid = lds_mr_resident_workgroups(ctx->n_cu);
  // the carry records of the batch kernel's queries (ieskf_lds_lean.h: tracked candidates and certificates between the
  // iterations of an update; 32 KB per scan): every launch of that kernel uses them, cut into parts or not
  CREATE_TRY(hipMalloc((void**)&ctx->d_relay_lane, (size_t)ctx->max_batch * kRelayLaneInts * sizeof(int)));
  CREATE_TRY(hipMemset(ctx->d_relay_lane, 0xFF, (size_t)ctx->max_batch * kRelayLaneInts * sizeof(int)));  // (empty records)
  if (ctx->max_batch > ctx->queue_grid && lds_mr_has_parts()) {  // (only batches beyond the device's workgroup slots are cut into parts)
    CREATE_TRY(hipMalloc((void**)&ctx->d_relay_hdr, (size_t)ctx->max_batch * 64 * sizeof(double)));
    CREATE_TRY(hipHostMalloc((void**)&ctx->h_relay_err, sizeof(int)));
    *ctx->h_relay_err = 0;
    CREATE_TRY(hipMalloc((void**)&ctx->d_queue, queue_ints(ctx) * sizeof(int)));
    CREATE_TRY(hipMemset(ctx->d_queue, 0, queue_ints(ctx) * sizeof(int)));
  } else {
    ctx->relay_at = 0;
  }
  CREATE_TRY(hipEventCreate(&ctx->ev_idx0));
  CREATE_TRY(hipEventCreate(&ctx->ev_idx1));
  CREATE_TRY(hipMalloc((void**)&ctx->d_meta_in, ctx->meta_in_bytes));
  CREATE_TRY(hipMalloc((void**)&ctx->d_meta_out, ctx->meta_out_bytes));
  ctx->d_state_in = (double*)ctx->d_meta_in, ctx->d_cov_in = (double*)(ctx->d_meta_in + m_cov), ctx->d_desc = (ScanDesc*)(ctx->d_meta_in + m_desc);
  ctx->d_state_out = (double*)ctx->d_meta_out, ctx->d_cov_out = (double*)(ctx->d_meta_out + m_cov), ctx->d_out = (OutRec*)(ctx->d_meta_out + m_out);
  CREATE_TRY(hipMalloc((void**)&ctx->d_lin, nb * 19 * 8));
  CREATE_TRY(hipMalloc((void**)&ctx->d_a6, nb * 21 * 8));
  CREATE_TRY(hipMalloc((void**)&ctx->d_idx, ctx->slot_cap * sizeof(int4)));
  CREATE_TRY(hipMalloc((void**)&ctx->d_walk_cache, ctx->slot_cap * 32));
  CREATE_TRY(hipMemset(ctx->d_walk_cache, 0xFF, ctx->slot_cap * 32));
  CREATE_TRY(hipMalloc((void**)&ctx->d_dump, 2 * LINS_MAX_QUERY * sizeof(lins_corr)));
  CREATE_TRY(hipMalloc((void**)&ctx->d_sums, nb * 28 * 8));
  CREATE_TRY(hipMalloc((void**)&ctx->d_counts, nb * 2 * sizeof(int)));
#undef CREATE_TRY
  *out = ctx;
  return LINS_OK;
}

void lins_destroy(lins_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  (void)hipHostFree(ctx->h_arena);
  (void)hipHostFree(ctx->h_meta);  // (h_state, h_cov, h_out, h_desc)
  (void)hipHostFree(ctx->h_order), (void)hipFree(ctx->d_order);
  (void)hipFree(ctx->d_arena);
  (void)hipFree(ctx->d_binned);
  (void)hipFree(ctx->d_gsorted);
  (void)hipFree(ctx->d_gridtab);
  (void)hipFree(ctx->d_relay_hdr), (void)hipFree(ctx->d_relay_lane), (void)hipFree(ctx->d_queue), (void)hipHostFree(ctx->h_relay_err);
  if (ctx->ev_idx0) (void)hipEventDestroy(ctx->ev_idx0);
  if (ctx->ev_idx1) (void)hipEventDestroy(ctx->ev_idx1);
  (void)hipFree(ctx->d_meta_in), (void)hipFree(ctx->d_meta_out);  // (d_state_in, d_cov_in, d_desc; d_state_out, d_cov_out, d_out)
  (void)hipFree(ctx->d_lin);
  (void)hipFree(ctx->d_a6);
  fe_free(ctx);
  streams_free(ctx);
  if (ctx->map_state && ctx->map_state_free) ctx->map_state_free(ctx->map_state);
  (void)hipFree(ctx->d_idx);
  (void)hipFree(ctx->d_walk_cache);
  (void)hipFree(ctx->d_dump);
  (void)hipFree(ctx->d_sums);
  (void)hipFree(ctx->d_counts);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->ev2) (void)hipEventDestroy(ctx->ev2);
  if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  for (int k = 0; k < lins_ctx::kHist; ++k) {
    if (ctx->hist0b[k]) (void)hipEventDestroy(ctx->hist0b[k]);
    if (ctx->hist1b[k]) (void)hipEventDestroy(ctx->hist1b[k]);
    if (ctx->hist0[k]) (void)hipEventDestroy(ctx->hist0[k]);
    if (ctx->hist1[k]) (void)hipEventDestroy(ctx->hist1[k]);
  }
  pipe_free(ctx);
  rccl_free(ctx);
  if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;  // (with it what was allocated after lins_create: lins_buf.h members, the device still current)
}

int lins_set_search(lins_ctx* ctx, const char* mode) {
  if (!ctx || !mode) return LINS_E_ARG;
  if (!std::strcmp(mode, "brute"))
    ctx->dprm.search = SEARCH_BRUTE;
  else if (!std::strcmp(mode, "binned"))
    ctx->dprm.search = SEARCH_BINNED;
  else if (!std::strcmp(mode, "lds"))  // LDS-resident grid, 1024 threads, 3 lanes per query
    ctx->dprm.search = SEARCH_LDS3;
  else if (!std::strcmp(mode, "lds1"))  // LDS-resident grid, 384 threads, 1 lane per query
    ctx->dprm.search = SEARCH_LDS;
  else if (!std::strcmp(mode, "mr"))  // multi-resident: part of the grid in LDS, 2 scans per CU
    ctx->dprm.search = SEARCH_MR;
  else if (!std::strcmp(mode, "auto"))  // "mr" for batches larger than the CU count, "lds" otherwise
    ctx->dprm.search = SEARCH_AUTO;
  else
    return LINS_E_ARG;
  return LINS_OK;
}

/* The kernel family the last batch (or pass) actually ran: the requested mode after "auto" and the eligibility
 * fall-backs were applied; "" before the first run. */
const char* lins_last_search(const lins_ctx* ctx) {
  if (!ctx) return "";
  switch (ctx->last_search) {
    case SEARCH_BRUTE: return "brute";
    case SEARCH_BINNED: return "binned";
    case SEARCH_LDS: return "lds1";
    case SEARCH_LDS3: return "lds";
    case SEARCH_MR: return "mr";
    default: return "";
  }
}

int lins_batch_upload(lins_ctx* ctx, int n, const lins_scan_pair* in) { return upload(ctx, n, in); }

/* The context's pinned staging arena, laid out for a batch of n scans with the given cloud sizes: clouds[4 s + c] is
 * where cloud c (0 surf_flat, 1 corner_sharp, 2 surf_less_flat_last, 3 corner_less_sharp_last) of scan s belongs, as
 * packed 16-byte points.  A caller that WRITES its clouds there (e.g. its feature extraction's output) and passes those
 * very pointers in the lins_scan_pair array of the next lins_batch_upload / lins_ieskf_update(_batch) call skips the
 * library's copy into the staging arena altogether: the points are validated where they lie and sent.                */
int lins_batch_map(lins_ctx* ctx, int n, const int32_t* counts, lins_point** clouds) {
  if (!ctx || n < 0 || (n && (!counts || !clouds))) return LINS_E_ARG;
  if (n == 0) return LINS_OK;  // (nothing to lay out: the header allows n >= 0)
  {  // (the side streams of the pipelined mode / an earlier asynchronous run may still read the arena's device copy — not
     // the pinned one: every upload waits for its own copies; nothing to join here)
  }
  std::vector<lins_scan_pair> shape((size_t)n);
  lins_point* const some = reinterpret_cast<lins_point*>(ctx->h_arena);  // (layout_batch only checks for null)
  for (int s = 0; s < n; ++s) {
    lins_scan_pair& p = shape[s];
    std::memset(&p, 0, offsetof(lins_scan_pair, state));
    p.n_surf_flat = counts[4 * s], p.n_corner_sharp = counts[4 * s + 1], p.n_surf_last = counts[4 * s + 2], p.n_corner_last = counts[4 * s + 3];
    p.surf_flat = p.corner_sharp = p.surf_less_flat_last = p.corner_less_sharp_last = some;
  }
  size_t off = 0, slots = 0;
  uint64_t bytes = 0;
  int rc = layout_batch(ctx, n, shape.data(), &off, &slots, &bytes);
  if (rc) return rc;
  ctx->n_uploaded = 0, ctx->ran = false;  // (the descriptors of whatever was uploaded are gone)
  for (int s = 0; s < n; ++s) {
    const ScanDesc& d = ctx->h_desc[s];
    const int offs[4] = {d.off_surf_q, d.off_corner_q, d.off_surf_t, d.off_corner_t};
    for (int c = 0; c < 4; ++c) clouds[4 * s + c] = reinterpret_cast<lins_point*>(ctx->h_arena + offs[c]);
  }
  return LINS_OK;
}

int lins_last_cut(const lins_ctx* ctx, int* parts, int* queue_timeouts) {
  if (!ctx || !parts || !queue_timeouts) return LINS_E_ARG;
  if (!ctx->ran) return LINS_E_STATE;
  *parts = ctx->last_parts;
  *queue_timeouts = (int)std::min<long long>(ctx->queue_timeouts, 0x7FFFFFFF);
  return LINS_OK;
}

/* HIP-event time (ms) of the search-index build of the last upload (grid_index_kernel over every scan of the batch:
 * the device counterpart of the reference's kd-tree build, setInputCloud in updatePointCloud, SE:1156-1160); 0 when
 * the batch cannot take the grid kernels (nothing was built).                                                       */
int lins_last_index_ms(lins_ctx* ctx, float* ms) {
  if (!ctx || !ms) return LINS_E_ARG;
  *ms = 0.f;
  if (!ctx->idx_timed) return LINS_E_STATE;
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev_idx1));
  HIP_TRY(ctx, hipEventElapsedTime(ms, ctx->ev_idx0, ctx->ev_idx1));
  return LINS_OK;
}

int lins_batch_run(lins_ctx* ctx, void* d_poses, int32_t scan_id_base) {
  if (!ctx) return LINS_E_ARG;
  if (ctx->n_uploaded <= 0) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  auto& q = ctx->pipe;
  const int set = q.on ? (int)(q.runs & 1u) : 0;
  const bool wait_comm = q.on && q.comm_pending[set];
  if (wait_comm) {  // this run rewrites the pose buffer the gather of run k - 2 read
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, q.ev_comm[set], 0));
    q.comm_pending[set] = false;
  }
  if (q.on) q.run_split[set] = false;
  const int h = (int)(ctx->hist_n % lins_ctx::kHist);
  HIP_TRY(ctx, hipEventRecord(ctx->hist0[h], ctx->stream));
  const RangeFlags& fl = ctx->fl;
  const Family fam = pick_family(ctx, ctx->n_uploaded, fl);
  const bool use_mr = fam.use_mr;
  ctx->last_search = fam.ran;
  // Several-part updates (the kernel's relay + work queue): when the batch has more scans than the device has workgroup
  // slots, a launch of one workgroup per scan ends with slots idle while the last whole updates finish; cut every relay_at
  // iterations the same work is several times as many shorter jobs, pulled from the launch's queue by as many persistent
  // workgroups as are resident at once, and that end shrinks.  Not with the phase profile (one record per scan), and
  // only with ICP_FREQ 1: with a larger one the iterations in between read the triplets an earlier part of the scan left in
  // idx_store — plain stores of another workgroup, possibly on another XCD.
  const bool cut_ok = use_mr && ctx->n_uploaded > ctx->queue_grid && !ctx->d_prof && ctx->prm.icp_freq == 1 && ctx->d_relay_hdr;
  // Two launch queues (lins_ctx::stream2): launches of <= queue_grid scans, whole updates, dealt alternately to the two
  // streams.  Not with the phase profile (one launch) or the pipelined gather mode (its events follow ONE stream);
  // split_mode 0 (lins_set_launch_queues, LINS_SPLIT_STREAMS=0) selects the one-launch form with its several-part updates.
  // ... and in the default mode (2) only when the caller is QUEUING runs — the run before this one is still in flight: a run
  // issued into an idle context is one launch with several-part updates, the shorter of the two forms for a run that is
  // waited for (room batch, 1024 scans x 10 iterations: 0.57 against 0.63 ms; queued back to back: 0.56 against 0.505 ms
  // per run — tools/split_launch_time.py).  Mode 3 (LINS_SPLIT_STREAMS=2) always takes the two queues.
  bool queued = ctx->split_mode >= 3;
  if (!queued && ctx->split_mode && ctx->hist_n > 0 && use_mr && ctx->n_uploaded > ctx->queue_grid) {  // (asked only where the answer matters)
    const int hp = (int)((ctx->hist_n - 1) % lins_ctx::kHist);
    queued = hipEventQuery(ctx->hist1[hp]) == hipErrorNotReady || (ctx->hist_split[hp] && hipEventQuery(ctx->hist1b[hp]) == hipErrorNotReady);
    (void)hipGetLastError();  // (hipErrorNotReady is an answer, not an error to keep)
  }
  const bool split = use_mr && queued && ctx->n_uploaded > ctx->queue_grid && !ctx->d_prof;
  const bool relay = !split && cut_ok && ctx->relay_at != 0 && relay_max_parts(ctx->prm.num_iter, ctx->relay_at, ctx->relay_cuts) > 1;
  RelayArgs ra;
  if (relay) {
    const int rcq = relay_prepare(ctx, ctx->n_uploaded, ctx->use_order, ra);
    if (rcq) return rcq;
  }
  ctx->last_parts = relay ? ra.parts : 1;
  ctx->hist_split[h] = split;
  // (a run that goes out on the context's stream alone after one that used the second queue — lins_set_launch_queues(1) or
  // another kernel family chosen between two queued runs — is ordered behind that queue: same scans, same scratch records)
  if (!split && ctx->split_pending)
    if (int rcs = split_join(ctx)) return rcs;
  if (split) {
    if (int rcq = split_prepare(ctx)) return rcq;
    const int n = ctx->n_uploaded, n_launch = (n + ctx->queue_grid - 1) / ctx->queue_grid, per = (n + n_launch - 1) / n_launch;
    if (ctx->d_walk_cache && (ctx->run_gen & 0xFFFF) + n_launch > 0xFFFF) {
      // the launch numbers of this run would come round in their low 16 bits (the walk cache's tags): next_run_gen's clear on
      // the context's stream would not be ordered against the second queue's launches — the cache is cleared HERE instead,
      // behind both queues and ahead of every launch of the run (the fork below), and the run starts the new round of numbers
      if (int rcs = split_join(ctx)) return rcs;
      HIP_TRY(ctx, hipMemsetAsync(ctx->d_walk_cache, 0xFF, ctx->slot_cap * 32, ctx->stream));
      ctx->run_gen = (ctx->run_gen | 0xFFFF) + 1;
    }
    if (ctx->split_dirty) {  // (uploads, index builds, downloads since the last fork: the second queue starts behind them)
      HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
      HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
      ctx->split_dirty = false;
    }
    if (wait_comm) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, q.ev_comm[set], 0));  // (the second queue writes that pose buffer too)
    HIP_TRY(ctx, hipEventRecord(ctx->hist0b[h], ctx->stream2));
    for (int c = 0; c < n_launch; ++c) {
      const int lo = c * per, cnt = std::min(per, n - lo);
      const int rcr = run_range(ctx, lo, cnt, n, fl, (lins_pose_record*)d_poses, scan_id_base, (c & 1) ? ctx->stream2 : ctx->stream);
      if (rcr) return rcr;
    }
    ctx->last_parts = 1;
    HIP_TRY(ctx, hipEventRecord(ctx->hist1[h], ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->hist1b[h], ctx->stream2));
    ctx->split_pending = true, ctx->split_h = h;
    if (q.on) q.run_split[set] = true, q.h_of[set] = h;  // (pipelined gather mode: the pose records of this run are complete when BOTH queues are through)
  } else {
    ctx->split_dirty = true;  // (a launch on the context's stream the second queue is not ordered behind)
    run_family(ctx, fam, ctx->stream, batch_io(ctx, 0, (lins_pose_record*)d_poses, scan_id_base, ctx->d_prof), ctx->n_uploaded,
               relay ? ctx->d_order + ctx->max_batch : (ctx->use_order ? ctx->d_order : nullptr), relay ? &ra : nullptr);
    HIP_TRY(ctx, hipEventRecord(ctx->hist1[h], ctx->stream));
    if (q.on) q.h_of[set] = h;  // (the pose records of this run are complete at hist1[h])
    // (The Joseph update, SE:594-598, is the update kernel's epilogue since round 3: ieskf_lds_impl.h joseph_epilogue.
    // Rounds 1-2 launched ieskf_joseph_kernel here, ~20 us + a launch per run; a side stream for it — measured at normal
    // and at lowest stream priority — lets its 1024 small workgroups sit on the LDS and wave slots the NEXT run's update
    // kernel needs for its second resident workgroup: that kernel then takes 0.86 instead of 0.71 ms.)
  }
  HIP_TRY(ctx, hipGetLastError());
  ctx->hist_n++;
  if (q.on) q.runs++;
  ctx->ran = true;
  return LINS_OK;
}

/* Pipelined staged mode (off by default).  With it on, lins_pose_allgather() leaves the exchange of a run's pose
 * records on the context's communication stream, so that it travels beside the kernels of the NEXT lins_batch_run().
 * The caller alternates two pose-record buffers (run k -> buffer k & 1) and may enqueue any number of runs before ONE
 * lins_sync(), which waits for everything.  Only the staged calls (upload / run / pose_allgather / sync / download /
 * total_iters / kernel-time queries) may be used while it is on; each of them re-joins the streams where it must.  */
int lins_set_pipelined(lins_ctx* ctx, int on) {
  if (!ctx) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  auto& q = ctx->pipe;
  if (on && !q.s_comm) {
    // A priority of its own (the highest; the second launch queue has the lowest, the context's stream the default): streams of
    // one priority may share a hardware queue, and a gather that waits for BOTH launch queues of run k on the queue that also
    // carries run k + 1's first launch holds that launch back until run k is through — the two launch queues then overlap
    // nothing (forced on one GPU: 18.9 M it/s against 19.5 without the gather, gpurun r06p).  The gather is ~10 us of work.
    int pr_least = 0, pr_greatest = 0;
    HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
    HIP_TRY(ctx, hipStreamCreateWithPriority(&q.s_comm, hipStreamNonBlocking, (ctx->comm_default_prio ? 0 : pr_greatest)));
    for (int k = 0; k < 2; ++k) {
      HIP_TRY(ctx, hipEventCreateWithFlags(&q.ev_comm[k], hipEventDisableTiming));
    }
  }
  int rc = pipe_join(ctx);
  if (rc) return rc;
  q.on = on != 0;
  return LINS_OK;
}

int lins_set_launch_queues(lins_ctx* ctx, int queues) {
  if (!ctx || (queues != 1 && queues != 2)) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = pipe_join(ctx)) return rc;
  ctx->split_mode = queues == 2 ? 1 : 0;
  return LINS_OK;
}

/* GPU time (ms) from the start of the first to the end of the last of the last n lins_batch_run() calls (both launch
 * queues): what n queued runs took on the device, launches overlapping or not.  Waits for the newest of them.        */
int lins_runs_span_ms(lins_ctx* ctx, int n, float* ms) {
  if (!ctx || !ms || n < 1 || n > lins_ctx::kHist || (unsigned)n > ctx->hist_n) return LINS_E_ARG;
  const int h0 = (int)((ctx->hist_n - n) % lins_ctx::kHist);
  float best = 0.f;
  for (int k = 0; k < n; ++k) {  // (ends are not ordered across the two queues: the latest of all)
    const int h = (int)((ctx->hist_n - n + k) % lins_ctx::kHist);
    float t = 0.f;
    HIP_TRY(ctx, hipEventSynchronize(ctx->hist1[h]));
    HIP_TRY(ctx, hipEventElapsedTime(&t, ctx->hist0[h0], ctx->hist1[h]));
    best = std::max(best, t);
    if (ctx->hist_split[h]) {
      HIP_TRY(ctx, hipEventSynchronize(ctx->hist1b[h]));
      HIP_TRY(ctx, hipEventElapsedTime(&t, ctx->hist0[h0], ctx->hist1b[h]));
      best = std::max(best, t);
    }
  }
  *ms = best;
  return LINS_OK;
}

/* per launch of the last n runs: its duration by the events of its own queue (ms; 2 per run with two queues, the second
 * 0 for a one-launch run): out[2 k], out[2 k + 1] */
int lins_launch_ms_history(lins_ctx* ctx, int n, float* ms) {
  if (!ctx || !ms || n < 1 || n > lins_ctx::kHist || (unsigned)n > ctx->hist_n) return LINS_E_ARG;
  for (int k = 0; k < n; ++k) {
    const int h = (int)((ctx->hist_n - n + k) % lins_ctx::kHist);
    HIP_TRY(ctx, hipEventSynchronize(ctx->hist1[h]));
    HIP_TRY(ctx, hipEventElapsedTime(&ms[2 * k], ctx->hist0[h], ctx->hist1[h]));
    ms[2 * k + 1] = 0.f;
    if (ctx->hist_split[h]) {
      HIP_TRY(ctx, hipEventSynchronize(ctx->hist1b[h]));
      HIP_TRY(ctx, hipEventElapsedTime(&ms[2 * k + 1], ctx->hist0b[h], ctx->hist1b[h]));
    }
  }
  return LINS_OK;
}

/* HIP-event times (ms) of the update kernels of the last n lins_batch_run() calls, oldest first (n <= 64 and <= the
 * runs so far); waits for the newest of them.                                                                       */
int lins_kernel_ms_history(lins_ctx* ctx, int n, float* ms) {
  if (!ctx || !ms || n < 0 || n > lins_ctx::kHist || (unsigned)n > ctx->hist_n) return LINS_E_ARG;
  for (int k = 0; k < n; ++k) {
    const int h = (int)((ctx->hist_n - n + k) % lins_ctx::kHist);
    HIP_TRY(ctx, hipEventSynchronize(ctx->hist1[h]));
    HIP_TRY(ctx, hipEventElapsedTime(&ms[k], ctx->hist0[h], ctx->hist1[h]));
    if (ctx->hist_split[h]) {  // (two launch queues: the run = from its first launch's start to its last launch's end)
      float b = 0.f;
      HIP_TRY(ctx, hipEventSynchronize(ctx->hist1b[h]));
      HIP_TRY(ctx, hipEventElapsedTime(&b, ctx->hist0[h], ctx->hist1b[h]));
      ms[k] = std::max(ms[k], b);
    }
  }
  return LINS_OK;
}

int lins_sync(lins_ctx* ctx) {
  if (!ctx) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = pipe_join(ctx);  // (side streams of the pipelined mode: ordered before the wait below)
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return relay_check(ctx);
}

int lins_batch_download(lins_ctx* ctx, int n, lins_result* out) {
  if (!ctx || !out || n < 0) return LINS_E_ARG;
  if (!ctx->ran || n > ctx->n_uploaded) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  {
    int rc = pipe_join(ctx);
    if (rc) return rc;
  }
  if (n == ctx->max_batch) {  // the whole context: posteriors and out records are one block (lins_ctx::h_meta)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_meta, ctx->d_meta_out, ctx->meta_out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_state, ctx->d_state_out, (size_t)n * 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_cov, ctx->d_cov_out, (size_t)n * 324 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, (size_t)n * sizeof(OutRec), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (int rc = relay_check(ctx)) return rc;  // (a scan whose hand-over never arrived holds an earlier launch's values)
  uint64_t tot = 0;
  for (int s = 0; s < n; ++s) {
    lins_result& r = out[s];
    std::memset(&r, 0, sizeof r);
    std::memcpy(r.state, ctx->h_state + (size_t)s * 19, sizeof r.state);
    std::memcpy(r.cov, ctx->h_cov + (size_t)s * 324, sizeof r.cov);
    const OutRec& o = ctx->h_out[s];
    r.residual_norm = o.residual_norm, r.update_norm = o.update_norm;
    r.iters = o.iters, r.converged = o.converged, r.diverged = o.diverged;
    r.m_surf = o.m_surf, r.m_corner = o.m_corner;
    r.reserved[0] = o.pad[0], r.reserved[1] = o.pad[1], r.reserved[2] = o.pad[2];
    tot += (uint64_t)o.iters;
  }
  if (n == ctx->n_uploaded) ctx->total_iters = tot;
  return LINS_OK;
}

int lins_last_kernel_ms(lins_ctx* ctx, float* ms) {
  if (!ctx || !ms) return LINS_E_ARG;
  if (!ctx->ran || ctx->hist_n == 0) return LINS_E_STATE;
  return lins_kernel_ms_history(ctx, 1, ms);
}

int lins_batch_bytes_per_iter(lins_ctx* ctx, uint64_t* bytes) {
  if (!ctx || !bytes) return LINS_E_ARG;
  *bytes = ctx->bytes_per_iter;
  return LINS_OK;
}

int lins_batch_total_iters(lins_ctx* ctx, uint64_t* iters) {
  if (!ctx || !iters) return LINS_E_ARG;
  if (!ctx->ran) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;  // (results of the second launch queue: ordered before what follows)
  int n = ctx->n_uploaded;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, (size_t)n * sizeof(OutRec), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t tot = 0;
  for (int s = 0; s < n; ++s) tot += (uint64_t)ctx->h_out[s].iters;
  *iters = ctx->total_iters = tot;
  return LINS_OK;
}

int lins_ieskf_update_batch(lins_ctx* ctx, int n, const lins_scan_pair* in, lins_result* out) {
  if (!ctx || n < 0 || (n && (!in || !out))) return LINS_E_ARG;
  // Host buffers in and out: the whole call is bounded by validation + packing and PCIe, not by the kernels.  Large
  // batches are therefore PIPELINED: a pool of host threads validates and packs scan after scan into the pinned
  // staging arena; as soon as a chunk of scans is complete, the calling thread sends it (copy stream) and queues its
  // kernels behind the copy (compute stream) while the pool is already packing the next chunks.  (The
  // the phase profile stay on the staged API: lins_batch_upload / _run.)
  int kChunk = 256;  // (measured: 4.6 / 4.2 / 4.1 / 5.7 ms per 1024 scans with chunks of 512 / 256 / 128 / 64)
  bool trace = false;
  if (const char* g = std::getenv("LINS_ENABLE_DEBUG_KNOBS"))
    if (g[0] == '1') {
      if (const char* e = std::getenv("LINS_BATCH_CHUNK")) kChunk = std::max(64, std::atoi(e));
      trace = std::getenv("LINS_BATCH_TRACE") != nullptr;  // stage times on stderr (and two extra syncs)
    }
  const auto t_begin = std::chrono::steady_clock::now();
  auto now_ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
  if (n < 2 * kChunk || ctx->d_prof) {
    const CallTrace tr;
    int rc = upload(ctx, n, in, /*wait*/ false);  // (lins_batch_download below waits for the whole chain)
    if (rc) return rc;
    if (n == 0) return LINS_OK;
    tr.mark("update: uploaded");
    if ((rc = lins_batch_run(ctx, nullptr, 0))) return rc;
    tr.mark("update: run queued");
    rc = lins_batch_download(ctx, n, out);
    tr.mark("update: downloaded");
    return rc;
  }
  size_t arena_used = 0, slots = 0;
  uint64_t bytes = 0;
  int rc = layout_batch(ctx, n, in, &arena_used, &slots, &bytes);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->copy_stream) {
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    BUF_TRY(ctx, ctx->ev_copy.create(hipEventDisableTiming));
  }
  ctx->n_uploaded = 0, ctx->ran = false;
  // the uploads below overwrite the inputs of whatever is still queued on the compute stream (an earlier asynchronous
  // lins_batch_run, the side streams of the pipelined mode): order the copy stream behind it
  if ((rc = pipe_join(ctx))) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev_copy, ctx->stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_copy, 0));

  // (kernel family per CHUNK: a scan that cannot take the grid kernels sends its own chunk of 256, not the whole batch,
  // to the any-size kernel — every family returns the same results, so a scan's bits do not depend on the cut)
  RangeFlags all{true, true, true};
  rc = pack_pipelined(
      n, kChunk, [&](int s) { return pack_one(ctx, in, s); },
      [&](int lo, int hi) -> int {
        if (trace) std::fprintf(stderr, "scans %d..%d packed at %.3f ms\n", lo, hi, now_ms());
        const RangeFlags fl = range_flags(ctx->h_desc + lo, hi - lo);
        const size_t arena_end = hi < n ? (size_t)ctx->h_desc[hi].off_surf_q : arena_used;
        int r = h2d_range(ctx, lo, hi, arena_end, ctx->copy_stream);
        if (r) return r;
        hipError_t e = hipEventRecord(ctx->ev_copy, ctx->copy_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ev_copy, 0);
        if (e == hipSuccess && lo == 0) e = hipEventRecord(ctx->hist0[ctx->hist_n % lins_ctx::kHist], ctx->stream);
        if (e != hipSuccess) return ctx_fail_hip(ctx, e, "chunk hand-over (event record / stream wait)");
        if ((r = build_index_range(ctx, lo, hi - lo, fl))) return r;
        if ((r = run_range(ctx, lo, hi - lo, n, fl, nullptr, 0))) return r;
        all.lds_ok = all.lds_ok && fl.lds_ok, all.mr_ok = all.mr_ok && fl.mr_ok, all.lds3_ok = all.lds3_ok && fl.lds3_ok;
        return 0;
      });
  if (rc) {
    (void)hipStreamSynchronize(ctx->copy_stream), (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  if (trace) {
    std::fprintf(stderr, "all issued at %.3f ms (arena %.1f MB)\n", now_ms(), arena_used * 16e-6);
    (void)hipStreamSynchronize(ctx->copy_stream);
    std::fprintf(stderr, "copies done at %.3f ms\n", now_ms());
    (void)hipStreamSynchronize(ctx->stream);
    std::fprintf(stderr, "kernels done at %.3f ms\n", now_ms());
  }
  // (the history entry of this call spans the whole pipelined region: the kernels of all chunks AND the copy waits
  // between them — lins_last_kernel_ms() after lins_ieskf_update_batch() is an upper bound of the kernel time)
  HIP_TRY(ctx, hipEventRecord(ctx->hist1[ctx->hist_n % lins_ctx::kHist], ctx->stream));
  ctx->hist_split[ctx->hist_n % lins_ctx::kHist] = false;  // (one queue: the slot's second-queue events are another run's)
  ctx->hist_n++;
  // the batch stays resident (inputs, search index): a later lins_batch_run finds its launch order too
  launch_order(ctx, n);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_order, ctx->h_order, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  ctx->idx_timed = false;  // (the index was built chunk by chunk between the copies: no single time to report)
  set_batch_state(ctx, n, all, slots, bytes);
  ctx->ran = true;
  return lins_batch_download(ctx, n, out);
}

/* The ICP / Gauss-Newton fallback of SE:585-592 (estimateTransform, SE:1163-1320) on the device:
 * n scans from the poses in in[].state, out[].state = that state with position and attitude
 * replaced, out[].cov = in[].cov (un-updated), out[].iters / converged = rounds run / stop rule hit.
 * LINS_E_UNSUPPORTED (nothing run) when a scan cannot take the grid kernels (unsorted rings, ring
 * ids >= 16, > 12288 target points): lins_host_perform_ieskf() then falls back to the host
 * Gauss-Newton step over lins_correspondences().                                                */
int lins_icp_update_batch(lins_ctx* ctx, int n, const lins_scan_pair* in, lins_result* out) {
  if (!ctx || n < 0 || (n && (!in || !out))) return LINS_E_ARG;
  int rc = upload(ctx, n, in);
  if (rc) return rc;
  ctx->n_uploaded = 0;  // not an IESKF batch
  if (n == 0) return LINS_OK;
  if (!ctx->fl.mr_ok) return LINS_E_UNSUPPORTED;
  if (ctx->prm.icp_freq != 1) {
    // stored triplets are reused between searches: a scan starts with empty ones, as the oracle does (the
    // reference's arrays keep whatever the previous scan left, SE:206-211), and the deferred corner commit
    // needs every query of a scan in one round of the 512-lane kernel
    for (int s = 0; s < n; ++s)
      if (in[s].n_surf_flat + in[s].n_corner_sharp > 512) return LINS_E_UNSUPPORTED;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_idx, 0xFF, ctx->slot_cap * sizeof(int4), ctx->stream));
  }
  launch_lds_mr_icp(ctx->stream, n, ctx->dprm, ctx->d_desc, ctx->d_arena, ctx->d_gsorted, ctx->d_gridtab, ctx->d_state_in,
                    ctx->d_state_out, ctx->d_out, ctx->d_idx);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_state, ctx->d_state_out, (size_t)n * 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, (size_t)n * sizeof(OutRec), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int s = 0; s < n; ++s) {
    lins_result& r = out[s];
    std::memset(&r, 0, sizeof r);
    std::memcpy(r.state, ctx->h_state + (size_t)s * 19, sizeof r.state);
    std::memcpy(r.cov, in[s].cov, sizeof r.cov);
    const OutRec& o = ctx->h_out[s];
    r.iters = o.iters, r.converged = o.converged, r.m_surf = o.m_surf, r.m_corner = o.m_corner;
  }
  return LINS_OK;
}

int lins_ieskf_update(lins_ctx* ctx, const lins_scan_pair* in, lins_result* out) {
  return lins_ieskf_update_batch(ctx, 1, in, out);
}

static int run_pass(lins_ctx* ctx, const lins_scan_pair* in, const double* lin_state, int iter, bool dump,
                    bool sums) {
  int rc = upload(ctx, 1, in);
  if (rc) return rc;
  ctx->n_uploaded = 0;  // the single-pass calls do not leave a runnable batch behind
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_lin, lin_state, 19 * 8, hipMemcpyHostToDevice, ctx->stream));
  const Family fam = pick_family(ctx, 1, ctx->fl);
  if (fam.use_mr) {
    launch_lds_mr_pass(ctx->stream, 1, ctx->dprm, ctx->d_desc, ctx->d_arena, ctx->d_gsorted, ctx->d_gridtab, ctx->d_lin,
                       ctx->d_state_in, iter, ctx->d_idx, dump ? ctx->d_dump : nullptr, sums ? ctx->d_sums : nullptr,
                       sums ? ctx->d_counts : nullptr);
  } else if (fam.use_lds) {
    launch_lds_pass(ctx->stream, 1, ctx->dprm, fam.search == SEARCH_LDS3 ? 3 : 1, ctx->d_desc, ctx->d_arena, ctx->d_gsorted, ctx->d_gridtab, ctx->d_lin, ctx->d_state_in, iter,
                    ctx->d_idx, dump ? ctx->d_dump : nullptr, sums ? ctx->d_sums : nullptr,
                    sums ? ctx->d_counts : nullptr);
  } else {
    DevParams dp = ctx->dprm;
    dp.search = fam.ran;
    launch_pass(ctx->stream, 1, dp, ctx->d_desc, ctx->d_arena, ctx->d_lin, ctx->d_state_in, iter, ctx->d_idx,
                dump ? ctx->d_dump : nullptr, sums ? ctx->d_sums : nullptr, sums ? ctx->d_counts : nullptr,
                ctx->d_binned);
  }
  HIP_TRY(ctx, hipGetLastError());
  return LINS_OK;
}

int lins_correspondences(lins_ctx* ctx, const lins_scan_pair* in, const double* lin_state, int iter,
                         lins_corr* surf, lins_corr* corner) {
  if (!ctx || !in || !lin_state) return LINS_E_ARG;
  int rc = run_pass(ctx, in, lin_state, iter, true, false);
  if (rc) return rc;
  if (surf && in->n_surf_flat)
    HIP_TRY(ctx, hipMemcpyAsync(surf, ctx->d_dump, sizeof(lins_corr) * in->n_surf_flat, hipMemcpyDeviceToHost, ctx->stream));
  if (corner && in->n_corner_sharp)
    HIP_TRY(ctx, hipMemcpyAsync(corner, ctx->d_dump + in->n_surf_flat, sizeof(lins_corr) * in->n_corner_sharp,
                                hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LINS_OK;
}

int lins_reduce_pass(lins_ctx* ctx, const lins_scan_pair* in, const double* lin_state, int iter, double* sums28,
                     int32_t* m_surf, int32_t* m_corner) {
  if (!ctx || !in || !lin_state || !sums28) return LINS_E_ARG;
  int rc = run_pass(ctx, in, lin_state, iter, false, true);
  if (rc) return rc;
  int counts[2];
  HIP_TRY(ctx, hipMemcpyAsync(sums28, ctx->d_sums, 28 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->d_counts, sizeof counts, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (m_surf) *m_surf = counts[0];
  if (m_corner) *m_corner = counts[1];
  return LINS_OK;
}

}  // extern "C"
