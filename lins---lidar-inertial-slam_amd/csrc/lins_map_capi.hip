// lins_map_capi.hip — C ABI of the scan-to-map row (include/lins_map.h): host orchestration around
// map_kernels.hip.  Per problem the two map clouds are bucketed into 1 m cells once (host counting sort,
// threaded over problems); each round the host forms the trigonometry of the current transform (libm, as the
// reference does, LM:579-592 / 1524-1529), the device evaluates every query (5-NN, fits, rows, 28 sums),
// and the host takes the 6-DoF Gauss-Newton step of LMOptimization in f32 (QR solve, degeneracy projection
// of round 0, stop rule) — 6x6 scalar algebra per problem.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/lins_map.h"
#include "lins_ctx_priv.h"
#include "lins_launch.h"
#include "local_map.h"
#include "lm_math.h"
#include "map_math.h"

using namespace lins;

namespace {

struct MapState {
  DevBuf<float4> d_raw, d_pts;
  PinBuf<float4> h_q;  // pinned staging of the queries of one call (one copy instead of two per problem)
  DevBuf<int> d_cells;
  DevBuf<double> d_partials;
  // one capacity (queries): grown together, d_q answers
  DevBuf<float4> d_q;
  DevBuf<lins_map_corr> d_rec;
  // one capacity (problems): grown together, d_probs answers
  DevBuf<MapDev> d_probs;
  DevBuf<MapRoundParams> d_rounds;
  DevBuf<MapGridJob> d_jobs;  // two per problem
  DevBuf<LmCarry> d_carry;
  DevBuf<lins_map_result> d_results;
  // the maps resident on the device (gridded): sizes per problem of the last upload, for LINS_MAP_REUSE
  std::vector<int> resident_sizes;
  std::vector<MapDev> resident_dev;
  float ms = 0.f;
  uint64_t queries = 0;
  bool selfcheck_done = false;
  int max_rounds = 10;  // lins_debug_map_rounds (test aid): the rounds lins_scan2map_batch runs at most
  // what the other mapping files keep per context (local_map.h MapSlot), freed with this state in the enum's order
  void* slot[kSlotCount] = {};
  void (*slot_free[kSlotCount])(void*) = {};

  int grow_problems(size_t n) { return grow_all(d_probs, n, d_rounds, n, d_jobs, 2 * n, d_carry, n, d_results, n); }
  int grow_queries(size_t n) { return grow_all(d_q, n, d_rec, n); }
};

void map_state_free(void* p) {
  MapState* m = (MapState*)p;
  for (int i = 0; i < kSlotCount; ++i)
    if (m->slot[i]) m->slot_free[i](m->slot[i]);
  delete m;
}

template <class F>
int parallel_for(int n, F fn) {
  const unsigned hw = std::thread::hardware_concurrency();
  const int T = std::max(1, std::min({16, (int)(hw ? hw : 1), n}));
  std::vector<int> rc(n, 0);
  std::atomic<int> next{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < T; ++t)
    pool.emplace_back([&] {
      for (int k; (k = next.fetch_add(1)) < n;) rc[k] = fn(k);
    });
  for (auto& th : pool) th.join();
  for (int k = 0; k < n; ++k)
    if (rc[k]) return rc[k];
  return 0;
}

// input contract of a map cloud + its bounding box in 1 m cells (the counting sort itself runs on the device)
int cloud_box(const lins_point* p, int n, int* cmin, int* cdim, long long* ncell) {
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i) {
    if (!std::isfinite(p[i].x) || !std::isfinite(p[i].y) || !std::isfinite(p[i].z)) return LINS_E_INPUT;
    if (std::fabs(p[i].x) > 1e6f || std::fabs(p[i].y) > 1e6f || std::fabs(p[i].z) > 1e6f) return LINS_E_INPUT;
    const int c[3] = {(int)std::floor(p[i].x), (int)std::floor(p[i].y), (int)std::floor(p[i].z)};
    for (int a = 0; a < 3; ++a) lo[a] = i ? std::min(lo[a], c[a]) : c[a], hi[a] = i ? std::max(hi[a], c[a]) : c[a];
  }
  *ncell = 1;
  for (int a = 0; a < 3; ++a) cmin[a] = lo[a], cdim[a] = hi[a] - lo[a] + 1, *ncell *= cdim[a];
  if (*ncell > (1ll << 26)) return LINS_E_CAPACITY;  // a map far larger than a local one (LM keeps ~50 key frames)
  return LINS_OK;
}

// Brings n problems onto the device: queries always; the maps (raw upload + device gridding) unless every problem
// carries LINS_MAP_REUSE and the resident maps have the same sizes — the local map of the mapping node only changes
// with its key frames.  Fills the device descriptors; active[k] = precondition of LM:1636.
int map_upload(lins_ctx* ctx, MapState* m, int n, const lins_map_problem* in, std::vector<MapDev>& dev, int* max_q) {
  bool reuse = (int)m->resident_dev.size() == n && n > 0;
  for (int k = 0; k < n; ++k) {
    const lins_map_problem& p = in[k];
    if (p.n_map_corner < 0 || p.n_map_surf < 0 || p.n_scan_corner < 0 || p.n_scan_surf < 0) return LINS_E_ARG;
    if ((p.n_map_corner && !p.map_corner) || (p.n_map_surf && !p.map_surf) || (p.n_scan_corner && !p.scan_corner) ||
        (p.n_scan_surf && !p.scan_surf))
      return LINS_E_ARG;
    if (!(p.reserved[0] & LINS_MAP_REUSE) || !reuse || m->resident_sizes[2 * k] != p.n_map_corner ||
        m->resident_sizes[2 * k + 1] != p.n_map_surf)
      reuse = false;
  }
  hipStream_t st = ctx_stream(ctx);
  int rc;
  if (!reuse) {
    m->resident_dev.clear(), m->resident_sizes.clear();
    std::vector<MapGridJob> jobs((size_t)n * 2);
    rc = parallel_for(2 * n, [&](int j) {
      const lins_map_problem& p = in[j / 2];
      MapGridJob& jb = jobs[j];
      jb.n = (j & 1) ? p.n_map_surf : p.n_map_corner;
      long long ncell = 1;
      const int r = cloud_box((j & 1) ? p.map_surf : p.map_corner, jb.n, jb.cmin, jb.cdim, &ncell);
      jb.ncell = (int)ncell;
      return r;
    });
    if (rc) return rc;
    size_t tot_pts = 0, tot_cells = 0;
    dev.assign(n, MapDev{});
    for (int k = 0; k < n; ++k)
      for (int w = 0; w < 2; ++w) {
        MapGridJob& jb = jobs[(size_t)k * 2 + w];
        jb.off_raw = jb.off_pts = (long long)tot_pts, jb.off_cells = (long long)tot_cells;
        dev[k].g[w].off_pts = jb.off_pts, dev[k].g[w].off_cells = jb.off_cells;
        for (int a = 0; a < 3; ++a) dev[k].g[w].cmin[a] = jb.cmin[a], dev[k].g[w].cdim[a] = jb.cdim[a];
        tot_pts += (size_t)jb.n, tot_cells += 2 * ((size_t)jb.ncell + 1);  // starts + scratch cursors
      }
    BUF_TRY(ctx, m->d_raw.grow(tot_pts));
    BUF_TRY(ctx, m->d_pts.grow(tot_pts));
    BUF_TRY(ctx, m->d_cells.grow(tot_cells));
    BUF_TRY(ctx, m->grow_problems((size_t)n));
    for (int k = 0; k < n; ++k) {
      if (in[k].n_map_corner)
        HIP_TRY(ctx, hipMemcpyAsync(m->d_raw + jobs[(size_t)k * 2].off_raw, in[k].map_corner, (size_t)in[k].n_map_corner * sizeof(float4), hipMemcpyHostToDevice, st));
      if (in[k].n_map_surf)
        HIP_TRY(ctx, hipMemcpyAsync(m->d_raw + jobs[(size_t)k * 2 + 1].off_raw, in[k].map_surf, (size_t)in[k].n_map_surf * sizeof(float4), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(ctx, hipMemcpyAsync(m->d_jobs, jobs.data(), jobs.size() * sizeof(MapGridJob), hipMemcpyHostToDevice, st));
    launch_map_grid(st, 2 * n, m->d_jobs, m->d_raw, m->d_pts, m->d_cells);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));  // (jobs goes out of scope)
    for (int k = 0; k < n; ++k) m->resident_sizes.push_back(in[k].n_map_corner), m->resident_sizes.push_back(in[k].n_map_surf);
  } else {
    dev = m->resident_dev;
  }
  size_t tot_q = 0;
  *max_q = 0;
  for (int k = 0; k < n; ++k) {
    dev[k].off_q = dev[k].off_rec = (long long)tot_q;
    dev[k].n_q[0] = in[k].n_scan_corner, dev[k].n_q[1] = in[k].n_scan_surf;
    dev[k].active = in[k].n_map_corner > 10 && in[k].n_map_surf > 100;  // LM:1636
    tot_q += (size_t)dev[k].n_q[0] + dev[k].n_q[1];
    *max_q = std::max(*max_q, dev[k].n_q[0] + dev[k].n_q[1]);
  }
  BUF_TRY(ctx, m->h_q.grow(tot_q));
  rc = parallel_for(n, [&](int k) {  // input contract + packing into the pinned staging buffer
    float4* dst = m->h_q + dev[k].off_q;
    for (int i = 0; i < in[k].n_scan_corner + in[k].n_scan_surf; ++i) {
      const lins_point& q = i < in[k].n_scan_corner ? in[k].scan_corner[i] : in[k].scan_surf[i - in[k].n_scan_corner];
      if (!std::isfinite(q.x) || !std::isfinite(q.y) || !std::isfinite(q.z)) return (int)LINS_E_INPUT;
      dst[i] = make_float4(q.x, q.y, q.z, q.intensity);
    }
    return (int)LINS_OK;
  });
  if (rc) return rc;
  BUF_TRY(ctx, m->grow_queries(tot_q));
  if (tot_q) HIP_TRY(ctx, hipMemcpyAsync(m->d_q, m->h_q, tot_q * sizeof(float4), hipMemcpyHostToDevice, st));
  m->resident_dev = dev;
  return LINS_OK;
}

// LINS_MAP_LOCAL: the maps and queries are the clouds of the last local-map build, read where they lie — the maps are
// gridded from the build's cloud arena (its 1 m boxes came back with the build), the queries are its cornerDS with
// surfTotalDS right behind (lins_local_map_capi.hip lays them out so).  No host cloud is read or uploaded.
int map_upload_local(lins_ctx* ctx, MapState* m, const LocalMapView& lv, std::vector<MapDev>& dev, int* max_q) {
  const int n = lv.n;
  std::vector<MapGridJob> jobs((size_t)n * 2);
  size_t tot_pts = 0, tot_cells = 0, tot_q = 0;
  dev.assign(n, MapDev{});
  *max_q = 0;
  for (int k = 0; k < n; ++k) {
    const lins_local_map_sizes& z = lv.sizes[k];
    for (int w = 0; w < 2; ++w) {
      MapGridJob& jb = jobs[(size_t)k * 2 + w];
      long long ncell = 1;
      for (int a = 0; a < 3; ++a) jb.cmin[a] = z.box_min[w][a], jb.cdim[a] = z.box_dim[w][a], ncell *= jb.cdim[a];
      if (ncell > (1ll << 26)) return LINS_E_CAPACITY;  // (cloud_box's limit)
      jb.n = z.n[w], jb.ncell = (int)ncell;
      jb.off_raw = lv.off[6 * k + w], jb.off_pts = (long long)tot_pts, jb.off_cells = (long long)tot_cells;
      dev[k].g[w].off_pts = jb.off_pts, dev[k].g[w].off_cells = jb.off_cells;
      for (int a = 0; a < 3; ++a) dev[k].g[w].cmin[a] = jb.cmin[a], dev[k].g[w].cdim[a] = jb.cdim[a];
      tot_pts += (size_t)jb.n, tot_cells += 2 * ((size_t)jb.ncell + 1);
    }
    dev[k].off_q = lv.off[6 * k + LINS_LOCAL_SCAN_CORNER], dev[k].off_rec = (long long)tot_q;
    dev[k].n_q[0] = z.n[LINS_LOCAL_SCAN_CORNER], dev[k].n_q[1] = z.n[LINS_LOCAL_SCAN_TOTAL];
    dev[k].active = z.n[0] > 10 && z.n[1] > 100;  // LM:1636
    tot_q += (size_t)dev[k].n_q[0] + dev[k].n_q[1];
    *max_q = std::max(*max_q, dev[k].n_q[0] + dev[k].n_q[1]);
  }
  BUF_TRY(ctx, m->d_pts.grow(tot_pts));
  BUF_TRY(ctx, m->d_cells.grow(tot_cells));
  BUF_TRY(ctx, m->grow_problems((size_t)n));
  BUF_TRY(ctx, m->grow_queries(tot_q));
  hipStream_t st = ctx_stream(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(m->d_jobs, jobs.data(), jobs.size() * sizeof(MapGridJob), hipMemcpyHostToDevice, st));
  launch_map_grid(st, 2 * n, m->d_jobs, lv.d_out, m->d_pts, m->d_cells);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(st));  // (jobs goes out of scope)
  // the gridded maps are resident as after an explicit upload: a later LINS_MAP_REUSE call may use them
  m->resident_sizes.clear();
  for (int k = 0; k < n; ++k) m->resident_sizes.push_back(lv.sizes[k].n[0]), m->resident_sizes.push_back(lv.sizes[k].n[1]);
  m->resident_dev = dev;
  return LINS_OK;
}

bool transform_finite(const float* t) {
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(t[i])) return false;
  return true;
}

MapState* state_of(lins_ctx* ctx) {
  void** slot = ctx_map_slot(ctx, map_state_free);
  if (!*slot) *slot = new MapState();
  return (MapState*)*slot;
}

// once per context: the device plane fit on a known wall (see map_selfcheck_kernel)
int map_selfcheck(lins_ctx* ctx, MapState* m) {
  if (m->selfcheck_done) return LINS_OK;
  DevBuf<float> d;
  float h[5] = {0, 0, 0, 0, 0};
  BUF_TRY(ctx, d.grow(5));
  launch_map_selfcheck(ctx_stream(ctx), d);
  hipError_t e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, ctx_stream(ctx));
  if (e == hipSuccess) e = hipStreamSynchronize(ctx_stream(ctx));
  if (e != hipSuccess) return ctx_fail_hip(ctx, e, "map self-check");
  // normal (0, -1, 0) scaled by the weight s ~ 0.97, signed distance -0.05 scaled likewise, accepted
  const bool ok = h[4] == 1.f && std::fabs(h[0]) < 1e-3f && std::fabs(h[2]) < 1e-3f && h[1] < -0.9f && std::fabs(h[3] + 0.0485f) < 2e-3f;
  if (!ok) return ctx_fail_hip(ctx, hipErrorUnknown, "scan-to-map plane fit self-check failed: the 5x3 QR is miscompiled (toolchain / flags changed?)");
  m->selfcheck_done = true;
  return LINS_OK;
}

}  // namespace

namespace lins {
void** map_slot(lins_ctx* ctx, MapSlot which, void (*free_fn)(void*)) {
  MapState* m = state_of(ctx);
  m->slot_free[which] = free_fn;
  return &m->slot[which];
}

// lins_scan2map_batch with LINS_MAP_LOCAL for the step of lins_streams_map_capi.hip: the same gridding, the same rounds,
// but the start transforms are not uploaded — map_associate_kernel forms them on the device from the resident poses and
// writes them where the first launch_map_lm reads them — and map_pose_finish_kernel runs behind the last round, so that
// what comes down is one lins_map_step_result per entry.  d_entries is already on its way on the context's stream.
// d_odom (or null): the two pose kernels read transformSum from the resident record of the entry's stream.
int scan2map_local_resident(lins_ctx* ctx, int n, const MapPoseEntry* d_entries, MapPoseRec* d_poses, lins_map_step_result* d_out,
                            lins_map_step_result* h_out, hipEvent_t* ev, const lins_stream_odom* d_odom) {
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  MapState* m = state_of(ctx);
  int rc = map_selfcheck(ctx, m);
  if (rc) return rc;
  LocalMapView lv{};
  if (local_map_view(ctx, &lv) || lv.n != n) return LINS_E_STATE;
  std::vector<MapDev> dev;
  int max_q = 0;
  if ((rc = map_upload_local(ctx, m, lv, dev, &max_q))) {
    m->resident_dev.clear(), m->resident_sizes.clear();
    return rc;
  }
  for (int k = 0; k < n; ++k) dev[k].pad = lv.sizes[k].status ? lv.sizes[k].status : dev[k].active;  // (for the two pose kernels)
  const int bpp = std::max(1, (max_q + map_block() - 1) / map_block());
  BUF_TRY(ctx, m->d_partials.grow((size_t)n * bpp * 28));
  hipStream_t st = ctx_stream(ctx);
  hipEvent_t e0, e1;
  ctx_events(ctx, &e0, &e1);
  HIP_TRY(ctx, hipMemcpyAsync(m->d_probs, dev.data(), (size_t)n * sizeof(MapDev), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipEventRecord(ev[0], st));
  launch_map_associate(st, n, d_entries, m->d_probs, d_poses, m->d_results, d_out, d_odom);
  HIP_TRY(ctx, hipEventRecord(ev[1], st));
  HIP_TRY(ctx, hipEventRecord(e0, st));
  launch_map_lm(st, n, -1, bpp, m->d_probs, m->d_rounds, m->d_partials, m->d_results, m->d_carry);
  for (int iter = 0; iter < m->max_rounds; ++iter) {
    launch_map_corr(st, n, bpp, m->d_probs, m->d_rounds, m->d_pts, m->d_cells, lv.d_out, m->d_rec, m->d_partials);
    launch_map_lm(st, n, iter, bpp, m->d_probs, m->d_rounds, m->d_partials, m->d_results, m->d_carry);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(e1, st));
  HIP_TRY(ctx, hipEventRecord(ev[2], st));
  launch_map_pose_finish(st, n, d_entries, m->d_probs, d_poses, m->d_results, d_out, d_odom);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ev[3], st));
  HIP_TRY(ctx, hipMemcpyAsync(h_out, d_out, (size_t)n * sizeof(lins_map_step_result), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipEventElapsedTime(&m->ms, e0, e1));
  m->queries = 0;
  for (int k = 0; k < n; ++k) m->queries += (uint64_t)h_out[k].iters * ((uint64_t)dev[k].n_q[0] + dev[k].n_q[1]);
  return LINS_OK;
}
}  // namespace lins

extern "C" {

int lins_scan2map_batch(lins_ctx* ctx, int n, const lins_map_problem* in, lins_map_result* out) {
  if (!ctx || n < 0 || (n && (!in || !out))) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  static_assert(sizeof(MapRoundParams) == 64 && sizeof(lins_map_corr) == 56, "layouts");
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  MapState* m = state_of(ctx);
  int rc = map_selfcheck(ctx, m);
  if (rc) return rc;
  int n_local = 0;
  for (int k = 0; k < n; ++k) {
    const int fl = in[k].reserved[0];
    if ((fl & LINS_MAP_LOCAL) && (fl & LINS_MAP_REUSE)) return LINS_E_ARG;
    n_local += (fl & LINS_MAP_LOCAL) != 0;
  }
  if (n_local && n_local != n) return LINS_E_ARG;  // a batch is local or explicit, not both
  for (int k = 0; k < n; ++k)
    if (!transform_finite(in[k].transform)) {  // (input contract, lins_map.h: like every LINS_E_INPUT, nothing stays resident)
      m->resident_dev.clear(), m->resident_sizes.clear();
      return LINS_E_INPUT;
    }
  LocalMapView lv{};
  if (n_local && (local_map_view(ctx, &lv) || lv.n != n)) return LINS_E_STATE;
  std::vector<MapDev> dev;
  int max_q = 0;
  rc = n_local ? map_upload_local(ctx, m, lv, dev, &max_q) : map_upload(ctx, m, n, in, dev, &max_q);
  if (rc) {
    m->resident_dev.clear(), m->resident_sizes.clear();
    return rc;
  }
  const float4* d_q = n_local ? lv.d_out : m->d_q;
  const int bpp = std::max(1, (max_q + map_block() - 1) / map_block());
  BUF_TRY(ctx, m->d_partials.grow((size_t)n * bpp * 28));
  hipStream_t st = ctx_stream(ctx);
  hipEvent_t e0, e1;
  ctx_events(ctx, &e0, &e1);
  for (int k = 0; k < n; ++k) {
    std::memcpy(out[k].transform, in[k].transform, sizeof out[k].transform);
    out[k].iters = 0, out[k].converged = 0, out[k].degenerate = 0, out[k].n_sel = 0;
  }
  // the ten rounds of scan2MapOptimization (LM:1640-1647) back to back on the device: correspondences + rows + sums,
  // then the 6x6 step, which also writes the next round's rotation terms and retires converged problems
  HIP_TRY(ctx, hipMemcpyAsync(m->d_probs, dev.data(), (size_t)n * sizeof(MapDev), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(m->d_results, out, (size_t)n * sizeof(lins_map_result), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipEventRecord(e0, st));
  launch_map_lm(st, n, -1, bpp, m->d_probs, m->d_rounds, m->d_partials, m->d_results, m->d_carry);
  for (int iter = 0; iter < m->max_rounds; ++iter) {
    launch_map_corr(st, n, bpp, m->d_probs, m->d_rounds, m->d_pts, m->d_cells, d_q, m->d_rec, m->d_partials);
    launch_map_lm(st, n, iter, bpp, m->d_probs, m->d_rounds, m->d_partials, m->d_results, m->d_carry);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(e1, st));
  HIP_TRY(ctx, hipMemcpyAsync(out, m->d_results, (size_t)n * sizeof(lins_map_result), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipEventElapsedTime(&m->ms, e0, e1));
  m->queries = 0;
  for (int k = 0; k < n; ++k) m->queries += (uint64_t)out[k].iters * ((uint64_t)dev[k].n_q[0] + dev[k].n_q[1]);
  return LINS_OK;
}

int lins_map_correspondences(lins_ctx* ctx, const lins_map_problem* in, lins_map_corr* corner, lins_map_corr* surf) {
  if (!ctx || !in || (in->n_scan_corner && !corner) || (in->n_scan_surf && !surf)) return LINS_E_ARG;
  if (in->reserved[0] & LINS_MAP_LOCAL) return LINS_E_ARG;  // (explicit clouds only)
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  MapState* m = state_of(ctx);
  int rc = map_selfcheck(ctx, m);
  if (rc) return rc;
  std::vector<MapDev> dev;
  int max_q = 0;
  rc = transform_finite(in->transform) ? map_upload(ctx, m, 1, in, dev, &max_q) : (int)LINS_E_INPUT;
  if (rc) {
    m->resident_dev.clear(), m->resident_sizes.clear();
    return rc;
  }
  dev[0].active = 1;  // a single pass is evaluated whatever the map sizes
  const int bpp = std::max(1, (max_q + map_block() - 1) / map_block());
  BUF_TRY(ctx, m->d_partials.grow((size_t)bpp * 28));
  hipStream_t st = ctx_stream(ctx);
  const MapRoundParams rd = lm_make_round(in->transform);
  HIP_TRY(ctx, hipMemcpyAsync(m->d_probs, dev.data(), sizeof(MapDev), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(m->d_rounds, &rd, sizeof rd, hipMemcpyHostToDevice, st));
  launch_map_corr(st, 1, bpp, m->d_probs, m->d_rounds, m->d_pts, m->d_cells, m->d_q, m->d_rec, m->d_partials);
  HIP_TRY(ctx, hipGetLastError());
  if (in->n_scan_corner)
    HIP_TRY(ctx, hipMemcpyAsync(corner, m->d_rec, (size_t)in->n_scan_corner * sizeof(lins_map_corr), hipMemcpyDeviceToHost, st));
  if (in->n_scan_surf)
    HIP_TRY(ctx, hipMemcpyAsync(surf, m->d_rec + in->n_scan_corner, (size_t)in->n_scan_surf * sizeof(lins_map_corr), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return LINS_OK;
}

/* Debug aid (not part of the drop-in surface; tests/test_gpu_map_rounds.py): lins_scan2map_batch of this context stops
 * after `rounds` rounds (0 .. 10; 10 is the behaviour without the call) — results are those of the last round run, so
 * that every round of the device's own loop can be held against the oracle's trace.  Declared by its users. */
int lins_debug_map_rounds(lins_ctx* ctx, int rounds) {
  if (!ctx || rounds < 0 || rounds > 10) return LINS_E_ARG;
  state_of(ctx)->max_rounds = rounds;
  return LINS_OK;
}

int lins_last_map_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* queries) {
  if (!ctx) return LINS_E_ARG;
  MapState* m = state_of(ctx);
  if (kernel_ms) *kernel_ms = m->ms;
  if (queries) *queries = m->queries;
  return LINS_OK;
}

}  // extern "C"
