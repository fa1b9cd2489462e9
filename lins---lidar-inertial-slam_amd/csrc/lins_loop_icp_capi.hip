// lins_loop_icp_capi.hip — C ABI of the loop-closure ICP (include/lins_map.h lins_loop_icp_*): host orchestration
// around loop_icp_kernels.hip.  The clouds are entries of the last archive assembly, read where they lie, or host
// clouds, uploaded; every target is gridded once into 1 m cells (map_grid_kernel); the rounds are queued in groups —
// search + sums kernel, step kernel, no host arithmetic — with one word "problems still running" read between groups;
// one more search without the cap gives the fitness score.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lins_map.h"
#include "../../include/lins_place.h"
#include "keyframe_archive.h"
#include "lins_ctx_priv.h"
#include "lins_launch.h"
#include "local_map.h"
#include "loop_icp.h"

using namespace lins;
using lins_licp::kSums;
using lins_licp::State;

namespace {

// Rounds queued between two reads of the "still running" word.  A round is two launches (~10 us of launch latency a
// pair); a read is one synchronisation (~30 us with the copy).  Loop closures converge in 10-30 rounds of the 100 the
// reference allows, so one group of 100 would queue 70-90 empty rounds.  8 is a reasoned default, not yet a measured
// one: tools/loop_icp_rate.py sweeps it (lins_debug_loop_icp_group).
constexpr int kLoopGroup = 8;

struct LoopMem {
  DevBuf<float4> d_src, d_raw, d_pts;
  PinBuf<float4> h_up;  // pinned staging of the host clouds of one call
  DevBuf<int> d_cells;
  DevBuf<LoopDev> d_probs;
  DevBuf<State> d_states;
  DevBuf<MapGridJob> d_jobs;
  DevBuf<double> d_partials;
  DevBuf<int> d_running;
  PinBuf<int> h_running;
  DevBuf<int32_t> d_idx;
  DevBuf<float> d_d;
  int max_rounds = 0;  // lins_debug_loop_icp_rounds (0: off)
  int shells = kLoopShells;
  int group = kLoopGroup;
  float ms = 0.f;
  uint64_t searches = 0;
  unsigned last_far = 0;
};

void loop_free(void* p) { delete (LoopMem*)p; }

LoopMem* mem_of(lins_ctx* ctx) {
  void** slot = map_slot(ctx, kSlotLoop, loop_free);
  if (!*slot) *slot = new LoopMem();
  return (LoopMem*)*slot;
}

bool cloud_finite(const lins_point* p, int n) {
  for (int i = 0; i < n; ++i) {
    if (!std::isfinite(p[i].x) || !std::isfinite(p[i].y) || !std::isfinite(p[i].z)) return false;
    if (std::fabs(p[i].x) > 1e6f || std::fabs(p[i].y) > 1e6f || std::fabs(p[i].z) > 1e6f) return false;
  }
  return true;
}

// the 1 m cell box of a cloud of the input contract (empty: min 0, dim 1)
void box_of(const lins_point* p, int n, int* cmin, int* cdim) {
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const int c[3] = {(int)std::floor(p[i].x), (int)std::floor(p[i].y), (int)std::floor(p[i].z)};
    for (int a = 0; a < 3; ++a) lo[a] = i ? std::min(lo[a], c[a]) : c[a], hi[a] = i ? std::max(hi[a], c[a]) : c[a];
  }
  for (int a = 0; a < 3; ++a) cmin[a] = lo[a], cdim[a] = hi[a] - lo[a] + 1;
}

struct Prepared {
  std::vector<LoopDev> dev;
  int bpp = 1;
};

// Validates n problems, uploads their host clouds, grids every target; fills the device descriptors (on the device
// too).  status[k] != 0: problem k is not run.
int prepare(lins_ctx* ctx, LoopMem* m, int n, const lins_loop_icp_problem* in, Prepared& P) {
  ArchiveView av{};
  bool have_view = false;
  size_t up_src = 0, up_tgt = 0;
  for (int k = 0; k < n; ++k) {
    const lins_loop_icp_problem& p = in[k];
    const int e[2] = {p.source_entry, p.target_entry};
    for (int w = 0; w < 2; ++w) {
      if (e[w] < -1) return LINS_E_ARG;
      if (e[w] >= 0) {
        if (!have_view) {
          if (int rc = archive_view(ctx, &av)) return rc;  // LINS_E_STATE: no assembly
          have_view = true;
        }
        if (e[w] >= av.n) return LINS_E_ARG;
      }
    }
    if (e[0] < 0) {
      if (p.n_source < 0 || (p.n_source && !p.source)) return LINS_E_ARG;
      up_src += (size_t)p.n_source;
    }
    if (e[1] < 0) {
      if (p.n_target < 0 || (p.n_target && !p.target)) return LINS_E_ARG;
      up_tgt += (size_t)p.n_target;
    }
  }
  for (int k = 0; k < n; ++k) {
    if (in[k].source_entry < 0 && !cloud_finite(in[k].source, in[k].n_source)) return LINS_E_INPUT;
    if (in[k].target_entry < 0 && !cloud_finite(in[k].target, in[k].n_target)) return LINS_E_INPUT;
  }
  hipStream_t st = ctx_stream(ctx);
  BUF_TRY(ctx, m->d_src.grow(up_src));
  BUF_TRY(ctx, m->d_raw.grow(up_tgt));
  BUF_TRY(ctx, m->h_up.grow(up_src + up_tgt));
  // descriptors and grid jobs: the host targets' jobs first (raw = the upload arena), then the entries' (raw = the
  // archive's cloud arena) — map_grid_kernel takes one raw arena a launch
  P.dev.assign(n, LoopDev{});
  std::vector<MapGridJob> jobs_host, jobs_entry;
  std::vector<lins_point> tmp;
  size_t at_src = 0, at_tgt = 0, tot_pts = 0, tot_cells = 0;
  int max_src = 0;
  for (int k = 0; k < n; ++k) {
    const lins_loop_icp_problem& p = in[k];
    LoopDev& d = P.dev[k];
    MapGridJob jb{};
    if (p.source_entry >= 0) {
      d.src = av.d_out + av.off[p.source_entry], d.n_src = av.info[p.source_entry].n;
    } else {
      if (p.n_source) std::memcpy(m->h_up + at_src, p.source, (size_t)p.n_source * sizeof(float4));
      d.src = m->d_src + at_src, d.n_src = p.n_source, at_src += (size_t)p.n_source;
    }
    if (p.target_entry >= 0) {
      const lins_submap_info& z = av.info[p.target_entry];
      d.tgt = av.d_out + av.off[p.target_entry], d.n_tgt = z.n;
      jb.off_raw = av.off[p.target_entry];
      if (av.filtered[p.target_entry] || z.n == 0) {  // the assembly's own box (an empty cloud: min 0, dim 1)
        for (int a = 0; a < 3; ++a) jb.cmin[a] = z.box_min[a], jb.cdim[a] = z.box_dim[a];
      } else {  // an unfiltered cloud carries no box: take it from a copy
        tmp.resize(z.n);
        HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), d.tgt, (size_t)z.n * sizeof(float4), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        box_of(tmp.data(), z.n, jb.cmin, jb.cdim);
      }
    } else {
      if (p.n_target) std::memcpy(m->h_up + up_src + at_tgt, p.target, (size_t)p.n_target * sizeof(float4));
      d.tgt = m->d_raw + at_tgt, d.n_tgt = p.n_target;
      jb.off_raw = (long long)at_tgt, at_tgt += (size_t)p.n_target;
      box_of(p.target, p.n_target, jb.cmin, jb.cdim);
    }
    long long ncell = 1;
    for (int a = 0; a < 3; ++a) ncell *= jb.cdim[a];
    if (ncell > (1ll << 26)) {  // (cloud_box's limit of the scan-to-map row)
      d.status = LINS_E_CAPACITY;
      for (int a = 0; a < 3; ++a) d.g.cmin[a] = 0, d.g.cdim[a] = 1;
      continue;
    }
    jb.n = d.n_tgt, jb.ncell = (int)ncell;
    jb.off_pts = (long long)tot_pts, jb.off_cells = (long long)tot_cells;
    d.g.off_pts = jb.off_pts, d.g.off_cells = jb.off_cells;
    for (int a = 0; a < 3; ++a) d.g.cmin[a] = jb.cmin[a], d.g.cdim[a] = jb.cdim[a];
    tot_pts += (size_t)jb.n, tot_cells += 2 * ((size_t)jb.ncell + 1);  // starts + scratch cursors
    (p.target_entry >= 0 ? jobs_entry : jobs_host).push_back(jb);
    max_src = std::max(max_src, d.n_src);
  }
  P.bpp = std::max(1, (max_src + kLoopQPerBlock - 1) / kLoopQPerBlock);
  const size_t nh = jobs_host.size(), ne = jobs_entry.size();
  jobs_host.insert(jobs_host.end(), jobs_entry.begin(), jobs_entry.end());
  BUF_TRY(ctx, m->d_pts.grow(tot_pts));
  BUF_TRY(ctx, m->d_cells.grow(tot_cells));
  BUF_TRY(ctx, m->d_probs.grow((size_t)n));
  BUF_TRY(ctx, m->d_states.grow((size_t)n));
  BUF_TRY(ctx, m->d_jobs.grow(jobs_host.size()));
  BUF_TRY(ctx, m->d_partials.grow((size_t)n * P.bpp * kSums));
  BUF_TRY(ctx, m->d_running.grow(128));
  BUF_TRY(ctx, m->h_running.grow(1));
  if (up_src) HIP_TRY(ctx, hipMemcpyAsync(m->d_src, m->h_up, up_src * sizeof(float4), hipMemcpyHostToDevice, st));
  if (up_tgt) HIP_TRY(ctx, hipMemcpyAsync(m->d_raw, m->h_up + up_src, up_tgt * sizeof(float4), hipMemcpyHostToDevice, st));
  if (!jobs_host.empty()) HIP_TRY(ctx, hipMemcpyAsync(m->d_jobs, jobs_host.data(), jobs_host.size() * sizeof(MapGridJob), hipMemcpyHostToDevice, st));
  if (nh) launch_map_grid(st, (int)nh, m->d_jobs, m->d_raw, m->d_pts, m->d_cells);
  if (ne) launch_map_grid(st, (int)ne, m->d_jobs + nh, av.d_out, m->d_pts, m->d_cells);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(m->d_probs, P.dev.data(), (size_t)n * sizeof(LoopDev), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));  // (the job and descriptor vectors go out of scope)
  return LINS_OK;
}

bool params_ok(const lins_loop_icp_params* p) {
  return p && p->max_iterations >= 1 && p->min_correspondences >= 0 && std::isfinite(p->max_corr_dist);
}

}  // namespace

namespace lins {
int loop_icp_debug_set(lins_ctx* ctx, int which, int value) {
  if (!ctx || value < 0) return LINS_E_ARG;
  LoopMem* m = mem_of(ctx);
  if (which == 0) m->max_rounds = value;
  else if (which == 1) m->shells = value;
  else if (which == 2) m->group = value ? value : kLoopGroup;
  else return LINS_E_ARG;
  return LINS_OK;
}
int loop_icp_debug_shells_default() { return kLoopShells; }
unsigned loop_icp_last_far(lins_ctx* ctx) { return mem_of(ctx)->last_far; }
}  // namespace lins

extern "C" {

void lins_loop_icp_default_params(lins_loop_icp_params* p) {
  if (p) lins_licp::default_params(p);
}

// T0: null (every problem starts from the identity) or n x 16 start transforms, checked by the caller
static int icp_batch(lins_ctx* ctx, int n, const lins_loop_icp_problem* in, const double* T0, const lins_loop_icp_params* prm, lins_loop_icp_result* out) {
  if (!ctx || n < 0 || (n && (!in || !out)) || !params_ok(prm)) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  LoopMem* m = mem_of(ctx);
  Prepared P;
  int rc = prepare(ctx, m, n, in, P);
  if (rc) return rc;
  hipStream_t st = ctx_stream(ctx);
  std::vector<State> states(n);
  for (int k = 0; k < n; ++k) {
    lins_licp::state_init(states[k]);
    if (T0) std::memcpy(states[k].T, T0 + 16 * (size_t)k, sizeof states[k].T), lins_licp::make_move(states[k].T, states[k].M);
  }
  const float cap2 = prm->max_corr_dist * prm->max_corr_dist;
  const int max_rounds = m->max_rounds ? std::min(m->max_rounds, prm->max_iterations) : prm->max_iterations;
  hipEvent_t e0, e1;
  ctx_events(ctx, &e0, &e1);
  HIP_TRY(ctx, hipMemcpyAsync(m->d_states, states.data(), (size_t)n * sizeof(State), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(m->d_running, 0, 128 * sizeof(int), st));
  HIP_TRY(ctx, hipEventRecord(e0, st));
  for (int done = 0, g = 0; done < max_rounds; ++g) {
    const int cnt = std::min(m->group, max_rounds - done);
    int* word = m->d_running + (g & 127);
    if (g >= 128) HIP_TRY(ctx, hipMemsetAsync(word, 0, sizeof(int), st));
    for (int i = 0; i < cnt; ++i) {
      launch_loop_search(st, n, P.bpp, 0, m->shells, cap2, m->d_probs, m->d_states, m->d_pts, m->d_cells, m->d_partials, nullptr, nullptr);
      launch_loop_step(st, n, P.bpp, 0, *prm, m->d_probs, m->d_states, m->d_partials, i + 1 == cnt ? word : nullptr);
    }
    HIP_TRY(ctx, hipGetLastError());
    done += cnt;
    if (done >= max_rounds) break;
    HIP_TRY(ctx, hipMemcpyAsync(m->h_running, word, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (*m->h_running == 0) break;
  }
  launch_loop_search(st, n, P.bpp, 1, m->shells, -1.f, m->d_probs, m->d_states, m->d_pts, m->d_cells, m->d_partials, nullptr, nullptr);
  launch_loop_step(st, n, P.bpp, 1, *prm, m->d_probs, m->d_states, m->d_partials, nullptr);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(e1, st));
  HIP_TRY(ctx, hipMemcpyAsync(states.data(), m->d_states, (size_t)n * sizeof(State), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipEventElapsedTime(&m->ms, e0, e1));
  m->searches = 0, m->last_far = 0;
  for (int k = 0; k < n; ++k) {
    const State& s = states[k];
    lins_loop_icp_result& r = out[k];
    std::memset(&r, 0, sizeof r);
    std::memcpy(r.transform, s.T, sizeof r.transform);
    r.status = P.dev[k].status;
    r.fitness = s.fitness, r.mse = s.mse, r.iterations = s.iterations, r.converged = s.converged, r.reason = s.reason;
    r.n_corr = s.n_corr, r.n_fitness = s.n_fitness, r.far_searches = s.far;
    if (r.status) continue;
    // rounds searched: the fitted ones, and the one that found too few correspondences
    const int rounds = s.iterations + (s.reason == LINS_ICP_NO_CORRESPONDENCES ? 1 : 0);
    m->searches += (uint64_t)(rounds + 1) * (uint64_t)P.dev[k].n_src;
    m->last_far += s.far;
  }
  return LINS_OK;
}

int lins_loop_icp_batch(lins_ctx* ctx, int n, const lins_loop_icp_problem* in, const lins_loop_icp_params* prm, lins_loop_icp_result* out) {
  return icp_batch(ctx, n, in, nullptr, prm, out);
}

int lins_loop_icp_batch_from(lins_ctx* ctx, int n, const lins_loop_icp_problem* in, const double* T0, const lins_loop_icp_params* prm,
                             lins_loop_icp_result* out) {
  if (n > 0 && !T0) return LINS_E_ARG;
  for (size_t i = 0; n > 0 && i < 16 * (size_t)n; ++i)
    if (!std::isfinite(T0[i])) return LINS_E_INPUT;
  return icp_batch(ctx, n, in, n > 0 ? T0 : nullptr, prm, out);
}

int lins_loop_icp_correspondences(lins_ctx* ctx, const lins_loop_icp_problem* in, const double T[16], float cap, int32_t* idx, float* sqdist) {
  if (!ctx || !in || !T) return LINS_E_ARG;
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(T[i])) return LINS_E_INPUT;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  LoopMem* m = mem_of(ctx);
  Prepared P;
  int rc = prepare(ctx, m, 1, in, P);
  if (rc) return rc;
  if (P.dev[0].status) return P.dev[0].status;
  const int ns = P.dev[0].n_src;
  if (ns && (!idx || !sqdist)) return LINS_E_ARG;
  BUF_TRY(ctx, m->d_idx.grow((size_t)ns));
  BUF_TRY(ctx, m->d_d.grow((size_t)ns));
  hipStream_t st = ctx_stream(ctx);
  State s;
  lins_licp::state_init(s);
  std::memcpy(s.T, T, sizeof s.T);
  lins_licp::make_move(s.T, s.M);
  hipEvent_t e0, e1;
  ctx_events(ctx, &e0, &e1);
  HIP_TRY(ctx, hipMemcpyAsync(m->d_states, &s, sizeof s, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipEventRecord(e0, st));
  launch_loop_search(st, 1, P.bpp, 0, m->shells, cap > 0.f ? cap * cap : -1.f, m->d_probs, m->d_states, m->d_pts, m->d_cells, m->d_partials, m->d_idx,
                     m->d_d);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(e1, st));
  if (ns) {
    HIP_TRY(ctx, hipMemcpyAsync(idx, m->d_idx, (size_t)ns * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(sqdist, m->d_d, (size_t)ns * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx, hipMemcpyAsync(&s, m->d_states, sizeof s, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipEventElapsedTime(&m->ms, e0, e1));
  m->searches = (uint64_t)ns, m->last_far = s.far;
  return LINS_OK;
}

int lins_last_loop_icp_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* searches) {
  if (!ctx) return LINS_E_ARG;
  LoopMem* m = mem_of(ctx);
  if (kernel_ms) *kernel_ms = m->ms;
  if (searches) *searches = m->searches;
  return LINS_OK;
}

}  // extern "C"
