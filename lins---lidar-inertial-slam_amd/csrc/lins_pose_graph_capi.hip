// lins_pose_graph_capi.hip — C ABI of the pose graph (include/lins_map.h lins_pose_graph_*): host orchestration around
// pose_graph_kernels.hip.  The bookkeeping of a slot's graph (validation, the measurements formed in f64, the six floats
// handed back) is lins_pg::Graph, shared with the CPU restatement; the factors and the increments live on the device in
// arrays sized at init — a solve uploads only the frames and loops added since the last one — and the trials are queued
// in groups with one word "problems still running" read between the groups.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lins_lifecycle.h"
#include "../../include/lins_map.h"
#include "../../include/lins_streams_map.h"
#include "../../include/lins_team.h"
#include "host/voxel_map.h"
#include "lifecycle.h"
#include "lins_ctx_priv.h"
#include "lins_launch.h"
#include "local_map.h"
#include "pose_graph.h"
#include "pose_graph_mem.h"
#include "snapshot.h"

using namespace lins;
using lins_pg::Graph;
using lins_pg::LoopRec;
using lins_pg::Prob;
using lins_pg::State;

namespace {

// Trials queued between two reads of the "still running" word.  A trial is one launch; the solve converges
// quadratically near the optimum, in 4-8 trials on the loop closures of the tests, so groups of 4 queue at most 3 empty
// launches.  A reasoned default, not a measured one.
constexpr int kPgGroup = 4;

void pg_release(PgMem* m) { *m = PgMem(); }

}  // namespace

namespace lins {
int pose_graph_slots(lins_ctx* ctx) { return mem_of(ctx)->n_slots; }

void pose_graph_room(lins_ctx* ctx, int slot, int* frames_left, int* loops_left, int* last_latest, int* last_closest) {
  const Graph& g = mem_of(ctx)->g[slot];
  if (frames_left) *frames_left = g.max_frames - g.n_frames();
  if (loops_left) *loops_left = g.max_loops - (int)g.loops.size();
  if (last_latest) *last_latest = g.loops.empty() ? -1 : g.loops.back().latest;
  if (last_closest) *last_closest = g.loops.empty() ? -1 : g.loops.back().closest;
}

int pose_graph_apply_check(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* streams) {
  PgMem* m = mem_of(ctx);
  for (int k = 0; k < n; ++k) {
    const int slot = slots[k], stream = streams[k];
    if (slot < 0 || slot >= m->n_slots || stream < -1) return LINS_E_ARG;
    for (int i = 0; i < k; ++i)
      if (slots[i] == slot || (stream >= 0 && streams[i] == stream)) return LINS_E_ARG;  // (a slot, a stream: once)
    const int N = m->g[slot].n_frames();
    if (N == 0) return LINS_E_ARG;
    const int in_archive = lins_archive_count(ctx, slot);
    if (in_archive != LINS_E_STATE && in_archive < N) return in_archive < 0 ? in_archive : LINS_E_ARG;
    int window = 0;
    const int on_ring = local_map_slots(ctx) ? local_map_ring(ctx, slot, &window) : 0;  // (0 rings: no local map)
    if (local_map_slots(ctx) && on_ring < std::min(window, N)) return LINS_E_ARG;  // no such slot, or a ring behind the graph
    if (stream >= 0) {
      if (!streams_map_streams(ctx)) return LINS_E_STATE;
      if (stream >= streams_map_streams(ctx)) return LINS_E_ARG;
    }
    if (in_archive != LINS_E_STATE || on_ring > 0) {  // what lins_archive_set_poses / lins_local_map_set_pose take
      lins_key_pose p;
      for (int i = 0; i < N; ++i) {
        m->g[slot].key_pose(i, &p);
        if (!lins_hostmap::pose_ok(p)) return LINS_E_INPUT;
      }
    }
  }
  return LINS_OK;
}

// (lifecycle.h) the graphs of the slots named as lins_pose_graph_init leaves them: no frames, no loops, nothing of
// them on the device (the next solve uploads from frame 0)
int pose_graph_release_apply(lins_ctx* ctx, int n, const int32_t* slots) {
  PgMem* m = mem_of(ctx);
  for (int k = 0; k < n; ++k) {
    Graph& g = m->g[slots[k]];
    const int max_frames = g.max_frames, max_loops = g.max_loops;
    g = Graph();
    g.max_frames = max_frames, g.max_loops = max_loops;
    m->up_frames[slots[k]] = m->up_loops[slots[k]] = 0;
  }
  return LINS_OK;
}

// ---- snapshot.h.  The host's Graph travels whole (Z, T, held, the loops' measurements; its D mirrors Z in this
// library).  Of what prob_of addresses, a solve reads before it writes (pose_graph.h solve_begin / solve_trial):
//   Z, D     rows below up_frames — D holds the solved increments after a solve with loops, nowhere else
//   loops    Z, var, latest, closest of the records below up_loops — the host's records, uploaded again (up_loops = 0)
// and writes before it reads: I, Q, T (phase_poses from D), Dt, Tt, B, c, P, q, S, y, the loops' M, r, w, and the state
// (uploaded).  So the D rows travel through the kernel, the Z rows are uploaded from the restored Graph, and the next
// solve starts from the same bits.
void pose_graph_snapshot_context(lins_ctx* ctx, SnapContext& c) {
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return;
  c.modules |= LINS_SNAP_GRAPH;
  c.base[LINS_SNAP_BUF_PG_D] = m->d_D.get(), c.units[LINS_SNAP_BUF_PG_D] = (int64_t)m->n_slots * m->F * 12;
}

int pose_graph_snapshot_describe(lins_ctx* ctx, int slot, SnapStream& s) {
  PgMem* m = mem_of(ctx);
  const Graph& g = m->g[slot];
  const size_t N = (size_t)g.n_frames(), L = g.loops.size();
  s.modules |= LINS_SNAP_GRAPH;
  s.counts.graph_frames = (int32_t)N, s.counts.graph_loops = (int32_t)L, s.counts.graph_up_frames = m->up_frames[slot];
  s.place.graph_off = (int64_t)slot * m->F * 12;
  char* p = s.host_section<char>(LINS_SNAP_SEC_PG_HOST, 216 * N + sizeof(lins_snapshot_loop) * L);
  std::memcpy(p, g.Z.data(), 96 * N), std::memcpy(p + 96 * N, g.T.data(), 96 * N), std::memcpy(p + 192 * N, g.held.data(), 24 * N);
  for (size_t l = 0; l < L; ++l) {
    lins_snapshot_loop R;
    std::memset(&R, 0, sizeof R);
    std::memcpy(R.Z, g.loops[l].Z, sizeof R.Z);
    R.var = g.loops[l].var, R.latest = g.loops[l].latest, R.closest = g.loops[l].closest;
    std::memcpy(p + 216 * N + l * sizeof R, &R, sizeof R);
  }
  return LINS_OK;
}

int pose_graph_restore_check(lins_ctx* ctx, int slot, lins_snapshot_limits& lim) {
  PgMem* m = mem_of(ctx);
  const Graph& g = m->g[slot];
  if (g.n_frames() || !g.loops.empty() || m->up_frames[slot] || m->up_loops[slot]) return LINS_E_STATE;
  lim.graph_frames = g.max_frames, lim.graph_loops = g.max_loops;
  return LINS_OK;
}

void pose_graph_restore_place(lins_ctx* ctx, int slot, const SnapView& v, SnapStream& s) {
  s.place.graph_off = (int64_t)slot * mem_of(ctx)->F * 12;
}

int pose_graph_restore_apply(lins_ctx* ctx, int slot, const SnapView& v) {
  PgMem* m = mem_of(ctx);
  Graph& g = m->g[slot];
  const size_t N = (size_t)v.info.counts.graph_frames, L = (size_t)v.info.counts.graph_loops, up = (size_t)v.info.counts.graph_up_frames;
  const char* p = v.sec(LINS_SNAP_SEC_PG_HOST);
  g.Z.resize(12 * N), g.T.resize(12 * N), g.held.resize(6 * N);
  std::memcpy(g.Z.data(), p, 96 * N), std::memcpy(g.T.data(), p + 96 * N, 96 * N), std::memcpy(g.held.data(), p + 192 * N, 24 * N);
  g.D = g.Z;
  g.loops.assign(L, LoopRec{});
  for (size_t l = 0; l < L; ++l) {
    lins_snapshot_loop R;
    std::memcpy(&R, p + 216 * N + l * sizeof R, sizeof R);
    std::memcpy(g.loops[l].Z, R.Z, sizeof R.Z);
    g.loops[l].var = R.var, g.loops[l].latest = R.latest, g.loops[l].closest = R.closest;
  }
  m->up_frames[slot] = (int)up, m->up_loops[slot] = 0;
  if (up) {
    hipStream_t st = ctx_stream(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(m->d_Z + (size_t)slot * m->F * 12, g.Z.data(), 96 * up, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  return LINS_OK;
}
}  // namespace lins

extern "C" {

int lins_pose_graph_release_slot(lins_ctx* ctx, int slot) {
  if (!ctx) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  const int32_t s = slot;
  if (int rc = release_list_check(1, &s, m->n_slots)) return rc;
  if (int rc = ctx_quiesce(ctx)) return rc;
  return pose_graph_release_apply(ctx, 1, &s);
}

void lins_pose_graph_default_params(lins_pose_graph_params* p) {
  if (p) lins_pg::default_params(p);
}

int lins_pose_graph_init(lins_ctx* ctx, int n_slots, int max_frames, int max_loops) {
  if (!ctx || n_slots < 1 || max_frames < 1 || max_loops < 0 || max_loops > lins_pg::kMaxLoops) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  PgMem* m = mem_of(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx_stream(ctx)));
  pg_release(m);
  const size_t n = (size_t)n_slots, F = (size_t)max_frames, L = (size_t)std::max(max_loops, 1);
  m->F = max_frames, m->L = (int)L;
  for (DevBuf<double>* p : {&m->d_Z, &m->d_D, &m->d_Dt, &m->d_I, &m->d_T, &m->d_Tt}) BUF_TRY(ctx, p->grow(n * F * 12));
  BUF_TRY(ctx, m->d_Q.grow(n * m->nq() * 12));
  BUF_TRY(ctx, m->d_B.grow(n * F * 36));
  BUF_TRY(ctx, m->d_P.grow(n * F * 36));
  BUF_TRY(ctx, m->d_c.grow(n * F * 6));
  BUF_TRY(ctx, m->d_q.grow(n * F * 6));
  BUF_TRY(ctx, m->d_S.grow(n * 36 * L * L));
  BUF_TRY(ctx, m->d_y.grow(n * 18 * L));
  BUF_TRY(ctx, m->d_loops.grow(n * L));
  BUF_TRY(ctx, m->d_st.grow(n));
  BUF_TRY(ctx, m->d_probs.grow(n));
  BUF_TRY(ctx, m->d_running.grow(128));
  BUF_TRY(ctx, m->h_running.grow(1));
  m->g.assign(n, Graph());
  for (Graph& g : m->g) g.max_frames = max_frames, g.max_loops = max_loops;
  m->up_frames.assign(n, 0), m->up_loops.assign(n, 0);
  m->n_slots = n_slots;
  return LINS_OK;
}

int lins_pose_graph_push(lins_ctx* ctx, int slot, const float last6[6], const float aft6[6]) {
  if (!ctx) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n_slots) return LINS_E_ARG;
  return m->g[slot].push(last6, aft6);
}

int lins_pose_graph_add_loop(lins_ctx* ctx, int slot, int latest_id, int closest_id, const lins_key_pose* pose_from, double fitness) {
  if (!ctx) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n_slots) return LINS_E_ARG;
  const int rc = m->g[slot].add_loop(latest_id, closest_id, pose_from, fitness);
  return rc < 0 ? rc : LINS_OK;
}

int lins_pose_graph_solve(lins_ctx* ctx, int n, const int32_t* slots, const lins_pose_graph_params* prm, lins_pose_graph_result* out) {
  if (!ctx || n < 0 || (n && (!slots || !out)) || !lins_pg::params_ok(prm)) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (n > m->n_slots) return LINS_E_ARG;
  std::vector<char> seen(m->n_slots, 0);
  for (int k = 0; k < n; ++k) {
    if (slots[k] < 0 || slots[k] >= m->n_slots || seen[slots[k]]) return LINS_E_ARG;
    seen[slots[k]] = 1;
  }
  m->ms = 0.f, m->iterations = 0;
  std::vector<int> run;  // the entries with loops: the others are returned with the bits they hold
  for (int k = 0; k < n; ++k) {
    std::memset(out + k, 0, sizeof out[k]);
    const Graph& g = m->g[slots[k]];
    if (!g.loops.empty() && g.n_frames() >= 2) run.push_back(k);
  }
  if (run.empty()) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t st = ctx_stream(ctx);
  const int nr = (int)run.size();
  std::vector<Prob> probs(nr);
  std::vector<State> states(nr);
  for (int i = 0; i < nr; ++i) {
    const int slot = slots[run[i]];
    const Graph& g = m->g[slot];
    probs[i] = prob_of(m, slot, i);
    lins_pg::state_init(states[i], *prm);
    const int f0 = m->up_frames[slot], f1 = g.n_frames(), l0 = m->up_loops[slot], l1 = (int)g.loops.size();
    if (f1 > f0) {  // a new frame's increment starts at its measurement
      HIP_TRY(ctx, hipMemcpyAsync(probs[i].Z + 12 * (size_t)f0, g.Z.data() + 12 * (size_t)f0, 12 * (size_t)(f1 - f0) * sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, hipMemcpyAsync(probs[i].D + 12 * (size_t)f0, g.Z.data() + 12 * (size_t)f0, 12 * (size_t)(f1 - f0) * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (l1 > l0) HIP_TRY(ctx, hipMemcpyAsync(probs[i].loops + l0, g.loops.data() + l0, (size_t)(l1 - l0) * sizeof(LoopRec), hipMemcpyHostToDevice, st));
  }
  HIP_TRY(ctx, hipMemcpyAsync(m->d_probs, probs.data(), (size_t)nr * sizeof(Prob), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(m->d_st, states.data(), (size_t)nr * sizeof(State), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(m->d_running, 0, 128 * sizeof(int), st));
  HIP_TRY(ctx, hipStreamSynchronize(st));  // (pageable sources: the graphs' vectors may grow behind this call)
  for (int i = 0; i < nr; ++i) m->up_frames[slots[run[i]]] = probs[i].n_frames, m->up_loops[slots[run[i]]] = probs[i].n_loops;
  hipEvent_t e0, e1;
  ctx_events(ctx, &e0, &e1);
  HIP_TRY(ctx, hipEventRecord(e0, st));
  launch_pose_graph_begin(st, nr, m->d_probs);
  for (int done = 0, grp = 0; done < prm->max_iterations; ++grp) {
    const int cnt = std::min(kPgGroup, prm->max_iterations - done);
    int* word = m->d_running + (grp & 127);
    if (grp >= 128) HIP_TRY(ctx, hipMemsetAsync(word, 0, sizeof(int), st));
    for (int i = 0; i < cnt; ++i) launch_pose_graph_trial(st, nr, m->d_probs, *prm, i + 1 == cnt ? word : nullptr);
    HIP_TRY(ctx, hipGetLastError());
    done += cnt;
    if (done >= prm->max_iterations) break;
    HIP_TRY(ctx, hipMemcpyAsync(m->h_running, word, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (*m->h_running == 0) break;
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(e1, st));
  std::vector<std::vector<double>> T(nr);
  for (int i = 0; i < nr; ++i) {
    T[i].resize(12 * (size_t)probs[i].n_frames);
    HIP_TRY(ctx, hipMemcpyAsync(T[i].data(), probs[i].T, T[i].size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx, hipMemcpyAsync(states.data(), m->d_st, (size_t)nr * sizeof(State), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipEventElapsedTime(&m->ms, e0, e1));
  for (int i = 0; i < nr; ++i) {
    const State& s = states[i];
    lins_pose_graph_result& r = out[run[i]];
    r.cost_before = s.cost0, r.cost_after = s.cost, r.max_increment = s.max_inc;
    r.iterations = s.iterations, r.reason = s.reason, r.status = LINS_OK;
    m->iterations += (uint64_t)s.iterations;
    m->g[slots[run[i]]].store_solution(T[i].data(), nullptr);
  }
  return LINS_OK;
}

int lins_pose_graph_poses(lins_ctx* ctx, int slot, int first_id, int n, lins_key_pose* out) {
  if (!ctx) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n_slots || first_id < 0 || n < 0 || (long long)first_id + n > m->g[slot].n_frames() || (n && !out)) return LINS_E_ARG;
  for (int i = 0; i < n; ++i) m->g[slot].key_pose(first_id + i, out + i);
  return LINS_OK;
}

int lins_pose_graph_count(lins_ctx* ctx, int slot, int32_t* n_loops) {
  if (!ctx) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n_slots) return LINS_E_ARG;
  if (n_loops) *n_loops = (int32_t)m->g[slot].loops.size();
  return m->g[slot].n_frames();
}

int lins_pose_graph_apply_batch(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* streams) {
  if (!ctx || n < 0 || (n && (!slots || !streams))) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  // everything that can refuse is asked first, so that a refused call changes nothing
  if (int rc = pose_graph_apply_check(ctx, n, slots, streams)) return rc;
  const bool archive = lins_archive_count(ctx, 0) != LINS_E_STATE;
  std::vector<int32_t> to;  // the streams written, and their newest poses
  std::vector<float> six;
  std::vector<lins_key_pose> poses;
  for (int k = 0; k < n; ++k) {
    const Graph& g = m->g[slots[k]];
    const int N = g.n_frames();
    poses.resize(N);
    for (int i = 0; i < N; ++i) g.key_pose(i, &poses[i]);
    if (archive) {  // correctPoses over the whole history
      if (int rc = lins_archive_set_poses(ctx, slots[k], 0, N, poses.data())) return rc;
    }
    const int on_ring = local_map_slots(ctx) ? local_map_ring(ctx, slots[k], nullptr) : 0;  // (0 rings: no local map)
    for (int age = 0; age < std::min(on_ring, N); ++age) {  // ... and over the ring: its frames are the newest, by age
      if (int rc = lins_local_map_set_pose(ctx, slots[k], age, &poses[N - 1 - age])) return rc;
    }
    if (streams[k] >= 0) {
      const float* p = &g.held[6 * (size_t)(N - 1)];
      to.push_back(streams[k]), six.insert(six.end(), p, p + 6);
    }
  }
  return streams_map_correct(ctx, (int)to.size(), to.data(), six.data());  // LM:1737-1749
}

}  // extern "C"

namespace {

// what lins_pose_graph_rebase_batch refuses
int rebase_check(PgMem* m, int n, const int32_t* slots, const double* X) {
  if (n > m->n_slots) return LINS_E_ARG;
  for (int k = 0; k < n; ++k) {
    if (slots[k] < 0 || slots[k] >= m->n_slots || m->g[slots[k]].n_frames() == 0) return LINS_E_ARG;
    for (int i = 0; i < k; ++i)
      if (slots[i] == slots[k]) return LINS_E_ARG;
  }
  for (int k = 0; k < n; ++k)
    if (!lins_pg::rebase_x_ok(X + 16 * (size_t)k)) return LINS_E_INPUT;
  return LINS_OK;
}

// The rebase of n checked slots.  The device's copy of a slot is brought up to its graph as a solve does it, the new prior
// goes into row 0 of its Z, the solve's begin launch forms the poses, and they come back.  poses_ok: what the caller
// goes on to do with the poses takes them (lins_team_rebase: lins_pose_graph_apply_batch's pose_ok); when it does not, the
// old priors go back into the device's rows — T on the device is written before it is read by every solve — and nothing
// of the graphs has changed.
int rebase_run(lins_ctx* ctx, PgMem* m, int n, const int32_t* slots, const double* X, bool poses_ok) {
  if (n == 0) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t st = ctx_stream(ctx);
  std::vector<Prob> probs(n);
  std::vector<State> states(n);
  std::vector<double> Z0(12 * (size_t)n), old(12 * (size_t)n);
  lins_pose_graph_params prm;
  lins_pg::default_params(&prm);
  for (int i = 0; i < n; ++i) {
    const int slot = slots[i];
    const Graph& g = m->g[slot];
    double Xg[12];
    lins_pg::rebase_x_pose(X + 16 * (size_t)i, Xg);
    g.rebased_prior(Xg, &Z0[12 * (size_t)i]);
    lins_pg::pose_copy(g.Z.data(), &old[12 * (size_t)i]);
    probs[i] = prob_of(m, slot, i);
    lins_pg::state_init(states[i], prm);
    const int f0 = m->up_frames[slot], f1 = g.n_frames(), l0 = m->up_loops[slot], l1 = (int)g.loops.size();
    if (f1 > f0) {
      HIP_TRY(ctx, hipMemcpyAsync(probs[i].Z + 12 * (size_t)f0, g.Z.data() + 12 * (size_t)f0, 12 * (size_t)(f1 - f0) * sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, hipMemcpyAsync(probs[i].D + 12 * (size_t)f0, g.Z.data() + 12 * (size_t)f0, 12 * (size_t)(f1 - f0) * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (l1 > l0) HIP_TRY(ctx, hipMemcpyAsync(probs[i].loops + l0, g.loops.data() + l0, (size_t)(l1 - l0) * sizeof(LoopRec), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(probs[i].Z, &Z0[12 * (size_t)i], 12 * sizeof(double), hipMemcpyHostToDevice, st));  // the changed prior
  }
  HIP_TRY(ctx, hipMemcpyAsync(m->d_probs, probs.data(), (size_t)n * sizeof(Prob), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(m->d_st, states.data(), (size_t)n * sizeof(State), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i) m->up_frames[slots[i]] = probs[i].n_frames, m->up_loops[slots[i]] = probs[i].n_loops;
  launch_pose_graph_begin(st, n, m->d_probs);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<std::vector<double>> T(n);
  for (int i = 0; i < n; ++i) {
    T[i].resize(12 * (size_t)probs[i].n_frames);
    HIP_TRY(ctx, hipMemcpyAsync(T[i].data(), probs[i].T, T[i].size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  bool ok = true;
  for (int i = 0; i < n && ok && poses_ok; ++i)
    for (int k = 0; k < probs[i].n_frames && ok; ++k) {
      float p[6];
      lins_pg::pose_to6(&T[i][12 * (size_t)k], p);
      ok = lins_hostmap::pose_ok(lins_key_pose{p[3], p[4], p[5], p[0], p[1], p[2]});
    }
  if (!ok) {
    for (int i = 0; i < n; ++i) HIP_TRY(ctx, hipMemcpyAsync(probs[i].Z, &old[12 * (size_t)i], 12 * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return LINS_E_INPUT;
  }
  for (int i = 0; i < n; ++i) m->g[slots[i]].store_rebased(&Z0[12 * (size_t)i], T[i].data());
  return LINS_OK;
}

}  // namespace

extern "C" {

int lins_pose_graph_rebase_batch(lins_ctx* ctx, int n, const int32_t* slots, const double* X) {
  if (!ctx || n < 0 || (n && (!slots || !X))) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (int rc = rebase_check(m, n, slots, X)) return rc;
  return rebase_run(ctx, m, n, slots, X, false);
}

int lins_team_rebase(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* streams, const double* X) {
  if (!ctx || n < 0 || (n && (!slots || !streams || !X))) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  // the union of the two calls' refusals, asked first (the poses as they stand; the rebased ones inside rebase_run)
  if (int rc = rebase_check(m, n, slots, X)) return rc;
  if (int rc = pose_graph_apply_check(ctx, n, slots, streams)) return rc;
  const bool taken = lins_archive_count(ctx, 0) != LINS_E_STATE || local_map_slots(ctx) > 0;  // (what pose_graph_apply_check looks at)
  if (int rc = rebase_run(ctx, m, n, slots, X, taken)) return rc;
  return lins_pose_graph_apply_batch(ctx, n, slots, streams);
}

int lins_pose_graph_apply(lins_ctx* ctx, int slot, int stream) {
  const int32_t s = slot, t = stream;
  return lins_pose_graph_apply_batch(ctx, 1, &s, &t);
}

int lins_last_pose_graph_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* iterations) {
  if (!ctx) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (kernel_ms) *kernel_ms = m->ms;
  if (iterations) *iterations = m->iterations;
  return LINS_OK;
}

int lins_debug_pose_graph_poses_f64(lins_ctx* ctx, int slot, int first_id, int n, double* out) {
  if (!ctx) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n_slots || first_id < 0 || n < 0 || (long long)first_id + n > m->g[slot].n_frames() || (n && !out)) return LINS_E_ARG;
  std::memcpy(out, m->g[slot].T.data() + 12 * (size_t)first_id, 12 * (size_t)n * sizeof(double));
  return LINS_OK;
}

int lins_debug_pose_graph_loop_z(lins_ctx* ctx, int slot, int loop, double z[12]) {
  if (!ctx || !z) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n_slots || loop < 0 || loop >= (int)m->g[slot].loops.size()) return LINS_E_ARG;
  std::memcpy(z, m->g[slot].loops[loop].Z, 12 * sizeof(double));
  return LINS_OK;
}

}  // extern "C"
