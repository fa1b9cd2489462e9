// loop_icp.cpp — the loop-closure ICP on the CPU (include/lins_host.h lins_host_loop_icp*): the restatement
// lins_loop_icp_batch (loop_icp_kernels.hip) is checked against.  performLoopClosure's alignment (LM:1114-1141) as the
// contract of include/lins_map.h states it: the arithmetic is ../loop_icp_math.h (the text the device compiles too),
// the search here is the exhaustive one, and the sums run in the contract's order — per tile of 32 source points the
// fixed tree over each eight, the four eights in order, the tiles in order.  Also the camera / lidar frame shuffle of
// LM:1156-1166 (lins_host_loop_pose_from), all f32.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../../include/lins_host.h"
#include "../loop_icp_math.h"
#include "loop_step.h"
#include "voxel_map.h"

using namespace lins_licp;
using lins_hostmap::cloud_ok;

namespace {

// steps 1-2 for every source point at M; cap2 < 0: no cap
void correspond(const lins_point* S, int ns, const lins_point* G, int ng, const float* M, float cap2, int32_t* idx, float* sq, float* moved) {
  for (int i = 0; i < ns; ++i) {
    float x, y, z;
    move_point(M, S[i].x, S[i].y, S[i].z, x, y, z);
    int best = -1;
    float bd = 0.f;
    for (int j = 0; j < ng; ++j) {
      const float d = sqdist(x, y, z, G[j].x, G[j].y, G[j].z);
      if (best < 0 || d < bd) best = j, bd = d;  // (ascending j: an equal d keeps the smaller index)
    }
    if (best >= 0 && cap2 >= 0.f && !(bd <= cap2)) best = -1;
    idx[i] = best, sq[i] = best >= 0 ? bd : 0.f;
    if (moved) moved[3 * i] = x, moved[3 * i + 1] = y, moved[3 * i + 2] = z;
  }
}

void sums_in_order(const lins_point* G, int ns, const int32_t* idx, const float* sq, const float* moved, double* sums) {
  for (int k = 0; k < kSums; ++k) sums[k] = 0.0;
  for (int t0 = 0; t0 < ns; t0 += kTile) {
    double tile[kSums];
    for (int k = 0; k < kSums; ++k) tile[k] = 0.0;
    for (int w = 0; w < kTile / kGroup; ++w) {
      double term[kGroup][kSums];
      for (int e = 0; e < kGroup; ++e) {
        const int i = t0 + w * kGroup + e;
        for (int k = 0; k < kSums; ++k) term[e][k] = 0.0;
        if (i < ns && idx[i] >= 0) {
          const lins_point& g = G[idx[i]];
          corr_terms(moved[3 * i], moved[3 * i + 1], moved[3 * i + 2], g.x, g.y, g.z, sq[i], term[e]);
        }
      }
      for (int k = 0; k < kSums; ++k) {
        double q[kGroup];
        for (int e = 0; e < kGroup; ++e) q[e] = term[e][k];
        tile[k] += tree8(q);
      }
    }
    for (int k = 0; k < kSums; ++k) sums[k] += tile[k];
  }
}

bool params_ok(const lins_loop_icp_params* p) { return p && p->max_iterations >= 1 && p->min_correspondences >= 0 && std::isfinite(p->max_corr_dist); }

// T0: null (the identity) or the start transform (lins_host_loop_icp_from)
int run(const lins_point* S, int ns, const lins_point* G, int ng, const lins_loop_icp_params* prm, int max_rounds, lins_loop_icp_round* rounds,
        int cap_rounds, lins_loop_icp_result* out, const double* T0 = nullptr) {
  if (ns < 0 || ng < 0 || (ns && !S) || (ng && !G) || !params_ok(prm) || !out || max_rounds < 0 || (cap_rounds && !rounds)) return LINS_E_ARG;
  if (!cloud_ok(S, ns) || !cloud_ok(G, ng)) return LINS_E_INPUT;
  State s;
  state_init(s);
  if (T0) {
    for (int i = 0; i < 16; ++i)
      if (!std::isfinite(T0[i])) return LINS_E_INPUT;
    std::memcpy(s.T, T0, sizeof s.T);
    make_move(s.T, s.M);
  }
  std::vector<int32_t> idx(ns ? ns : 1);
  std::vector<float> sq(ns ? ns : 1), moved(ns ? 3 * (size_t)ns : 1);
  const float cap2 = prm->max_corr_dist * prm->max_corr_dist;
  int n_rounds = 0;
  double sums[kSums];
  while (s.active && (max_rounds == 0 || n_rounds < max_rounds)) {
    correspond(S, ns, G, ng, s.M, cap2, idx.data(), sq.data(), moved.data());
    sums_in_order(G, ns, idx.data(), sq.data(), moved.data(), sums);
    lins_loop_icp_round r;
    std::memset(&r, 0, sizeof r);
    std::memcpy(r.T_in, s.T, sizeof r.T_in);
    double D[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, q[4] = {0, 0, 0, 0};
    step_from_sums(*prm, sums, s, D, q);
    std::memcpy(r.delta, D, sizeof r.delta), std::memcpy(r.T_out, s.T, sizeof r.T_out), std::memcpy(r.stop, q, sizeof r.stop);
    r.n_corr = s.n_corr, r.reason = s.reason, r.mse = sums[0] > 0 ? sums[16] / sums[0] : 0.0;
    if (n_rounds < cap_rounds) rounds[n_rounds] = r;
    ++n_rounds;
  }
  correspond(S, ns, G, ng, s.M, -1.f, idx.data(), sq.data(), moved.data());
  sums_in_order(G, ns, idx.data(), sq.data(), moved.data(), sums);
  fitness_from_sums(sums, s);
  std::memset(out, 0, sizeof *out);
  std::memcpy(out->transform, s.T, sizeof out->transform);
  out->fitness = s.fitness, out->mse = s.mse, out->iterations = s.iterations, out->converged = s.converged, out->reason = s.reason;
  out->n_corr = s.n_corr, out->n_fitness = s.n_fitness, out->far_searches = 0, out->status = LINS_OK;
  return n_rounds;
}

}  // namespace

extern "C" {

void lins_loop_icp_default_params(lins_loop_icp_params* p) {
  if (p) default_params(p);
}

int lins_host_loop_icp(const lins_point* source, int n_source, const lins_point* target, int n_target, const lins_loop_icp_params* prm,
                       int max_rounds, lins_loop_icp_result* out) {
  const int rc = run(source, n_source, target, n_target, prm, max_rounds, nullptr, 0, out);
  return rc < 0 ? rc : LINS_OK;
}

int lins_host_loop_icp_from(const lins_point* source, int n_source, const lins_point* target, int n_target, const double T0[16],
                            const lins_loop_icp_params* prm, int max_rounds, lins_loop_icp_result* out) {
  if (!T0) return LINS_E_ARG;
  const int rc = run(source, n_source, target, n_target, prm, max_rounds, nullptr, 0, out, T0);
  return rc < 0 ? rc : LINS_OK;
}

int lins_host_loop_icp_trace(const lins_point* source, int n_source, const lins_point* target, int n_target, const lins_loop_icp_params* prm,
                             lins_loop_icp_round* rounds, int cap_rounds, lins_loop_icp_result* out) {
  if (cap_rounds < 0) return LINS_E_ARG;
  return run(source, n_source, target, n_target, prm, 0, rounds, cap_rounds, out);
}

int lins_host_loop_icp_correspondences(const lins_point* source, int n_source, const lins_point* target, int n_target, const double T[16],
                                       float cap, int32_t* idx, float* sqdist_out) {
  if (n_source < 0 || n_target < 0 || (n_source && (!source || !idx || !sqdist_out)) || (n_target && !target) || !T) return LINS_E_ARG;
  if (!cloud_ok(source, n_source) || !cloud_ok(target, n_target)) return LINS_E_INPUT;
  float M[12];
  make_move(T, M);
  correspond(source, n_source, target, n_target, M, cap > 0.f ? cap * cap : -1.f, idx, sqdist_out, nullptr);
  return LINS_OK;
}

int lins_host_loop_icp_step(const double sums[17], const lins_loop_icp_params* prm, int mode, lins_loop_icp_state* state, double delta[16],
                            double stop[4]) {
  if (!sums || !params_ok(prm) || !state || (mode != 0 && mode != 1) || (mode == 0 && (!delta || !stop))) return LINS_E_ARG;
  State s;
  state_from_public(*state, s);
  if (mode == 0) {
    if (!s.active) return LINS_OK;
    for (int i = 0; i < 16; ++i) delta[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 4; ++i) stop[i] = 0.0;
    step_from_sums(*prm, sums, s, delta, stop);
  } else {
    fitness_from_sums(sums, s);
  }
  state_to_public(s, *state);
  return LINS_OK;
}

int lins_host_loop_window(int latest, int closest, int search_num, int32_t* ids, int cap) {
  if (cap < 0) return LINS_E_ARG;
  const int n = lins_loop::window_size(latest, closest, search_num);
  if (n > cap) return LINS_E_CAPACITY;
  if (n && !ids) return LINS_E_ARG;
  return lins_loop::window(latest, closest, search_num, ids);
}

int lins_host_loop_candidate(int latest, int closest, int last_latest, int last_closest) {
  return lins_loop::candidate(latest, closest, last_latest, last_closest);
}

int lins_host_loop_accept(int converged, double fitness, float max_fitness) { return lins_loop::accept(converged, fitness, max_fitness) ? 1 : 0; }

int lins_host_loop_variance(double fitness, double* variance) { return lins_loop::variance(fitness, variance) ? 1 : 0; }

int lins_host_loop_choose(int k, const int32_t* converged, const double* fitness, float max_fitness) {
  if (k <= 0 || !converged || !fitness) return -1;
  return lins_loop::choose(k, converged, fitness, max_fitness);
}

int lins_host_loop_pose_from(const double T[16], const lins_key_pose* wrong, lins_key_pose* pose_from) {
  if (!T || !wrong || !pose_from) return LINS_E_ARG;
  lins_loop::pose_from(T, *wrong, pose_from);
  return LINS_OK;
}

}  // extern "C"
