// pose_graph.cpp — the CPU restatement of the pose graph (include/lins_host.h lins_host_pose_graph_*): the phases of
// csrc/pose_graph.h run lane by lane, in the order the device's workgroup runs them.
#include "../pose_graph.h"

#include <cstring>
#include <vector>

#include "pose_graph_host.h"

using namespace lins_pg;

namespace {

struct Work {  // the arrays of one problem
  std::vector<double> Z, D, Dt, I, T, Tt, Q, B, c, P, q, S, y;
  std::vector<LoopRec> loops;
  State st;
  Prob prob(const Graph& g) {
    const size_t F = (size_t)g.n_frames(), L = g.loops.size();
    Z = g.Z, D = g.D;
    Dt.assign(12 * F, 0.0), I.assign(12 * F, 0.0), T.assign(12 * F, 0.0), Tt.assign(12 * F, 0.0);
    Q.assign(12 * (F / kPrefixBlock + 2), 0.0), B.assign(36 * F, 0.0), c.assign(6 * F, 0.0), P.assign(36 * F, 0.0), q.assign(6 * F, 0.0);
    S.assign(36 * L * L, 0.0), y.assign(18 * L, 0.0);
    loops = g.loops;
    Prob p{};
    p.n_frames = (int)F, p.n_loops = (int)L;
    p.Z = Z.data(), p.D = D.data(), p.Dt = Dt.data(), p.I = I.data(), p.T = T.data(), p.Tt = Tt.data(), p.Q = Q.data();
    p.B = B.data(), p.c = c.data(), p.P = P.data(), p.q = q.data(), p.loops = loops.data(), p.S = S.data(), p.y = y.data();
    p.st = &st;
    return p;
  }
};

}  // namespace

extern "C" {

void lins_pose_graph_default_params(lins_pose_graph_params* p) {
  if (p) default_params(p);
}

lins_host_pose_graph* lins_host_pose_graph_create(int max_frames, int max_loops) {
  if (max_frames < 1 || max_loops < 0) return nullptr;
  lins_host_pose_graph* h = new lins_host_pose_graph();
  h->g.max_frames = max_frames, h->g.max_loops = max_loops;
  return h;
}
void lins_host_pose_graph_destroy(lins_host_pose_graph* g) { delete g; }

int lins_host_pose_graph_push(lins_host_pose_graph* g, const float last6[6], const float aft6[6]) {
  return g ? g->g.push(last6, aft6) : LINS_E_ARG;
}
int lins_host_pose_graph_add_loop(lins_host_pose_graph* g, int latest_id, int closest_id, const lins_key_pose* pose_from, double fitness) {
  if (!g) return LINS_E_ARG;
  const int rc = g->g.add_loop(latest_id, closest_id, pose_from, fitness);
  return rc < 0 ? rc : LINS_OK;
}

int lins_host_pose_graph_solve(lins_host_pose_graph* h, const lins_pose_graph_params* prm, lins_pose_graph_result* out) {
  if (!h || !out || !lins_pg::params_ok(prm)) return LINS_E_ARG;
  Graph& g = h->g;
  std::memset(out, 0, sizeof *out);
  if (g.loops.empty() || g.n_frames() < 2) return LINS_OK;  // the bits it holds, 0 iterations
  Work w;
  Prob P = w.prob(g);
  state_init(w.st, *prm);
  double sh[kShared];
  HostExec ex;
  solve_begin(ex, P, sh);
  while (w.st.active) solve_trial(ex, P, *prm, sh);
  g.store_solution(P.T, P.D);
  out->cost_before = w.st.cost0, out->cost_after = w.st.cost, out->max_increment = w.st.max_inc;
  out->iterations = w.st.iterations, out->reason = w.st.reason, out->status = LINS_OK;
  return LINS_OK;
}

int lins_host_pose_graph_rebase(lins_host_pose_graph* h, const double X[16]) {
  if (!h || !X || h->g.n_frames() == 0) return LINS_E_ARG;
  if (!rebase_x_ok(X)) return LINS_E_INPUT;
  Graph& g = h->g;
  double Xg[12], Z0[12];
  rebase_x_pose(X, Xg);
  g.rebased_prior(Xg, Z0);
  Work w;
  Prob P = w.prob(g);
  pose_copy(Z0, P.Z);
  lins_pose_graph_params prm;
  default_params(&prm);
  state_init(w.st, prm);
  double sh[kShared];
  solve_begin(HostExec{}, P, sh);  // phase_poses from the increments as they stand, in the solve's prefix order
  g.store_rebased(Z0, P.T);
  return LINS_OK;
}

int lins_host_pose_graph_poses(lins_host_pose_graph* h, int first_id, int n, lins_key_pose* out) {
  if (!h || first_id < 0 || n < 0 || first_id + n > h->g.n_frames() || (n && !out)) return LINS_E_ARG;
  for (int i = 0; i < n; ++i) h->g.key_pose(first_id + i, out + i);
  return LINS_OK;
}
int lins_host_pose_graph_count(lins_host_pose_graph* h, int32_t* n_loops) {
  if (!h) return LINS_E_ARG;
  if (n_loops) *n_loops = (int32_t)h->g.loops.size();
  return h->g.n_frames();
}
int lins_host_pose_graph_poses_f64(lins_host_pose_graph* h, int first_id, int n, double* out) {
  if (!h || first_id < 0 || n < 0 || first_id + n > h->g.n_frames() || (n && !out)) return LINS_E_ARG;
  std::memcpy(out, h->g.T.data() + 12 * (size_t)first_id, 12 * (size_t)n * sizeof(double));
  return LINS_OK;
}
int lins_host_pose_graph_loop_z(lins_host_pose_graph* h, int loop, double z[12]) {
  if (!h || loop < 0 || loop >= (int)h->g.loops.size() || !z) return LINS_E_ARG;
  std::memcpy(z, h->g.loops[loop].Z, 12 * sizeof(double));
  return LINS_OK;
}

int lins_host_pose_graph_linearize(lins_host_pose_graph* h, const double* poses, double* r_odo, double* D, double* gvec, double* r_loop, double* M) {
  if (!h) return LINS_E_ARG;
  const Graph& g = h->g;
  const double* T = poses ? poses : g.T.data();
  for (int k = 1; k < g.n_frames(); ++k) {
    double Dk[12], r[6], H[36], gg[6];
    between(T + 12 * (k - 1), T + 12 * k, Dk);
    lin_odometry(&g.Z[12 * (size_t)k], Dk, r, H, gg);
    if (r_odo) std::memcpy(r_odo + 6 * (k - 1), r, sizeof r);
    if (D) std::memcpy(D + 36 * (k - 1), H, sizeof H);
    if (gvec) std::memcpy(gvec + 6 * (k - 1), gg, sizeof gg);
  }
  for (size_t l = 0; l < g.loops.size(); ++l) {
    const LoopRec& R = g.loops[l];
    double r[6], Ml[36];
    lin_loop(R.Z, T + 12 * R.latest, T + 12 * R.closest, R.latest > R.closest, r, Ml);
    if (r_loop) std::memcpy(r_loop + 6 * l, r, sizeof r);
    if (M) std::memcpy(M + 36 * l, Ml, sizeof Ml);
  }
  return LINS_OK;
}

void lins_host_pose_from6(const float p[6], double T[12]) { pose_from6(p, T); }
void lins_host_pose_to6(const double T[12], float p[6]) { pose_to6(T, p); }

}  // extern "C"
