// team_graph.cpp — the CPU restatement of the team graph (include/lins_host.h lins_host_team_*): the phases of
// csrc/pose_graph_team.h run lane by lane, in the order the device's workgroup runs them.
#include "../pose_graph_team.h"

#include <cstring>
#include <vector>

#include "pose_graph_host.h"

using namespace lins_pg;

namespace {

struct TeamWork {  // the arrays of one group
  std::vector<TeamMember> mt;
  std::vector<TeamFactorIn> fin;
  std::vector<double> Z, D, Dt, I, T, Tt, Q, B, c, P, q, S, y;
  std::vector<LoopRec> loops;
  std::vector<TeamSpan> spans;
  State st;
  int frames = 0, own_loops = 0;
};

// lins_team_graph_solve's refusals for one group whose slots are member indices; the member table and the factors
int team_check(int n, lins_host_pose_graph* const* graphs, const double* root_variance, int n_factors, const lins_team_factor* factors,
               bool capacity, TeamWork& w) {
  if (n < 1 || !graphs || n_factors < 0 || (n_factors && !factors) || (n > 1 && !root_variance)) return LINS_E_ARG;
  for (int i = 0; i < n; ++i) {
    if (!graphs[i] || graphs[i]->g.n_frames() == 0) return LINS_E_ARG;
    for (int j = 0; j < i; ++j)
      if (graphs[j] == graphs[i]) return LINS_E_ARG;
  }
  for (int i = 0; i < n_factors; ++i) {
    const lins_team_factor& f = factors[i];
    if (f.slot_b < 0 || f.slot_b >= n || f.slot_a < 0 || f.slot_a >= n || f.slot_a == f.slot_b) return LINS_E_ARG;
    if (f.id_b < 0 || f.id_b >= graphs[f.slot_b]->g.n_frames() || f.id_a < 0 || f.id_a >= graphs[f.slot_a]->g.n_frames()) return LINS_E_ARG;
  }
  for (int i = 6; i < 6 * n; ++i)
    if (!team_var_ok(root_variance[i])) return LINS_E_INPUT;
  for (int i = 0; i < n_factors; ++i)
    if (!team_z_ok(factors[i].Z) || !team_var_ok(factors[i].var)) return LINS_E_INPUT;
  if (n > kTeamMaxMembers) return LINS_E_CAPACITY;
  long long cap = 0;
  std::vector<int> counts(n);
  std::vector<const double*> var(n);
  w.own_loops = 0;
  for (int i = 0; i < n; ++i) {
    const Graph& g = graphs[i]->g;
    counts[i] = g.n_frames(), var[i] = root_variance ? root_variance + 6 * i : nullptr, w.own_loops += (int)g.loops.size();
    cap += g.max_loops > 1 ? g.max_loops : 1;
  }
  if (cap > kMaxLoops) cap = kMaxLoops;
  if (capacity && (long long)w.own_loops + n_factors > cap) return LINS_E_CAPACITY;
  w.mt.resize(n);
  w.frames = team_members(n, counts.data(), var.data(), w.mt.data(), nullptr);
  w.fin.clear();
  for (int i = 0; i < n_factors; ++i)
    w.fin.push_back(TeamFactorIn{factors[i].slot_b, factors[i].id_b, factors[i].slot_a, factors[i].id_a, factors[i].Z, factors[i].var});
  return LINS_OK;
}

TeamProb team_prob(TeamWork& w, int n, lins_host_pose_graph* const* graphs) {
  const size_t F = (size_t)w.frames;
  size_t q_rows = 0;
  w.Z.clear(), w.D.clear();
  std::vector<const std::vector<LoopRec>*> own(n);
  for (int i = 0; i < n; ++i) {
    const Graph& g = graphs[i]->g;
    w.Z.insert(w.Z.end(), g.Z.begin(), g.Z.end());
    w.D.insert(w.D.end(), g.D.begin(), g.D.end());
    pose_copy(&g.Z[0], &w.D[12 * (size_t)w.mt[i].off]);  // a root's estimate starts at its prior
    own[i] = &g.loops;
    q_rows += (size_t)g.n_frames() / kPrefixBlock + 2;
  }
  team_loops(n, w.mt.data(), own.data(), (int)w.fin.size(), w.fin.data(), w.loops, w.spans);
  const size_t L = w.loops.size();
  w.Dt.assign(12 * F, 0.0), w.I.assign(12 * F, 0.0), w.T.assign(12 * F, 0.0), w.Tt.assign(12 * F, 0.0);
  w.Q.assign(12 * q_rows, 0.0), w.B.assign(36 * F, 0.0), w.c.assign(6 * F, 0.0), w.P.assign(36 * F, 0.0), w.q.assign(6 * F, 0.0);
  w.S.assign(36 * L * L + 1, 0.0), w.y.assign(18 * L + 1, 0.0);
  TeamProb p{};
  p.n_members = n, p.n_frames = w.frames, p.n_loops = (int)L;
  p.members = w.mt.data();
  p.Z = w.Z.data(), p.D = w.D.data(), p.Dt = w.Dt.data(), p.I = w.I.data(), p.T = w.T.data(), p.Tt = w.Tt.data(), p.Q = w.Q.data();
  p.B = w.B.data(), p.c = w.c.data(), p.P = w.P.data(), p.q = w.q.data();
  p.loops = w.loops.data(), p.spans = w.spans.data(), p.S = w.S.data(), p.y = w.y.data();
  p.st = &w.st;
  return p;
}

}  // namespace

extern "C" {

int lins_host_team_factor(const double Tb[12], const double Ta[12], const double* X, double fitness, lins_team_factor* out) {
  if (!Tb || !Ta || !out) return LINS_E_ARG;
  const double var = (double)(float)fitness;
  if ((X && !rebase_x_ok(X)) || !team_var_ok(var)) return LINS_E_INPUT;
  double Xg[12];
  if (X) rebase_x_pose(X, Xg);
  std::memset(out, 0, sizeof *out);
  out->var = var;
  team_factor_z(Tb, Ta, X ? Xg : nullptr, out->Z);
  return LINS_OK;
}

int lins_host_team_graph_solve(int n_members, lins_host_pose_graph* const* graphs, const double* root_variance, int n_factors,
                               const lins_team_factor* factors, const lins_pose_graph_params* prm, lins_team_graph_result* out) {
  if (!out || !params_ok(prm)) return LINS_E_ARG;
  TeamWork w;
  if (int rc = team_check(n_members, graphs, root_variance, n_factors, factors, true, w)) return rc;
  std::memset(out, 0, sizeof *out);
  out->n_frames = w.frames, out->n_loops = w.own_loops, out->n_factors = n_factors;
  if (w.own_loops + n_factors == 0) return LINS_OK;  // the bits it holds, 0 iterations
  TeamProb G = team_prob(w, n_members, graphs);
  state_init(w.st, *prm);
  std::vector<double> sh(kTeamShared);
  HostExec ex;
  team_begin(ex, G, G.members, sh.data());
  while (w.st.active) team_trial(ex, G, G.members, *prm, sh.data());
  bool ok = true;
  for (int k = 0; k < w.frames && ok; ++k) ok = team_pose_storable(G.T + 12 * (size_t)k);
  lins_pose_graph_result& r = out->solve;
  r.cost_before = w.st.cost0, r.cost_after = w.st.cost, r.max_increment = w.st.max_inc;
  r.iterations = w.st.iterations, r.reason = w.st.reason, r.status = ok ? LINS_OK : LINS_E_INPUT;
  if (!ok) return LINS_OK;
  for (int i = 0; i < n_members; ++i) {
    Graph& g = graphs[i]->g;
    const size_t off = 12 * (size_t)w.mt[i].off;
    g.store_solution(G.T + off, G.D + off);
    if (i > 0) g.store_rebased(G.T + off, G.T + off);  // the solved root is the prior now
  }
  return LINS_OK;
}

int lins_host_team_graph_linearize(int n_members, lins_host_pose_graph* const* graphs, const double* root_variance, int n_factors,
                                   const lins_team_factor* factors, const double* poses, double* r_factor, double* M, double* r_root,
                                   double* H_root, double* g_root) {
  TeamWork w;
  if (int rc = team_check(n_members, graphs, root_variance, n_factors, factors, false, w)) return rc;
  std::vector<double> own;
  if (!poses) {
    for (int i = 0; i < n_members; ++i) own.insert(own.end(), graphs[i]->g.T.begin(), graphs[i]->g.T.end());
    poses = own.data();
  }
  for (int i = 0; i < n_factors; ++i) {
    const TeamFactorIn& f = w.fin[i];
    double r[6], Ml[36];
    lin_loop(f.Z, poses + 12 * (size_t)(w.mt[f.mb].off + f.id_b), poses + 12 * (size_t)(w.mt[f.ma].off + f.id_a), 0, r, Ml);
    if (r_factor) std::memcpy(r_factor + 6 * (size_t)i, r, sizeof r);
    if (M) std::memcpy(M + 36 * (size_t)i, Ml, sizeof Ml);
  }
  for (int i = 1; i < n_members; ++i) {
    double r[6], H[36], g[6];
    lin_odometry_var(&graphs[i]->g.Z[0], poses + 12 * (size_t)w.mt[i].off, w.mt[i].var, r, H, g);
    if (r_root) std::memcpy(r_root + 6 * (size_t)(i - 1), r, sizeof r);
    if (H_root) std::memcpy(H_root + 36 * (size_t)(i - 1), H, sizeof H);
    if (g_root) std::memcpy(g_root + 6 * (size_t)(i - 1), g, sizeof g);
  }
  return LINS_OK;
}

}  // extern "C"
