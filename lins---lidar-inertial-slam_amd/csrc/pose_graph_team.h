// pose_graph_team.h — the team graph's solve as ONE text for the device and the CPU (include/lins_team.h
// lins_team_graph_solve, DESIGN.md §5.3 "Team graph"), in the phase form of pose_graph.h and on its scalar pieces: the
// odometry and loop factors, the costs, the 6 x 6 inverse, the adjoint, the retraction and the prefix product are CALLED
// from pose_graph.h / pose_graph_math.h, not restated.  A group of one member and no team factor runs, operation for
// operation, what solve_begin / solve_trial run for that member.
//
// A group is the concatenation of its members' chains: member m owns the rows off_m .. off_m + n_m - 1 of every per-frame
// array.  Row off_m + j, j >= 1, is the member's increment D_j as in the single solve.  Row off_m is the member's root: for
// member 0, the anchor, the prior Z[0], exact and no unknown; for every other member an unknown T_0 — D[off_m] holds it,
// Z[off_m] holds the prior's measurement, its factor is E = Z^-1 T_0 under the member's six root variances, and it
// retracts like an increment (an increment relative to the identity).  So the unknowns of a group are the rows 1 ..
// n_frames - 1, each with a 6 x 6 block of its own, as in the single solve.
//
// A loop l has a support of at most two signed intervals of rows (TeamSpan), its rows being sigma_l(k) M_l Ad(T_k):
//   a member's own loop   one interval (lo, hi] inside the member, sigma = +1, the sign folded into M_l as today;
//   a team factor on ((b, id_b), (a, id_a)), E = Z^-1 T_b^-1 T_a, M = J_E Ad(T_a^-1) with no sign folded in:
//                         chain a's unknowns up to id_a with sigma = +1, chain b's up to id_b with sigma = -1, the roots
//                         included where they are unknowns; the two intervals are listed in group order.
// S_{l,l'} = W^-1 delta + M_l (sum_k sigma_l(k) sigma_l'(k) P_k) M_l'^T over the intersection of the two supports: at most
// one interval per chain, so at most two.  The order of that sum: the intervals in group order, each as kChunks chunk
// sums over consecutive rows added left to right, each total under its sign, then the totals left to right.  The loops'
// right-hand side sums q_k over the loop's own intervals the same way.
#pragma once
#include "pose_graph.h"

namespace lins_pg {

constexpr int kTeamMaxMembers = 32;  // members of a group: the member table lies in LDS beside the phase scratch
// doubles of phase scratch: pose_graph.h's layout for the first interval ([0, 252) chunk sums, [256, 292) the 6 x 6 sum,
// [292, 298) the q sum, [300, 342) its chunk sums; [256, 259) cost, largest step and accept flag at the trial's end), and
// for the second interval [400, 652) chunk sums, [652, 694) q's chunk sums
constexpr int kTeamShared = 696;

struct TeamMember {
  int off, n;       // first row and frames
  int qoff, first;  // first row of the member's prefix of blocks; first unknown row (off + 1 for the anchor, off otherwise)
  double var[6];    // the root factor's variances, rotation first (unused for the anchor)
};

struct TeamSpan {
  int lo[2], hi[2];  // rows lo < k <= hi
  int sg[2];         // +1, -1; 0: no such interval
  int team, pad;     // 1: a team factor (M without a sign); 0: a member's own loop
};

struct TeamProb {  // one group where the phases work on it (device or host memory)
  int n_members, n_frames, n_loops, pad;
  const TeamMember* members;
  double *Z, *D, *Dt, *I, *T, *Tt, *Q, *B, *c, *P, *q;  // as Prob's, over the concatenated rows; Q: the members' prefixes back to back
  LoopRec* loops;    // the members' loops in member order, then the team factors; latest / closest are rows
  TeamSpan* spans;
  double* S;
  double* y;
  State* st;
};

struct TeamCopy {  // one member's rows (m*) against its group's rows (g*), for the device's gather and scatter
  double *mZ, *mD, *mT;
  double *gZ, *gD, *gT;
  int n, root;     // frames; 1: a non-anchor member (its solved root becomes its prior)
  int store, pad;  // scatter: 1 where the group's solution is stored
};

// the supports of the loops (host bookkeeping, both libraries)
inline TeamSpan team_span_own(const LoopRec& R) {
  TeamSpan s{};
  s.lo[0] = loop_lo(R), s.hi[0] = loop_hi(R), s.sg[0] = 1;
  return s;
}
// a team factor between row rb of member mb and row ra of member ma (mb != ma)
inline TeamSpan team_span_factor(const TeamMember* mt, int mb, int rb, int ma, int ra) {
  TeamSpan s{};
  const int ia = ma < mb ? 0 : 1, ib = 1 - ia;
  s.lo[ia] = mt[ma].first - 1, s.hi[ia] = ra, s.sg[ia] = 1;
  s.lo[ib] = mt[mb].first - 1, s.hi[ib] = rb, s.sg[ib] = -1;
  s.team = 1;
  return s;
}

// the root factor: lin_odometry / cost_odometry with the six variances handed in
LINS_HD void lin_odometry_var(const double* Z, const double* D, const double* var, double* r, double* H, double* g) {
  double E[12], J[36];
  between(Z, D, E);
  residual_of(E, r);
  residual_jacobian(E, r, J);
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 6; ++j) {
      double s = J[i] * (J[j] / var[0]);
      for (int p = 1; p < 6; ++p) s += J[6 * p + i] * (J[6 * p + j] / var[p]);
      H[6 * i + j] = s;
    }
    double s = J[i] * (r[0] / var[0]);
    for (int p = 1; p < 6; ++p) s += J[6 * p + i] * (r[p] / var[p]);
    g[i] = s;
  }
}
LINS_HD double cost_odometry_var(const double* Z, const double* D, const double* var) {
  double E[12], r[6];
  between(Z, D, E);
  residual_of(E, r);
  double s = r[0] * r[0] / var[0];
  for (int p = 1; p < 6; ++p) s += r[p] * r[p] / var[p];
  return s;
}

// the member whose root row k is, 0 where k is no unknown root
LINS_HD int team_root_of(const TeamMember* mt, int nm, int k) {
  for (int m = 1; m < nm; ++m)
    if (mt[m].off == k) return m;
  return 0;
}

// the intersection of two supports: n[i] rows from lo[i] + 1 on under the sign sg[i], in group order; of[i]: the interval
// of the first support it lies in
struct TeamCut {
  int lo[2], n[2], sg[2], of[2];
};
LINS_HD void team_cut(const TeamSpan& a, const TeamSpan& b, TeamCut& c) {
  int cnt = 0;
  for (int i = 0; i < 2; ++i) c.lo[i] = 0, c.n[i] = 0, c.sg[i] = 1, c.of[i] = 0;
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) {
      if (a.sg[i] == 0 || b.sg[j] == 0) continue;
      const int lo = a.lo[i] > b.lo[j] ? a.lo[i] : b.lo[j], hi = a.hi[i] < b.hi[j] ? a.hi[i] : b.hi[j];
      if (hi > lo && cnt < 2) c.lo[cnt] = lo, c.n[cnt] = hi - lo, c.sg[cnt] = a.sg[i] * b.sg[j], c.of[cnt] = i, ++cnt;
    }
  if (cnt == 2 && c.lo[1] < c.lo[0]) {
    int x;
    x = c.lo[0], c.lo[0] = c.lo[1], c.lo[1] = x;
    x = c.n[0], c.n[0] = c.n[1], c.n[1] = x;
    x = c.sg[0], c.sg[0] = c.sg[1], c.sg[1] = x;
    x = c.of[0], c.of[0] = c.of[1], c.of[1] = x;
  }
}
// sigma_l(k), 0 outside the support
LINS_HD int team_sign(const TeamSpan& s, int k) {
  if (s.sg[0] != 0 && s.lo[0] < k && k <= s.hi[0]) return s.sg[0];
  if (s.sg[1] != 0 && s.lo[1] < k && k <= s.hi[1]) return s.sg[1];
  return 0;
}

// every member's poses by phase_poses itself, member after member: blocks of kPrefixBlock inside a member, never across
// two.  A non-anchor member's root is the row D[off] (the unknown), the anchor's the prior Z[0].
template <class Exec>
LINS_HD void team_phase_poses(const Exec& ex, const TeamProb& G, const TeamMember* mt, double* D, double* T) {
  for (int m = 0; m < G.n_members; ++m) {
    Prob p{};
    p.n_frames = mt[m].n;
    p.Z = (m == 0 ? G.Z : D) + 12 * (size_t)mt[m].off;
    p.I = G.I + 12 * (size_t)mt[m].off;
    p.Q = G.Q + 12 * (size_t)mt[m].qoff;
    phase_poses(ex, p, D + 12 * (size_t)mt[m].off, T + 12 * (size_t)mt[m].off);
  }
}

// phase_cost's order over the rows of the group: lane t adds its rows t + 1, t + 1 + kThreads ... in order (a root row
// under its member's variances), lane 0 adds the lanes in order, then the loops in order
template <class Exec>
LINS_HD void team_phase_cost(const Exec& ex, const TeamProb& G, const TeamMember* mt, const double* D, const double* T, double* sh) {
  ex([&](int t) {
    double s = 0.0;
    for (int k = t + 1; k < G.n_frames; k += kThreads) {
      const int root = team_root_of(mt, G.n_members, k);
      if (root) s += cost_odometry_var(G.Z + 12 * (size_t)k, D + 12 * (size_t)k, mt[root].var);
      else s += cost_odometry(G.Z + 12 * (size_t)k, D + 12 * (size_t)k);
    }
    sh[t] = s;
  });
  ex([&](int t) {
    if (t == 0) {
      double s = sh[0];
      for (int i = 1; i < kThreads; ++i) s += sh[i];
      for (int l = 0; l < G.n_loops; ++l) s += cost_loop(G.loops[l], T);
      sh[256] = 0.5 * s;
    }
  });
}

template <class Exec>
LINS_HD void team_begin(const Exec& ex, const TeamProb& G, const TeamMember* mt, double* sh) {
  team_phase_poses(ex, G, mt, G.D, G.T);
  team_phase_cost(ex, G, mt, G.D, G.T, sh);
  ex([&](int t) {
    if (t == 0) G.st->cost = sh[256], G.st->cost0 = sh[256];
  });
}

// one Levenberg-Marquardt trial: solve_trial's steps over the group's rows
template <class Exec>
LINS_HD void team_trial(const Exec& ex, const TeamProb& G, const TeamMember* mt, const lins_pose_graph_params& prm, double* sh) {
  const int N = G.n_frames, L = G.n_loops, m = 6 * L;
  const double lambda = G.st->lambda;
  // 1 the blocks of the unknowns, and the loops' residuals and M
  ex([&](int t) {
    for (int k = t + 1; k < N; k += kThreads) {
      double r[6], H[36], g[6], A[36], X[36];
      const int root = team_root_of(mt, G.n_members, k);
      if (root) lin_odometry_var(G.Z + 12 * (size_t)k, G.D + 12 * (size_t)k, mt[root].var, r, H, g);
      else lin_odometry(G.Z + 12 * (size_t)k, G.D + 12 * (size_t)k, r, H, g);
      for (int i = 0; i < 6; ++i) H[7 * i] += lambda;
      double* B = G.B + 36 * (size_t)k;
      chol6_inverse(H, B);
      mul6v(B, g, G.c + 6 * (size_t)k);
      adjoint(G.T + 12 * (size_t)k, A);
      mul66(A, B, X);
      mul66t(X, A, G.P + 36 * (size_t)k);
      mul6v(A, G.c + 6 * (size_t)k, G.q + 6 * (size_t)k);
    }
    for (int l = t; l < L; l += kThreads) {
      LoopRec& R = G.loops[l];
      lin_loop(R.Z, G.T + 12 * (size_t)R.latest, G.T + 12 * (size_t)R.closest, !G.spans[l].team && R.latest > R.closest, R.r, R.M);
    }
  });
  // 2 S and the right-hand side, block by block
  for (int l = 0; l < L; ++l)
    for (int l2 = l; l2 < L; ++l2) {
      const LoopRec &Ra = G.loops[l], &Rb = G.loops[l2];
      TeamCut cut;
      team_cut(G.spans[l], G.spans[l2], cut);
      const int qs0 = G.spans[l].sg[cut.of[0]], qs1 = G.spans[l].sg[cut.of[1]];  // the signs of q's sums (l2 == l)
      ex([&](int t) {
        for (int v = 0; v < 2; ++v) {
          if (v == 1 && cut.n[1] == 0) break;
          const int first = cut.lo[v] + 1, n = cut.n[v];
          double* ps = sh + 400 * v;
          double* qsum = v == 0 ? sh + 300 : sh + 652;
          if (t < 36 * kChunks) {
            const int e = t % 36, c = t / 36;
            double s = 0.0;
            for (int k = chunk_begin(first, n, c); k < chunk_begin(first, n, c + 1); ++k) s += G.P[36 * (size_t)k + e];
            ps[36 * c + e] = s;
          }
          if (l2 == l && t < 6 * kChunks) {
            const int e = t % 6, c = t / 6;
            double s = 0.0;
            for (int k = chunk_begin(first, n, c); k < chunk_begin(first, n, c + 1); ++k) s += G.q[6 * (size_t)k + e];
            qsum[6 * c + e] = s;
          }
        }
      });
      ex([&](int t) {
        if (t < 36) {
          double s = sh[t];
          for (int c = 1; c < kChunks; ++c) s += sh[36 * c + t];
          s = cut.sg[0] > 0 ? s : -s;
          if (cut.n[1] > 0) {
            double u = sh[400 + t];
            for (int c = 1; c < kChunks; ++c) u += sh[400 + 36 * c + t];
            s += cut.sg[1] > 0 ? u : -u;
          }
          sh[256 + t] = s;
        }
        if (l2 == l && t < 6) {
          double s = sh[300 + t];
          for (int c = 1; c < kChunks; ++c) s += sh[300 + 6 * c + t];
          s = qs0 > 0 ? s : -s;
          if (cut.n[1] > 0) {
            double u = sh[652 + t];
            for (int c = 1; c < kChunks; ++c) u += sh[652 + 6 * c + t];
            s += qs1 > 0 ? u : -u;
          }
          sh[292 + t] = s;
        }
      });
      ex([&](int t) {
        if (t < 36) {
          const int i = t / 6, j = t % 6;
          double v = 0.0;
          for (int p = 0; p < 6; ++p) {
            double u = sh[256 + 6 * p] * Rb.M[6 * j];
            for (int q = 1; q < 6; ++q) u += sh[256 + 6 * p + q] * Rb.M[6 * j + q];
            v += Ra.M[6 * i + p] * u;
          }
          if (l2 == l && i == j) v += Ra.var;
          G.S[(size_t)(6 * l + i) * m + 6 * l2 + j] = v;
          if (l2 != l) G.S[(size_t)(6 * l2 + j) * m + 6 * l + i] = v;
        }
        if (l2 == l && t < 6) {
          double s = Ra.M[6 * t] * sh[292];
          for (int p = 1; p < 6; ++p) s += Ra.M[6 * t + p] * sh[292 + p];
          G.y[6 * l + t] = Ra.r[t] - s;
        }
      });
    }
  // 3 Cholesky of S in place (right-looking, column by column), then L z = y and L^T mu = z
  double *y = G.y, *z = G.y + m, *mu = G.y + 2 * m;
  for (int j = 0; j < m; ++j) {
    ex([&](int t) {
      const double d = sqrt(G.S[(size_t)j * m + j]);
      for (int i = j + 1 + t; i < m; i += kThreads) G.S[(size_t)i * m + j] = G.S[(size_t)i * m + j] / d;
    });
    ex([&](int t) {
      const int w = m - j - 1;
      for (int x = t; x < w * w; x += kThreads) {
        const int i = j + 1 + x / w, k = j + 1 + x % w;
        if (k <= i) G.S[(size_t)i * m + k] -= G.S[(size_t)i * m + j] * G.S[(size_t)k * m + j];
      }
      if (t == 0) G.S[(size_t)j * m + j] = sqrt(G.S[(size_t)j * m + j]);
    });
  }
  for (int j = 0; j < m; ++j)
    ex([&](int t) {
      const double x = y[j] / G.S[(size_t)j * m + j];
      for (int i = j + 1 + t; i < m; i += kThreads) y[i] -= G.S[(size_t)i * m + j] * x;
      if (t == 0) z[j] = x;
    });
  for (int j = m - 1; j >= 0; --j)
    ex([&](int t) {
      const double x = z[j] / G.S[(size_t)j * m + j];
      for (int i = t; i < j; i += kThreads) z[i] -= G.S[(size_t)j * m + i] * x;
      if (t == 0) mu[j] = x;
    });
  // 4 w_l = M_l^T mu_l
  ex([&](int t) {
    for (int l = t; l < L; l += kThreads) mul6tv(G.loops[l].M, mu + 6 * l, G.loops[l].w);
  });
  // 5 the step d_k = -(c_k + B_k Ad(T_k)^T sum_{l over k} sigma_l(k) w_l) and the trial rows
  ex([&](int t) {
    double big = 0.0;
    for (int k = t + 1; k < N; k += kThreads) {
      double v[6] = {0, 0, 0, 0, 0, 0}, A[36], u[6], h[6], d[6];
      for (int l = 0; l < L; ++l) {
        const LoopRec& R = G.loops[l];
        const int sg = team_sign(G.spans[l], k);
        if (sg > 0)
          for (int i = 0; i < 6; ++i) v[i] += R.w[i];
        else if (sg < 0)
          for (int i = 0; i < 6; ++i) v[i] -= R.w[i];
      }
      adjoint(G.T + 12 * (size_t)k, A);
      mul6tv(A, v, u);
      mul6v(G.B + 36 * (size_t)k, u, h);
      for (int i = 0; i < 6; ++i) {
        d[i] = -(G.c[6 * (size_t)k + i] + h[i]);
        big = fabs(d[i]) > big ? fabs(d[i]) : big;
      }
      retract(G.D + 12 * (size_t)k, d, G.Dt + 12 * (size_t)k);
    }
    sh[t] = big;
  });
  ex([&](int t) {
    if (t == 0) {
      double big = sh[0];
      for (int i = 1; i < kThreads; ++i) big = sh[i] > big ? sh[i] : big;
      sh[257] = big;
    }
  });
  // 6 the trial's poses and cost
  team_phase_poses(ex, G, mt, G.Dt, G.Tt);
  team_phase_cost(ex, G, mt, G.Dt, G.Tt, sh);
  // 7 accept or reject, lambda, the stop rule: the single solve's (pose_graph.h solve_trial has the reasons)
  ex([&](int t) {
    if (t == 0) {
      State& s = *G.st;
      const double c0 = s.cost, c1 = sh[256], inc = sh[257], dec = c0 - c1;
      const int flat = fabs(dec) <= prm.rel_cost_decrease * c0;
      const int accept = flat || c1 < c0;
      s.max_inc = inc;
      s.iterations += 1;
      if (accept) s.cost = c1, s.lambda = lambda * prm.lambda_down;
      else s.lambda = lambda * prm.lambda_up;
      if (flat) s.reason = LINS_PG_REL_COST;
      else if (accept && inc <= prm.max_increment) s.reason = LINS_PG_INCREMENT;
      else if (s.iterations >= prm.max_iterations) s.reason = LINS_PG_ITERATIONS;
      if (s.reason != LINS_PG_NONE) s.active = 0;
      sh[258] = accept ? 1.0 : 0.0;
    }
  });
  ex([&](int t) {
    if (sh[258] != 0.0)
      for (int k = t + 1; k < N; k += kThreads) {
        pose_copy(G.Dt + 12 * (size_t)k, G.D + 12 * (size_t)k);
        pose_copy(G.Tt + 12 * (size_t)k, G.T + 12 * (size_t)k);
      }
  });
}

// ---- the group's bookkeeping on the host, shared by both libraries ----
struct TeamFactorIn {  // a team factor with its slots resolved to members of the group
  int mb, id_b, ma, id_a;
  const double* Z;
  double var;
};
// what a factor's measurement and a variance must be (else LINS_E_INPUT): finite, a rotation by rebase_x_ok's bound
inline bool team_z_ok(const double* Z) {
  double X[16];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) X[4 * i + j] = Z[3 * i + j];
    X[4 * i + 3] = Z[9 + i];
  }
  X[12] = 0.0, X[13] = 0.0, X[14] = 0.0, X[15] = 1.0;
  return rebase_x_ok(X);
}
inline bool team_var_ok(double v) { return std::isfinite(v) && v > 0.0; }

// the member table of n members with counts[m] frames; root_variance: 6 per member (member 0's unread); returns the rows
inline int team_members(int n, const int* counts, const double* const* root_variance, TeamMember* mt, int* q_rows) {
  int off = 0, qoff = 0;
  for (int m = 0; m < n; ++m) {
    mt[m].off = off, mt[m].n = counts[m], mt[m].qoff = qoff, mt[m].first = m == 0 ? off + 1 : off;
    for (int i = 0; i < 6; ++i) mt[m].var[i] = (m && root_variance[m]) ? root_variance[m][i] : odo_variance(i);
    off += counts[m], qoff += counts[m] / kPrefixBlock + 2;
  }
  if (q_rows) *q_rows = qoff;
  return off;
}
// the group's loop records and supports: the members' loops with their ids moved to rows, then the factors
inline void team_loops(int n, const TeamMember* mt, const std::vector<LoopRec>* const* own, int n_factors, const TeamFactorIn* f,
                       std::vector<LoopRec>& loops, std::vector<TeamSpan>& spans) {
  loops.clear(), spans.clear();
  for (int m = 0; m < n; ++m)
    for (const LoopRec& R0 : *own[m]) {
      LoopRec R{};
      pose_copy(R0.Z, R.Z);
      R.var = R0.var, R.latest = R0.latest + mt[m].off, R.closest = R0.closest + mt[m].off;
      loops.push_back(R), spans.push_back(team_span_own(R));
    }
  for (int i = 0; i < n_factors; ++i) {
    LoopRec R{};
    pose_copy(f[i].Z, R.Z);
    R.var = f[i].var, R.latest = mt[f[i].mb].off + f[i].id_b, R.closest = mt[f[i].ma].off + f[i].id_a;
    loops.push_back(R), spans.push_back(team_span_factor(mt, f[i].mb, R.latest, f[i].ma, R.closest));
  }
}
// Z = (Xg T_b)^-1 T_a; Xg null: the identity
inline void team_factor_z(const double* Tb, const double* Ta, const double* Xg, double* Z) {
  if (Xg) {
    double XT[12];
    compose(Xg, Tb, XT);
    between(XT, Ta, Z);
  } else {
    between(Tb, Ta, Z);
  }
}
// whether the solved rows can be stored: finite, inside the archive's bound once rounded to the six floats
inline bool team_pose_storable(const double* T) {
  float p[6];
  pose_to6(T, p);
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(p[i])) return false;
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(T[i])) return false;
  return std::fabs(p[3]) <= 1e6f && std::fabs(p[4]) <= 1e6f && std::fabs(p[5]) <= 1e6f;
}

}  // namespace lins_pg
