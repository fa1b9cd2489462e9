// pose_graph.h — the pose graph's solve as ONE text for the device and the CPU (include/lins_map.h lins_pose_graph_*,
// DESIGN.md §5.3 "Pose graph"), on the scalar definitions of pose_graph_math.h.
//
// A problem is worked on by kThreads lanes in phases: within a phase lane t does fn(t), and no lane reads what another
// lane writes in the same phase; between phases everything written is visible.  The device runs a phase as
// `fn(threadIdx.x); __syncthreads();` (one workgroup per problem, pose_graph_kernels.hip), the CPU as
// `for t in 0 .. kThreads - 1: fn(t)` (host/pose_graph.cpp).  Every sum has one order, written here, that depends on the
// problem alone — so a problem's result bits do not depend on the batch it is in, and host and device differ only where
// libm does.
//
// Unknowns: the increments D_k = T_{k-1}^-1 T_k, k = 1 .. N - 1; T_0 is the prior's measurement, exactly.  Perturbation
// D_k <- retract(D_k, d_k).  Odometry factor k depends on d_k alone (6 x 6 blocks A_k = D_k + lambda I, gradient g_k);
// loop l on (T_b, T_a) = (latest, closest) has E = Z^-1 T_b^-1 T_a and the rows J_{l,k} = M_l Ad(T_k) for lo < k <= hi,
// M_l = s J_E Ad(T_a^-1), s = -1 when b > a, +1 otherwise.  With mu = S^-1 (r_L - J A^-1 g), S = W^-1 + J A^-1 J^T, the
// step is d = -A^-1 (g + J^T mu).
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include "../../include/lins_host.h"  // lins_map.h: lins_pose_graph_params / _result
#include "pose_graph_math.h"

namespace lins_pg {

constexpr int kThreads = 256;     // lanes of a problem (the workgroup)
constexpr int kPrefixBlock = 32;  // consecutive increments composed left to right in one block of the prefix product
constexpr int kChunks = 7;        // a span's sum over frames: kChunks sums over consecutive frames, added left to right
constexpr int kShared = 400;      // doubles of phase scratch (LDS on the device)

struct LoopRec {
  double Z[12];
  double var;
  int latest, closest;
  double M[36], r[6], w[6];
};

struct State {
  double lambda, cost, cost0, max_inc;
  int iterations, reason, active, status;
};

struct Prob {       // one slot's graph where the phases work on it (device or host memory)
  int n_frames, n_loops;
  int slot, pad;
  double* Z;        // [F][12]  Z[0]: the prior; Z[k]: odometry factor k
  double* D;        // [F][12]  the increments ([0] unused)
  double* Dt;       //          the trial increments
  double* I;        //          the prefix inside each block
  double* T;        //          absolute poses of D
  double* Tt;       //          absolute poses of Dt
  double* Q;        // [F / kPrefixBlock + 2][12]  the prefix of blocks
  double* B;        // [F][36]  A_k^-1
  double* c;        // [F][6]   A_k^-1 g_k
  double* P;        // [F][36]  Ad(T_k) A_k^-1 Ad(T_k)^T
  double* q;        // [F][6]   Ad(T_k) A_k^-1 g_k
  LoopRec* loops;   // [max_loops]
  double* S;        // [6 L][6 L]
  double* y;        // [3][6 L]  right-hand side, forward solution, mu
  State* st;
};

LINS_HD void default_params(lins_pose_graph_params* p) {
  p->max_iterations = 50, p->reserved = 0;
  p->rel_cost_decrease = 1e-12, p->max_increment = 1e-11;
  p->lambda_initial = 1e-5, p->lambda_up = 10.0, p->lambda_down = 0.1;
}

// what a solve accepts as parameters (else LINS_E_ARG)
inline bool params_ok(const lins_pose_graph_params* p) {
  return p && p->max_iterations >= 1 && std::isfinite(p->rel_cost_decrease) && std::isfinite(p->max_increment) && p->lambda_initial > 0.0 &&
         std::isfinite(p->lambda_initial) && p->lambda_up > 1.0 && std::isfinite(p->lambda_up) && p->lambda_down > 0.0 && p->lambda_down <= 1.0;
}
// The most loops a slot may be sized for.  The loops' core is dense: S takes 288 L^2 bytes a slot (1.2 MB at 64), and a
// trial runs 3 L (L + 1) / 2 phases for S and 24 L for its Cholesky and the two triangular solves, each behind a barrier
// (6 240 + 1 536 at 64).  The reference closes a loop at most once per detection pass; tens of loops a slot is the design.
constexpr int kMaxLoops = 64;

LINS_HD void state_init(State& s, const lins_pose_graph_params& prm) {
  s.lambda = prm.lambda_initial, s.cost = 0.0, s.cost0 = 0.0, s.max_inc = 0.0;
  s.iterations = 0, s.reason = LINS_PG_NONE, s.active = 1, s.status = 0;
}

// odometry factor: residual r of E = Z^-1 D, Hessian block H = J^T Sigma^-1 J, gradient g = J^T Sigma^-1 r
LINS_HD void lin_odometry(const double* Z, const double* D, double* r, double* H, double* g) {
  double E[12], J[36];
  between(Z, D, E);
  residual_of(E, r);
  residual_jacobian(E, r, J);
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 6; ++j) {
      double s = J[i] * (J[j] / odo_variance(0));
      for (int p = 1; p < 6; ++p) s += J[6 * p + i] * (J[6 * p + j] / odo_variance(p));
      H[6 * i + j] = s;
    }
    double s = J[i] * (r[0] / odo_variance(0));
    for (int p = 1; p < 6; ++p) s += J[6 * p + i] * (r[p] / odo_variance(p));
    g[i] = s;
  }
}
LINS_HD double cost_odometry(const double* Z, const double* D) {
  double E[12], r[6];
  between(Z, D, E);
  residual_of(E, r);
  double s = r[0] * r[0] / odo_variance(0);
  for (int p = 1; p < 6; ++p) s += r[p] * r[p] / odo_variance(p);
  return s;
}
// loop factor on (Tb, Ta): residual and M = s J_E Ad(Ta^-1)
LINS_HD void loop_residual(const double* Z, const double* Tb, const double* Ta, double* E, double* r) {
  double X[12];
  between(Tb, Ta, X);
  between(Z, X, E);
  residual_of(E, r);
}
LINS_HD void lin_loop(const double* Z, const double* Tb, const double* Ta, int b_after_a, double* r, double* M) {
  double E[12], J[36], Ti[12], A[36];
  loop_residual(Z, Tb, Ta, E, r);
  residual_jacobian(E, r, J);
  inverse(Ta, Ti);
  adjoint(Ti, A);
  mul66(J, A, M);
  if (b_after_a)
    for (int i = 0; i < 36; ++i) M[i] = -M[i];
}
LINS_HD double cost_loop(const LoopRec& L, const double* T) {
  double E[12], r[6];
  loop_residual(L.Z, T + 12 * L.latest, T + 12 * L.closest, E, r);
  double s = r[0] * r[0];
  for (int p = 1; p < 6; ++p) s += r[p] * r[p];
  return s / L.var;
}
LINS_HD int loop_lo(const LoopRec& L) { return L.latest < L.closest ? L.latest : L.closest; }
LINS_HD int loop_hi(const LoopRec& L) { return L.latest < L.closest ? L.closest : L.latest; }
// chunk c of the n frames first .. first + n - 1
LINS_HD int chunk_begin(int first, int n, int c) { return first + (int)(((long long)c * n) / kChunks); }

// T_k = T_0 D_1 ... D_k in the association order of the contract: blocks of kPrefixBlock increments left to right, the
// block totals left to right, T_k = (prefix of blocks) (prefix inside the block)
template <class Exec>
LINS_HD void phase_poses(const Exec& ex, const Prob& P, const double* D, double* T) {
  const int n = P.n_frames - 1, nb = (n + kPrefixBlock - 1) / kPrefixBlock;
  ex([&](int t) {
    for (int b = t; b < nb; b += kThreads) {
      const int k0 = b * kPrefixBlock + 1, k1 = (k0 + kPrefixBlock <= n + 1) ? k0 + kPrefixBlock : n + 1;
      pose_copy(D + 12 * k0, P.I + 12 * k0);
      for (int k = k0 + 1; k < k1; ++k) compose(P.I + 12 * (k - 1), D + 12 * k, P.I + 12 * k);
    }
  });
  ex([&](int t) {
    if (t == 0) {
      pose_copy(P.Z, P.Q);
      for (int b = 0; b < nb; ++b) {
        const int last = ((b + 1) * kPrefixBlock < n) ? (b + 1) * kPrefixBlock : n;
        compose(P.Q + 12 * b, P.I + 12 * last, P.Q + 12 * (b + 1));
      }
    }
  });
  ex([&](int t) {
    for (int k = t; k <= n; k += kThreads) {
      if (k == 0) pose_copy(P.Z, T);
      else compose(P.Q + 12 * ((k - 1) / kPrefixBlock), P.I + 12 * k, T + 12 * k);
    }
  });
}

// C = 1/2 sum r^T Sigma^-1 r -> sh[256]: lane t adds its frames t + 1, t + 1 + kThreads ... in order; lane 0 adds the
// lanes in order, then the loops in order
template <class Exec>
LINS_HD void phase_cost(const Exec& ex, const Prob& P, const double* D, const double* T, double* sh) {
  ex([&](int t) {
    double s = 0.0;
    for (int k = t + 1; k < P.n_frames; k += kThreads) s += cost_odometry(P.Z + 12 * k, D + 12 * k);
    sh[t] = s;
  });
  ex([&](int t) {
    if (t == 0) {
      double s = sh[0];
      for (int i = 1; i < kThreads; ++i) s += sh[i];
      for (int l = 0; l < P.n_loops; ++l) s += cost_loop(P.loops[l], T);
      sh[256] = 0.5 * s;
    }
  });
}

// the first launch of a solve: the poses and the cost of the graph as it stands
template <class Exec>
LINS_HD void solve_begin(const Exec& ex, const Prob& P, double* sh) {
  phase_poses(ex, P, P.D, P.T);
  phase_cost(ex, P, P.D, P.T, sh);
  ex([&](int t) {
    if (t == 0) P.st->cost = sh[256], P.st->cost0 = sh[256];
  });
}

// one Levenberg-Marquardt trial.  Returns nothing: the state says whether the problem goes on.
template <class Exec>
LINS_HD void solve_trial(const Exec& ex, const Prob& P, const lins_pose_graph_params& prm, double* sh) {
  const int N = P.n_frames, L = P.n_loops, m = 6 * L;
  const double lambda = P.st->lambda;
  // 1 the odometry blocks, and the loops' residuals and M
  ex([&](int t) {
    for (int k = t + 1; k < N; k += kThreads) {
      double r[6], H[36], g[6], A[36], X[36];
      lin_odometry(P.Z + 12 * k, P.D + 12 * k, r, H, g);
      for (int i = 0; i < 6; ++i) H[7 * i] += lambda;
      double* B = P.B + 36 * k;
      chol6_inverse(H, B);
      mul6v(B, g, P.c + 6 * k);
      adjoint(P.T + 12 * k, A);
      mul66(A, B, X);
      mul66t(X, A, P.P + 36 * k);
      mul6v(A, P.c + 6 * k, P.q + 6 * k);
    }
    for (int l = t; l < L; l += kThreads) {
      LoopRec& R = P.loops[l];
      lin_loop(R.Z, P.T + 12 * R.latest, P.T + 12 * R.closest, R.latest > R.closest, R.r, R.M);
    }
  });
  // 2 S = W^-1 + J A^-1 J^T block by block (the upper triangle, mirrored), and the right-hand side r_L - J A^-1 g
  for (int l = 0; l < L; ++l)
    for (int l2 = l; l2 < L; ++l2) {
      const LoopRec &Ra = P.loops[l], &Rb = P.loops[l2];
      const int lo = loop_lo(Ra) > loop_lo(Rb) ? loop_lo(Ra) : loop_lo(Rb), hi = loop_hi(Ra) < loop_hi(Rb) ? loop_hi(Ra) : loop_hi(Rb);
      const int n = hi > lo ? hi - lo : 0;  // frames lo + 1 .. hi
      ex([&](int t) {
        if (t < 36 * kChunks) {
          const int e = t % 36, c = t / 36;
          double s = 0.0;
          for (int k = chunk_begin(lo + 1, n, c); k < chunk_begin(lo + 1, n, c + 1); ++k) s += P.P[36 * k + e];
          sh[36 * c + e] = s;
        }
        if (l2 == l && t < 6 * kChunks) {
          const int e = t % 6, c = t / 6;
          double s = 0.0;
          for (int k = chunk_begin(lo + 1, n, c); k < chunk_begin(lo + 1, n, c + 1); ++k) s += P.q[6 * k + e];
          sh[300 + 6 * c + e] = s;
        }
      });
      ex([&](int t) {
        if (t < 36) {
          double s = sh[t];
          for (int c = 1; c < kChunks; ++c) s += sh[36 * c + t];
          sh[256 + t] = s;
        }
        if (l2 == l && t < 6) {
          double s = sh[300 + t];
          for (int c = 1; c < kChunks; ++c) s += sh[300 + 6 * c + t];
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
          P.S[(size_t)(6 * l + i) * m + 6 * l2 + j] = v;
          if (l2 != l) P.S[(size_t)(6 * l2 + j) * m + 6 * l + i] = v;
        }
        if (l2 == l && t < 6) {
          double s = Ra.M[6 * t] * sh[292];
          for (int p = 1; p < 6; ++p) s += Ra.M[6 * t + p] * sh[292 + p];
          P.y[6 * l + t] = Ra.r[t] - s;
        }
      });
    }
  // 3 Cholesky of S in place (right-looking, column by column), then L z = y and L^T mu = z
  double *y = P.y, *z = P.y + m, *mu = P.y + 2 * m;
  for (int j = 0; j < m; ++j) {
    ex([&](int t) {
      const double d = sqrt(P.S[(size_t)j * m + j]);
      for (int i = j + 1 + t; i < m; i += kThreads) P.S[(size_t)i * m + j] = P.S[(size_t)i * m + j] / d;
    });
    ex([&](int t) {
      const int w = m - j - 1;
      for (int x = t; x < w * w; x += kThreads) {
        const int i = j + 1 + x / w, k = j + 1 + x % w;
        if (k <= i) P.S[(size_t)i * m + k] -= P.S[(size_t)i * m + j] * P.S[(size_t)k * m + j];
      }
      if (t == 0) P.S[(size_t)j * m + j] = sqrt(P.S[(size_t)j * m + j]);
    });
  }
  for (int j = 0; j < m; ++j)
    ex([&](int t) {
      const double x = y[j] / P.S[(size_t)j * m + j];
      for (int i = j + 1 + t; i < m; i += kThreads) y[i] -= P.S[(size_t)i * m + j] * x;
      if (t == 0) z[j] = x;
    });
  for (int j = m - 1; j >= 0; --j)
    ex([&](int t) {
      const double x = z[j] / P.S[(size_t)j * m + j];
      for (int i = t; i < j; i += kThreads) z[i] -= P.S[(size_t)j * m + i] * x;
      if (t == 0) mu[j] = x;
    });
  // 4 w_l = M_l^T mu_l
  ex([&](int t) {
    for (int l = t; l < L; l += kThreads) mul6tv(P.loops[l].M, mu + 6 * l, P.loops[l].w);
  });
  // 5 the step d_k = -(c_k + B_k Ad(T_k)^T sum_{l over k} w_l) and the trial increments
  ex([&](int t) {
    double big = 0.0;
    for (int k = t + 1; k < N; k += kThreads) {
      double v[6] = {0, 0, 0, 0, 0, 0}, A[36], u[6], h[6], d[6];
      for (int l = 0; l < L; ++l) {
        const LoopRec& R = P.loops[l];
        if (loop_lo(R) < k && k <= loop_hi(R))
          for (int i = 0; i < 6; ++i) v[i] += R.w[i];
      }
      adjoint(P.T + 12 * k, A);
      mul6tv(A, v, u);
      mul6v(P.B + 36 * k, u, h);
      for (int i = 0; i < 6; ++i) {
        d[i] = -(P.c[6 * k + i] + h[i]);
        big = fabs(d[i]) > big ? fabs(d[i]) : big;
      }
      retract(P.D + 12 * k, d, P.Dt + 12 * k);
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
  phase_poses(ex, P, P.Dt, P.Tt);
  phase_cost(ex, P, P.Dt, P.Tt, sh);
  // 7 accept or reject, lambda, the stop rule
  ex([&](int t) {
    if (t == 0) {
      State& s = *P.st;
      const double c0 = s.cost, c1 = sh[256], inc = sh[257], dec = c0 - c1;
      // A trial whose cost differs from the estimate's by no more than the stop rule's bound is not told apart from no
      // change by its cost: the solve takes this last step — it is the damped Gauss-Newton step, small where the cost is
      // flat — and stops.  (Taking it only on c1 < c0 would let the rounding of two costs decide the last step,
      // differently on the host and on the device.)
      const int flat = fabs(dec) <= prm.rel_cost_decrease * c0;
      const int accept = flat || c1 < c0;
      s.max_inc = inc;
      s.iterations += 1;
      if (accept) s.cost = c1, s.lambda = lambda * prm.lambda_down;
      else s.lambda = lambda * prm.lambda_up;
      // (a rejected step's size says nothing: it shrinks with every rejection's lambda)
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
        pose_copy(P.Dt + 12 * k, P.D + 12 * k);
        pose_copy(P.Tt + 12 * k, P.T + 12 * k);
      }
  });
}

// ---- the graph's bookkeeping on the host, shared by both libraries: validation, the measurements formed once in f64 when
// a frame or a loop is added, and the six floats lins_pose_graph_poses hands back.  A refused call changes nothing. ----
struct Graph {
  int max_frames = 0, max_loops = 0;
  std::vector<double> Z;     // [N][12]  Z[0] the prior, Z[k] = pose(last)^-1 pose(aft)
  std::vector<double> T;     // [N][12]  the estimate in f64: pose(aft) as pushed, the solved pose after a solve with loops
  std::vector<float> held;   // [N][6]   the estimate as six floats in the mapping node's order: the bits pushed, or the
                             //          solved pose rounded once
  std::vector<double> D;     // [N][12]  the increments of the estimate (the CPU library's; the device library keeps them on the device)
  std::vector<LoopRec> loops;
  int n_frames() const { return (int)(held.size() / 6); }

  static bool finite6(const float* p) {
    for (int i = 0; i < 6; ++i)
      if (!std::isfinite(p[i])) return false;
    return true;
  }
  int push(const float* last6, const float* aft6) {
    if (!aft6 || (n_frames() && !last6)) return LINS_E_ARG;
    if (!finite6(aft6) || (n_frames() && !finite6(last6))) return LINS_E_INPUT;
    if (n_frames() >= max_frames) return LINS_E_CAPACITY;
    double A[12], B[12], Zk[12];
    pose_from6(aft6, A);
    if (n_frames() == 0) {
      pose_copy(A, Zk);
    } else {
      pose_from6(last6, B);
      between(B, A, Zk);
    }
    Z.insert(Z.end(), Zk, Zk + 12);
    D.insert(D.end(), Zk, Zk + 12);
    T.insert(T.end(), A, A + 12);
    held.insert(held.end(), aft6, aft6 + 6);
    return n_frames() - 1;
  }
  int add_loop(int latest, int closest, const lins_key_pose* pf, double fitness) {
    if (!pf || latest < 0 || closest < 0 || latest >= n_frames() || closest >= n_frames() || latest == closest) return LINS_E_ARG;
    const double var = (double)(float)fitness;
    const float f[6] = {pf->x, pf->y, pf->z, pf->roll, pf->pitch, pf->yaw};
    if (!finite6(f) || !std::isfinite(var) || !(var > 0.0)) return LINS_E_INPUT;
    if ((int)loops.size() >= max_loops) return LINS_E_CAPACITY;
    LoopRec R{};
    double From[12], To[12];
    pose_from_lidar(pf->x, pf->y, pf->z, pf->roll, pf->pitch, pf->yaw, From);
    pose_from6(&held[6 * (size_t)closest], To);
    between(From, To, R.Z);
    R.var = var, R.latest = latest, R.closest = closest;
    loops.push_back(R);
    return (int)loops.size() - 1;
  }
  // the solved absolute poses of frames 1 .. N - 1 become the estimate (frame 0 is the prior: it keeps its bits)
  void store_solution(const double* Tsolved, const double* Dsolved) {
    for (int k = 1; k < n_frames(); ++k) {
      if (Dsolved) pose_copy(Dsolved + 12 * k, &D[12 * (size_t)k]);
      pose_copy(Tsolved + 12 * k, &T[12 * (size_t)k]);
      pose_to6(Tsolved + 12 * k, &held[6 * (size_t)k]);
    }
  }
  // ---- rebase (include/lins_team.h lins_pose_graph_rebase_batch): the whole history moves into another frame by the prior
  // alone, Z[0] <- X Z[0] — the unknowns are increments and the prior holds exactly, so no factor's residual moves.
  // the prior a rebase by Xg (a pose in the graph's axes) gives: ONE compose
  void rebased_prior(const double* Xg, double* Z0) const { compose(Xg, &Z[0], Z0); }
  // the new prior with the poses phase_poses formed from it, every frame's — frame 0 is the prior and moves with it
  void store_rebased(const double* Z0, const double* Tnew) {
    pose_copy(Z0, &Z[0]), pose_copy(Z0, &D[0]);
    for (int k = 0; k < n_frames(); ++k) {
      pose_copy(Tnew + 12 * k, &T[12 * (size_t)k]);
      pose_to6(Tnew + 12 * k, &held[6 * (size_t)k]);
    }
  }
  // PointTypePose as LM:1721-1733 assigns it
  void key_pose(int id, lins_key_pose* out) const {
    const float* p = &held[6 * (size_t)id];
    out->x = p[3], out->y = p[4], out->z = p[5], out->roll = p[0], out->pitch = p[1], out->yaw = p[2];
  }
};

// ---- the X of a rebase: 4 x 4 row-major f64 in the archive's axes — what lins_rendezvous_step returns, the axes of
// lins_key_pose's x, y, z and of the clouds.  The graph's axes are those permuted (pose_from6: t = (z, x, y) of the key
// pose), so X in the graph's axes is X's entries moved, exactly.
// what a rebase accepts (else LINS_E_INPUT): sixteen finite entries, a last row of 0 0 0 1, |R^T R - I| <= 1e-9 in every
// entry and det R > 0
inline bool rebase_x_ok(const double* X) {
  if (!X) return false;
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(X[i])) return false;
  if (X[12] != 0.0 || X[13] != 0.0 || X[14] != 0.0 || X[15] != 1.0) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double s = (X[i] * X[j] + X[4 + i] * X[4 + j]) + X[8 + i] * X[8 + j];
      if (!(std::fabs(s - (i == j ? 1.0 : 0.0)) <= 1e-9)) return false;
    }
  const double det = X[0] * (X[5] * X[10] - X[6] * X[9]) - X[1] * (X[4] * X[10] - X[6] * X[8]) + X[2] * (X[4] * X[9] - X[5] * X[8]);
  return det > 0.0;
}
inline void rebase_x_pose(const double* X, double* Xg) {
  const int archive_of[3] = {2, 0, 1};  // graph axis -> the archive axis that is the same direction
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Xg[3 * i + j] = X[4 * archive_of[i] + archive_of[j]];
    Xg[9 + i] = X[4 * archive_of[i] + 3];
  }
}

}  // namespace lins_pg
