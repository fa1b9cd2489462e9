// loop_icp_math.h — the scalar definition of the loop-closure ICP's arithmetic (include/lins_map.h, DESIGN.md §5.3
// "Loop-closure ICP"), host + device: the f32 move and distance, the order of the f64 sums, the Kabsch fit with its
// 3 x 3 SVD (one-sided cyclic Jacobi, fixed sweep count: only + - x / sqrt), the composition and the stop rule.
// loop_icp_kernels.hip runs it on the device, host/loop_icp.cpp on the CPU: one text, so the two cannot drift apart.
#pragma once
#include <float.h>
#include <math.h>

#include "../../include/lins_host.h"  // lins_map.h: the parameters; lins_loop_icp_state
#include "lins_math.h"  // LINS_HD

#ifdef __HIPCC__
#define LICP_UNROLL _Pragma("unroll")
#else
#define LICP_UNROLL
#endif

namespace lins_licp {

constexpr int kTile = 32;   // source points per tile of the sums
constexpr int kGroup = 8;   // consecutive points under one fixed-shape tree
constexpr int kSums = 17;   // 0: count  1-3: S x'  4-6: S g  7-15: S x'_i g_j (3 i + j)  16: S d
constexpr int kSweeps = 10; // Jacobi sweeps of the 3 x 3 SVD (f64 converges in 5-6; the count is part of the contract)
// H counts as of rank < 2 when sigma2 <= kRankFloor sigma1, kRankFloor = c u with u = 2^-53 and c = 2^14.  Exactly collinear
// points leave a second singular value of rounding noise in the f64 raw-moment H: over lines of at least 1 m within 100 m of
// the origin, formed in plain f64 and decomposed by LAPACK, at most 1.7e3 u sigma1 (tests/loop_fit_cases.py
// collinear_floor); c is 8 x that, rounded up to a power of two.  Part of the contract.
constexpr double kRankFloor = 16384.0 * 1.1102230246251565e-16;

LINS_HD void default_params(lins_loop_icp_params* p) {
  p->transformation_epsilon = 1e-6, p->fitness_epsilon = 1e-6, p->rel_mse = 1e-5, p->rotation_threshold = 0.99999;
  p->max_corr_dist = 100.f, p->max_iterations = 100, p->min_correspondences = 3, p->reserved = 0;
}

// step 1: M = the upper three rows of T rounded to f32
LINS_HD void make_move(const double* T, float* M) {
  LICP_UNROLL
  for (int i = 0; i < 12; ++i) M[i] = (float)T[i];
}
LINS_HD void move_point(const float* M, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
  oy = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
  oz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
}
// step 2: the project's squared distance
LINS_HD float sqdist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}
// one correspondence's terms of the sums
LINS_HD void corr_terms(float sx, float sy, float sz, float gx, float gy, float gz, float d, double* v) {
  const double s[3] = {(double)sx, (double)sy, (double)sz}, g[3] = {(double)gx, (double)gy, (double)gz};
  v[0] = 1.0;
  LICP_UNROLL
  for (int i = 0; i < 3; ++i) v[1 + i] = s[i], v[4 + i] = g[i];
  LICP_UNROLL
  for (int i = 0; i < 3; ++i)
    LICP_UNROLL
    for (int j = 0; j < 3; ++j) v[7 + 3 * i + j] = s[i] * g[j];
  v[16] = (double)d;
}
// the fixed tree over eight consecutive points (what three xor-butterfly steps over lanes 32, 16, 8 apart compute)
LINS_HD double tree8(const double* q) { return ((q[0] + q[4]) + (q[2] + q[6])) + ((q[1] + q[5]) + (q[3] + q[7])); }

// U S V^T = H by one-sided Jacobi; returns R = V diag(1, 1, det(V U^T)) U^T.  The columns are ordered by falling
// singular value and the third column of U is u0 x u1 — the same R as with the SVD's own third column, and defined for
// a rank-2 H; an H of rank < 2 (collinear or coincident points: the rotation is not determined; sigma2 <= kRankFloor sigma1)
// gives the identity.
LINS_HD void kabsch_rotation(const double* H, double* R) {
  double A[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  LICP_UNROLL
  for (int i = 0; i < 9; ++i) A[i] = H[i];
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    LICP_UNROLL
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      double alpha = 0, beta = 0, gamma = 0;
      LICP_UNROLL
      for (int i = 0; i < 3; ++i) alpha += A[3 * i + p] * A[3 * i + p], beta += A[3 * i + q] * A[3 * i + q], gamma += A[3 * i + p] * A[3 * i + q];
      if (gamma == 0.0) continue;
      const double zeta = (beta - alpha) / (2.0 * gamma);
      const double az = zeta < 0 ? -zeta : zeta;
      const double t = (zeta < 0 ? -1.0 : 1.0) / (az + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
      LICP_UNROLL
      for (int i = 0; i < 3; ++i) {
        const double ap = A[3 * i + p], aq = A[3 * i + q];
        A[3 * i + p] = c * ap - s * aq, A[3 * i + q] = s * ap + c * aq;
        const double vp = V[3 * i + p], vq = V[3 * i + q];
        V[3 * i + p] = c * vp - s * vq, V[3 * i + q] = s * vp + c * vq;
      }
    }
  }
  double n2[3];
  LICP_UNROLL
  for (int j = 0; j < 3; ++j) n2[j] = (A[j] * A[j] + A[3 + j] * A[3 + j]) + A[6 + j] * A[6 + j];
  // columns by falling norm (three compare-and-swaps of whole columns of A and V; constant indices throughout)
  LICP_UNROLL
  for (int k = 0; k < 3; ++k) {
    const int a = k == 1 ? 1 : 0, b = k == 1 ? 2 : 1;
    if (n2[b] > n2[a]) {
      const double tn = n2[a];
      n2[a] = n2[b], n2[b] = tn;
      LICP_UNROLL
      for (int i = 0; i < 3; ++i) {
        const double ta = A[3 * i + a], tv = V[3 * i + a];
        A[3 * i + a] = A[3 * i + b], A[3 * i + b] = ta, V[3 * i + a] = V[3 * i + b], V[3 * i + b] = tv;
      }
    }
  }
  LICP_UNROLL
  for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  if (!(n2[1] > (kRankFloor * kRankFloor) * n2[0])) return;  // (n2 = sigma^2; false for 0 > 0 and for a NaN too)
  const double s0 = sqrt(n2[0]), s1 = sqrt(n2[1]);
  double U[9];  // U = [u0 u1 u0 x u1]; W = V, its columns in the same order
  const double* W = V;
  LICP_UNROLL
  for (int i = 0; i < 3; ++i) U[3 * i] = A[3 * i] / s0, U[3 * i + 1] = A[3 * i + 1] / s1;
  U[2] = U[3] * U[7] - U[6] * U[4], U[5] = U[6] * U[1] - U[0] * U[7], U[8] = U[0] * U[4] - U[3] * U[1];
  // det U = +1 by construction, so det(V U^T) has the sign of det W
  const double detw = W[0] * (W[4] * W[8] - W[5] * W[7]) - W[1] * (W[3] * W[8] - W[5] * W[6]) + W[2] * (W[3] * W[7] - W[4] * W[6]);
  const double dd = detw < 0 ? -1.0 : 1.0;
  LICP_UNROLL
  for (int i = 0; i < 3; ++i)
    LICP_UNROLL
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (W[3 * i] * U[3 * j] + W[3 * i + 1] * U[3 * j + 1]) + dd * (W[3 * i + 2] * U[3 * j + 2]);
}

// step 4 from the sums: Delta (row-major 4 x 4) mapping the moved source points onto their targets.  H is formed from the
// raw second moments, H = S x' g^T - n mu_s mu_g^T, so that one pass over the points gives everything.
LINS_HD void fit_from_sums(const double* sums, double* D) {
  const double n = sums[0];
  double ms[3], mg[3], H[9], R[9];
  LICP_UNROLL
  for (int i = 0; i < 3; ++i) ms[i] = sums[1 + i] / n, mg[i] = sums[4 + i] / n;
  LICP_UNROLL
  for (int i = 0; i < 3; ++i)
    LICP_UNROLL
    for (int j = 0; j < 3; ++j) H[3 * i + j] = sums[7 + 3 * i + j] - n * (ms[i] * mg[j]);
  kabsch_rotation(H, R);
  LICP_UNROLL
  for (int i = 0; i < 3; ++i) {
    LICP_UNROLL
    for (int j = 0; j < 3; ++j) D[4 * i + j] = R[3 * i + j];
    D[4 * i + 3] = mg[i] - ((R[3 * i] * ms[0] + R[3 * i + 1] * ms[1]) + R[3 * i + 2] * ms[2]);
  }
  D[12] = D[13] = D[14] = 0.0, D[15] = 1.0;
}

LINS_HD void compose(const double* D, const double* T, double* out) {  // out = D T
  LICP_UNROLL
  for (int i = 0; i < 4; ++i)
    LICP_UNROLL
    for (int j = 0; j < 4; ++j) out[4 * i + j] = ((D[4 * i] * T[j] + D[4 * i + 1] * T[4 + j]) + D[4 * i + 2] * T[8 + j]) + D[4 * i + 3] * T[12 + j];
}

struct State {  // one problem between two rounds
  double T[16];
  double mse_prev, mse, fitness;
  float M[12];
  int iterations, converged, reason, n_corr, n_fitness, active;
  unsigned far;
  int pad;
};

LINS_HD void state_init(State& s) {
  LICP_UNROLL
  for (int i = 0; i < 16; ++i) s.T[i] = (i % 5 == 0) ? 1.0 : 0.0;
  make_move(s.T, s.M);
  s.mse_prev = DBL_MAX, s.mse = 0.0, s.fitness = DBL_MAX;
  s.iterations = 0, s.converged = 0, s.reason = LINS_ICP_NONE, s.n_corr = 0, s.n_fitness = 0, s.active = 1, s.far = 0, s.pad = 0;
}

// steps 3-6 of round k = s.iterations from the round's sums; D (may be read when the round fitted) and the four stop
// quantities q = {0.5 (trace R - 1), |t|^2, |mse - mse_prev|, |mse - mse_prev| / mse_prev} for the trace
LINS_HD void step_from_sums(const lins_loop_icp_params& prm, const double* sums, State& s, double* D, double* q) {
  s.n_corr = (int)sums[0];
  if (s.n_corr < prm.min_correspondences) {
    s.converged = 0, s.reason = LINS_ICP_NO_CORRESPONDENCES, s.active = 0;
    return;
  }
  fit_from_sums(sums, D);
  double Tn[16];
  compose(D, s.T, Tn);
  LICP_UNROLL
  for (int i = 0; i < 16; ++i) s.T[i] = Tn[i];
  make_move(s.T, s.M);
  s.iterations += 1;
  const double mse = sums[16] / sums[0];
  const double rot = 0.5 * (((D[0] + D[5]) + D[10]) - 1.0), t2 = (D[3] * D[3] + D[7] * D[7]) + D[11] * D[11];
  const double diff = mse - s.mse_prev, ad = diff < 0 ? -diff : diff, rel = ad / s.mse_prev;
  q[0] = rot, q[1] = t2, q[2] = ad, q[3] = rel;
  int reason = LINS_ICP_NONE;
  if (s.iterations >= prm.max_iterations) reason = LINS_ICP_ITERATIONS;
  else if (rot >= prm.rotation_threshold && t2 <= prm.transformation_epsilon) reason = LINS_ICP_TRANSFORM;
  else if (ad < prm.fitness_epsilon) reason = LINS_ICP_ABS_MSE;
  else if (rel < prm.rel_mse) reason = LINS_ICP_REL_MSE;
  s.mse = mse, s.mse_prev = mse;
  if (reason != LINS_ICP_NONE) s.converged = 1, s.reason = reason, s.active = 0;
}

LINS_HD void fitness_from_sums(const double* sums, State& s) {
  s.n_fitness = (int)sums[0];
  s.fitness = s.n_fitness > 0 ? sums[16] / sums[0] : DBL_MAX;
}

// the state as the test entries of the step take and return it (include/lins_host.h lins_loop_icp_state)
inline void state_from_public(const lins_loop_icp_state& p, State& s) {
  state_init(s);
  for (int i = 0; i < 16; ++i) s.T[i] = p.T[i];
  make_move(s.T, s.M);
  s.mse_prev = p.mse_prev, s.mse = p.mse, s.fitness = p.fitness;
  s.iterations = p.iterations, s.converged = p.converged, s.reason = p.reason, s.n_corr = p.n_corr, s.n_fitness = p.n_fitness, s.active = p.active;
}
inline void state_to_public(const State& s, lins_loop_icp_state& p) {
  for (int i = 0; i < 16; ++i) p.T[i] = s.T[i];
  for (int i = 0; i < 12; ++i) p.move[i] = s.M[i];
  p.mse_prev = s.mse_prev, p.mse = s.mse, p.fitness = s.fitness;
  p.iterations = s.iterations, p.converged = s.converged, p.reason = s.reason, p.n_corr = s.n_corr, p.n_fitness = s.n_fitness, p.active = s.active;
}

}  // namespace lins_licp
