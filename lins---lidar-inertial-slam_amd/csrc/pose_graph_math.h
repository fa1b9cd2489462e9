// pose_graph_math.h — the scalar definition of the pose graph's arithmetic (include/lins_map.h lins_pose_graph_*,
// DESIGN.md §5.3 "Pose graph"), host + device: six floats <-> pose, compose / inverse, Exp / Log on SO(3), the residual
// of a between-factor with its Jacobian, the adjoint, the 6 x 6 Cholesky.  pose_graph.h builds the solve from it;
// pose_graph_kernels.hip runs that on the device, host/pose_graph.cpp on the CPU: one text, so the two differ only
// where libm does (sin, cos, atan2, asin; sqrt and + - x / are correctly rounded on both, contraction is off).
//
// A pose is double[12]: R row-major in [0, 9), t in [9, 12).  A twist is (omega, v), rotation first.
#pragma once
#include <math.h>

#include "lins_math.h"  // LINS_HD

#ifdef __HIPCC__
#define PG_UNROLL _Pragma("unroll")
#else
#define PG_UNROLL
#endif

namespace lins_pg {

// R = Rz(z) Ry(y) Rx(x) — gtsam's Rot3::RzRyRx(x, y, z) — from angles already promoted to double
LINS_HD void rot_zyx(double x, double y, double z, double* R) {
  const double cx = cos(x), sx = sin(x), cy = cos(y), sy = sin(y), cz = cos(z), sz = sin(z);
  R[0] = cz * cy, R[1] = cz * sy * sx - sz * cx, R[2] = cz * sy * cx + sz * sx;
  R[3] = sz * cy, R[4] = sz * sy * sx + cz * cx, R[5] = sz * sy * cx - cz * sx;
  R[6] = -sy, R[7] = cy * sx, R[8] = cy * cx;
}
// the mapping node's six floats (pitch, yaw, roll, y, z, x) -> pose: Rot3::RzRyRx(p[2], p[0], p[1]), Point3(p[5], p[3], p[4])
LINS_HD void pose_from6(const float* p, double* T) {
  rot_zyx((double)p[2], (double)p[0], (double)p[1], T);
  T[9] = (double)p[5], T[10] = (double)p[3], T[11] = (double)p[4];
}
// a pose as lins_host_loop_pose_from returns it (LM:1166-1168): Rot3::RzRyRx(roll, pitch, yaw), Point3(x, y, z)
LINS_HD void pose_from_lidar(float x, float y, float z, float roll, float pitch, float yaw, double* T) {
  rot_zyx((double)roll, (double)pitch, (double)yaw, T);
  T[9] = (double)x, T[10] = (double)y, T[11] = (double)z;
}
// pose -> six floats: x = atan2(R21, R22), y = asin(-R20), z = atan2(R10, R00), each rounded once to f32 (|y| at pi / 2
// is outside the contract)
LINS_HD void pose_to6(const double* T, float* p) {
  p[2] = (float)atan2(T[7], T[8]);
  p[0] = (float)asin(-T[6]);
  p[1] = (float)atan2(T[3], T[0]);
  p[5] = (float)T[9], p[3] = (float)T[10], p[4] = (float)T[11];
}

LINS_HD void pose_copy(const double* A, double* C) {
  PG_UNROLL
  for (int i = 0; i < 12; ++i) C[i] = A[i];
}
// C = A B (C distinct from A and B); every sum left to right
LINS_HD void compose(const double* A, const double* B, double* C) {
  PG_UNROLL
  for (int i = 0; i < 3; ++i) {
    PG_UNROLL
    for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
    C[9 + i] = ((A[3 * i] * B[9] + A[3 * i + 1] * B[10]) + A[3 * i + 2] * B[11]) + A[9 + i];
  }
}
// C = A^-1 = (R^T, -R^T t)
LINS_HD void inverse(const double* A, double* C) {
  PG_UNROLL
  for (int i = 0; i < 3; ++i) {
    PG_UNROLL
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * j + i];
    C[9 + i] = -((A[i] * A[9] + A[3 + i] * A[10]) + A[6 + i] * A[11]);
  }
}
// C = A^-1 B
LINS_HD void between(const double* A, const double* B, double* C) {
  double Ai[12];
  inverse(A, Ai);
  compose(Ai, B, C);
}

// Exp on SO(3), Rodrigues: R = I + a [w]x + b [w]x^2, a = sin(th) / th, b = 2 sin^2(th / 2) / th^2; the small-angle branch
// th^2 < 1e-16 takes a = 1 - th^2 / 6, b = 1 / 2 - th^2 / 24 (exact to double there).
LINS_HD void so3_exp(const double* w, double* R) {
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  double a, b;
  if (t2 < 1e-16) {
    a = 1.0 - t2 / 6.0, b = 0.5 - t2 / 24.0;
  } else {
    const double th = sqrt(t2), sh = sin(0.5 * th);
    a = sin(th) / th, b = 2.0 * sh * sh / t2;
  }
  const double xx = w[0] * w[0], yy = w[1] * w[1], zz = w[2] * w[2], xy = w[0] * w[1], xz = w[0] * w[2], yz = w[1] * w[2];
  R[0] = 1.0 - b * (yy + zz), R[1] = b * xy - a * w[2], R[2] = b * xz + a * w[1];
  R[3] = b * xy + a * w[2], R[4] = 1.0 - b * (xx + zz), R[5] = b * yz - a * w[0];
  R[6] = b * xz - a * w[1], R[7] = b * yz + a * w[0], R[8] = 1.0 - b * (xx + yy);
}
// Log on SO(3): u = vee(R - R^T) / 2 = sin(th) axis, c = (trace - 1) / 2, th = atan2(|u|, c), w = (th / |u|) u; the
// small-angle branch |u|^2 < 1e-16 takes th / |u| = 1 + |u|^2 / 6.  Rotations by pi (|u| = 0 with c < 0) are outside the
// contract: a residual's rotation is small.
LINS_HD void so3_log(const double* R, double* w) {
  const double u0 = 0.5 * (R[7] - R[5]), u1 = 0.5 * (R[2] - R[6]), u2 = 0.5 * (R[3] - R[1]);
  const double s2 = (u0 * u0 + u1 * u1) + u2 * u2;
  double f;
  if (s2 < 1e-16) {
    f = 1.0 + s2 / 6.0;
  } else {
    const double s = sqrt(s2), c = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    f = atan2(s, c) / s;
  }
  w[0] = f * u0, w[1] = f * u1, w[2] = f * u2;
}
// The inverse right Jacobian of SO(3): Log(R Exp(d)) = w + Jri(w) d + O(d^2), Jri = I + [w]x / 2 + c [w]x^2 with
// c = 1 / th^2 - (1 + cos th) / (2 th sin th); the small-angle branch th^2 < 1e-6 takes c = 1 / 12 + th^2 / 720 (the next
// term, th^4 / 30240, is below 4e-17 there; the closed form's cancellation costs c about 1e-16 / th^2 <= 1e-10 above it,
// which enters the matrix times th^2).
LINS_HD void so3_jri(const double* w, double* J) {
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  double c;
  if (t2 < 1e-6) {
    c = 1.0 / 12.0 + t2 / 720.0;
  } else {
    const double th = sqrt(t2);
    c = 1.0 / t2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
  }
  const double xx = w[0] * w[0], yy = w[1] * w[1], zz = w[2] * w[2], xy = w[0] * w[1], xz = w[0] * w[2], yz = w[1] * w[2];
  J[0] = 1.0 - c * (yy + zz), J[1] = c * xy - 0.5 * w[2], J[2] = c * xz + 0.5 * w[1];
  J[3] = c * xy + 0.5 * w[2], J[4] = 1.0 - c * (xx + zz), J[5] = c * yz - 0.5 * w[0];
  J[6] = c * xz - 0.5 * w[1], J[7] = c * yz + 0.5 * w[0], J[8] = 1.0 - c * (xx + yy);
}

// the retraction: C = (R Exp(omega), t + R v)
LINS_HD void retract(const double* T, const double* d, double* C) {
  double E[12];
  so3_exp(d, E);
  E[9] = d[3], E[10] = d[4], E[11] = d[5];
  compose(T, E, C);
}
// the residual of E = Z^-1 Ti^-1 Tj in the chart: r = (Log R_E, t_E)
LINS_HD void residual_of(const double* E, double* r) {
  so3_log(E, r);
  r[3] = E[9], r[4] = E[10], r[5] = E[11];
}
// its Jacobian with respect to a right twist on E, E (I + eta^): blockdiag(Jri(r_omega), R_E), 6 x 6 row-major
LINS_HD void residual_jacobian(const double* E, const double* r, double* J) {
  double Q[9];
  so3_jri(r, Q);
  PG_UNROLL
  for (int i = 0; i < 36; ++i) J[i] = 0.0;
  PG_UNROLL
  for (int i = 0; i < 3; ++i) {
    PG_UNROLL
    for (int j = 0; j < 3; ++j) J[6 * i + j] = Q[3 * i + j], J[6 * (i + 3) + 3 + j] = E[3 * i + j];
  }
}
// Ad(T) for twists (omega, v): [[R, 0], [[t]x R, R]], 6 x 6 row-major.  Ad(A B) = Ad(A) Ad(B).
LINS_HD void adjoint(const double* T, double* A) {
  const double* t = T + 9;
  PG_UNROLL
  for (int j = 0; j < 3; ++j) {
    const double r0 = T[j], r1 = T[3 + j], r2 = T[6 + j];
    A[j] = r0, A[6 + j] = r1, A[12 + j] = r2;
    A[3 + j] = 0.0, A[9 + j] = 0.0, A[15 + j] = 0.0;
    A[18 + j] = t[1] * r2 - t[2] * r1, A[24 + j] = t[2] * r0 - t[0] * r2, A[30 + j] = t[0] * r1 - t[1] * r0;
    A[21 + j] = r0, A[27 + j] = r1, A[33 + j] = r2;
  }
}
// C = A B, C = A B^T, y = A x, y = A^T x for 6 x 6 row-major; every sum left to right over the inner index
LINS_HD void mul66(const double* A, const double* B, double* C) {
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      double s = A[6 * i] * B[j];
      for (int p = 1; p < 6; ++p) s += A[6 * i + p] * B[6 * p + j];
      C[6 * i + j] = s;
    }
}
LINS_HD void mul66t(const double* A, const double* B, double* C) {
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      double s = A[6 * i] * B[6 * j];
      for (int p = 1; p < 6; ++p) s += A[6 * i + p] * B[6 * j + p];
      C[6 * i + j] = s;
    }
}
LINS_HD void mul6v(const double* A, const double* x, double* y) {
  for (int i = 0; i < 6; ++i) {
    double s = A[6 * i] * x[0];
    for (int p = 1; p < 6; ++p) s += A[6 * i + p] * x[p];
    y[i] = s;
  }
}
LINS_HD void mul6tv(const double* A, const double* x, double* y) {
  for (int i = 0; i < 6; ++i) {
    double s = A[i] * x[0];
    for (int p = 1; p < 6; ++p) s += A[6 * p + i] * x[p];
    y[i] = s;
  }
}
// 6 x 6 Cholesky A = L L^T (lower, row by row) and B = A^-1 through it; A symmetric positive definite (D + lambda I)
LINS_HD void chol6_inverse(const double* A, double* B) {
  double L[36];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = A[6 * i + j];
      for (int p = 0; p < j; ++p) s -= L[6 * i + p] * L[6 * j + p];
      L[6 * i + j] = i == j ? sqrt(s) : s / L[6 * j + j];
    }
  for (int c = 0; c < 6; ++c) {  // column c of the inverse: L y = e_c, L^T x = y
    double y[6];
    for (int i = 0; i < 6; ++i) {
      double s = i == c ? 1.0 : 0.0;
      for (int p = 0; p < i; ++p) s -= L[6 * i + p] * y[p];
      y[i] = s / L[6 * i + i];
    }
    for (int i = 5; i >= 0; --i) {
      double s = y[i];
      for (int p = i + 1; p < 6; ++p) s -= L[6 * p + i] * y[p];
      y[i] = s / L[6 * i + i];
    }
    for (int i = 0; i < 6; ++i) B[6 * i + c] = y[i];
  }
}

// the noise of the prior and of every odometry factor (LM:383-385): variances, rotation first
LINS_HD double odo_variance(int i) { return (i == 3 || i == 4) ? 1e-8 : 1e-6; }

}  // namespace lins_pg
