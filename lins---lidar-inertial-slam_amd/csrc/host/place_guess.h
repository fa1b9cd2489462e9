// place_guess.h — the start transform of an ICP from a place match (lins_host_place_guess), ONE text compiled into both
// libraries: host/place.cpp exports it, lins_loop_step_place (lins_loop_step_capi.hip) forms its guesses with it.
// T0 = M_c R_up(shift 2 pi / kNS) M_q^-1 in f64, row-major; M: a stored key pose as the archive's assembly applies it
// (loop_step.h key_pose_matrix).  Host code: f64 libm, no contraction.
#pragma once
#include <cmath>

#include "loop_step.h"
#include "place_math.h"

namespace lins_place {

inline void mul4(const double* A, const double* B, double* C) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) C[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j] + A[4 * i + 3] * B[12 + j];
}

// shift in [0, kNS), up_axis in [0, 2]: checked by the caller
inline void guess(const lins_key_pose& pose_q, const lins_key_pose& pose_c, int shift, int up_axis, double* T0) {
  double Mq[16], Mc[16], Mi[16], R[16], A[16];
  lins_loop::key_pose_matrix(pose_q, Mq), lins_loop::key_pose_matrix(pose_c, Mc);  // (loop_step.h: the conversion behind pose_from)
  // M_q^-1 = (R^T, -R^T t)
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Mi[4 * i + j] = Mq[4 * j + i];
    Mi[4 * i + 3] = -(Mq[i] * Mq[3] + Mq[4 + i] * Mq[7] + Mq[8 + i] * Mq[11]);
  }
  Mi[12] = Mi[13] = Mi[14] = 0.0, Mi[15] = 1.0;
  const double th = shift * (6.283185307179586476925 / kNS), c = std::cos(th), s = std::sin(th);
  const int a = (up_axis + 1) % 3, b = (up_axis + 2) % 3;
  for (int i = 0; i < 16; ++i) R[i] = (i % 5 == 0) ? 1.0 : 0.0;
  R[4 * a + a] = c, R[4 * a + b] = -s, R[4 * b + a] = s, R[4 * b + b] = c;
  mul4(Mc, R, A), mul4(A, Mi, T0);
}

// The same formula for lins_rendezvous_step (include/lins_team.h), with the sine and the cosine taken from ONE sincos
// call.  guess() above leaves the choice to the compiler: g++ fuses its two calls into sincos, clang keeps sin and cos,
// and glibc's sincos and sin differ by an ulp at some angles (shift 8: 0x1.7c7d7a833bec2p-1 against ...ec1p-1) — the two
// libraries then disagree in the last bit of T0.  guess() keeps its text and each library's bits; a chain that has to
// match a step bit for bit across the two libraries takes this one.  The key poses' matrices have the same choice in them.
// (loop_step.h key_pose_matrix and its get_transformation<double>, with the three angles' sines and cosines by sincos)
inline void team_pose_matrix(const lins_key_pose& p, double* M) {
  double cr, sr, cp, sp, cy, sy;
  ::sincos((double)p.yaw, &sr, &cr), ::sincos((double)p.roll, &sp, &cp), ::sincos((double)p.pitch, &sy, &cy);
  const double L[16] = {cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, p.z, sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr, p.x,
                        -sp,     cp * sr,                cp * cr,                p.y, 0.0,     0.0,                    0.0,                    1.0};
  const int lidar_of[3] = {1, 2, 0};  // camera axis -> the lidar axis that is the same direction
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) M[4 * i + j] = L[4 * lidar_of[i] + lidar_of[j]];
    M[4 * i + 3] = L[4 * lidar_of[i] + 3];
  }
  M[12] = M[13] = M[14] = 0.0, M[15] = 1.0;
}
inline void guess_team(const lins_key_pose& pose_q, const lins_key_pose& pose_c, int shift, int up_axis, double* T0) {
  double Mq[16], Mc[16], Mi[16], R[16], A[16];
  team_pose_matrix(pose_q, Mq), team_pose_matrix(pose_c, Mc);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Mi[4 * i + j] = Mq[4 * j + i];
    Mi[4 * i + 3] = -(Mq[i] * Mq[3] + Mq[4 + i] * Mq[7] + Mq[8 + i] * Mq[11]);
  }
  Mi[12] = Mi[13] = Mi[14] = 0.0, Mi[15] = 1.0;
  const double th = shift * (6.283185307179586476925 / kNS);
  double c, s;
  ::sincos(th, &s, &c);
  const int a = (up_axis + 1) % 3, b = (up_axis + 2) % 3;
  for (int i = 0; i < 16; ++i) R[i] = (i % 5 == 0) ? 1.0 : 0.0;
  R[4 * a + a] = c, R[4 * a + b] = -s, R[4 * b + a] = s, R[4 * b + b] = c;
  mul4(Mc, R, A), mul4(A, Mi, T0);
}

}  // namespace lins_place
