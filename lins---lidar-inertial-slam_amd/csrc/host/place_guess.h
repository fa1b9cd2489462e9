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

}  // namespace lins_place
