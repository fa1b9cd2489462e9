// filter_math.h — the scalar definition of what the streams' device-resident filter does around an update, host +
// device (DESIGN.md §5.3 "Device-resident filter"): one IMU sample's state propagation with the non-zero blocks of F_t
// and G_t (KF:125-169), and the scan's finish — filter_->update's result through integrateTransformation (SE:608-617),
// reset(1) (KF:320-352) and calculateRPfromGravity + correctRollPitch (SE:602-605, 427-431).  filter_kernels.hip runs it
// on the device, host/filter_finish.cpp on the CPU: one text, so the two cannot drift apart.  Built with
// -ffp-contract=off on both sides; the only arithmetic the two do not share is libm's / ocml's sin, cos, asin, atan2.
#pragma once
#include <math.h>

#include "lins_math.h"

namespace lins_filt {

using lins::M3;
using lins::Q4;
using lins::V3;

constexpr double kDeg = 3.14159265358979323846 / 180.0;
constexpr double kG0 = 9.81;  // parameters.h:63
constexpr int kAux = 16;      // doubles of a stream's filter besides state, covariance and noise:
// 0-2 acc_last, 3-5 gyr_last, 6 time, 7-9 init_pos_std^2, 10-12 (init_att_std deg2rad)^2, 13 has_imu (0 / 1)
constexpr int kAuxAcc = 0, kAuxGyr = 3, kAuxTime = 6, kAuxPosVar = 7, kAuxAttVar = 10, kAuxHasImu = 13;

struct St {
  V3 p, v;
  Q4 q;
  V3 ba, bw, g;
};
LINS_HD St load(const double* s) {
  return {{s[0], s[1], s[2]}, {s[3], s[4], s[5]}, {s[6], s[7], s[8], s[9]}, {s[10], s[11], s[12]}, {s[13], s[14], s[15]}, {s[16], s[17], s[18]}};
}
LINS_HD void store(const St& st, double* s) {
  s[0] = st.p.x, s[1] = st.p.y, s[2] = st.p.z, s[3] = st.v.x, s[4] = st.v.y, s[5] = st.v.z;
  s[6] = st.q.w, s[7] = st.q.x, s[8] = st.q.y, s[9] = st.q.z;
  s[10] = st.ba.x, s[11] = st.ba.y, s[12] = st.ba.z, s[13] = st.bw.x, s[14] = st.bw.y, s[15] = st.bw.z;
  s[16] = st.g.x, s[17] = st.g.y, s[18] = st.g.z;
}

// ---- predict: one IMU sample (KF:137-169), in the operation order of host/state_predictor.cpp ----------------------
// The caller has applied the first-sample rule (KF:129-133).  The blocks that change from sample to sample:
//   Ft(3, 6) = -R [acc - ba]x   Ft(3, 9) = -R   Ft(6, 6) = -[gyr - bw]x   Gt(3, 0) = -R dt
// the others are constants (+-I, +-dt I) the caller writes itself.
struct Blocks {
  M3 f36, negR, f66;
};
LINS_HD Blocks propagate(St& s, V3 acc_last, V3 gyr_last, double dt, V3 acc, V3 gyr) {
  using namespace lins;
  V3 un_acc_0 = qrot(s.q, acc_last - s.ba) + s.g;
  V3 un_gyr = 0.5 * (gyr_last + gyr) - s.bw;
  s.q = qnormalized(qmul(s.q, axis2quat(dt * un_gyr)));
  V3 un_acc_1 = qrot(s.q, acc - s.ba) + s.g;
  V3 un_acc = 0.5 * (un_acc_0 + un_acc_1);
  s.p = s.p + dt * s.v + (0.5 * dt * dt) * un_acc;
  s.v = s.v + dt * un_acc;
  Blocks b;
  M3 R = qmat(s.q);
  for (int k = 0; k < 9; ++k) b.negR.m[k] = -R.m[k];
  b.f36 = mmul(b.negR, skew(acc - s.ba));
  M3 sk = skew(gyr - s.bw);
  for (int k = 0; k < 9; ++k) b.f66.m[k] = -1.0 * sk.m[k];
  return b;
}

// ---- finish -----------------------------------------------------------------------------------------------------------
LINS_HD M3 get_block(const double* M, int r, int c) {
  M3 b;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) b.m[i * 3 + j] = M[(r + i) * 18 + c + j];
  return b;
}
LINS_HD void set_block(double* M, int r, int c, const M3& b) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[(r + i) * 18 + c + j] = 1.0 * b.m[i * 3 + j];
}

// integrateTransformation (SE:608-617): the global state advanced by the filter's relative one
LINS_HD void integrate(St& g, const St& f) {
  using namespace lins;
  g.p = qrot(g.q, f.p) + g.p;
  g.q = qmul(g.q, f.q);
  g.v = qrot(qmul(g.q, qinverse(f.q)), f.v);
  g.ba = f.ba;
  g.bw = f.bw;
  g.g = qrot(g.q, f.g);
}

// reset(1) (KF:320-352) as lins_filter_reset1 computes it, the covariance's blocks only: the caller has zeroed every
// other entry of cov (a kernel does that with all its lanes).  The quirk is kept: gn_ is "rotated" by the quaternion
// that has just been set to identity, so only its norm is reset.
struct ResetBlocks {
  M3 vel, accb, gyrb, gra;
};
LINS_HD ResetBlocks reset1_blocks(const double* cov, Q4 q) {
  using namespace lins;
  M3 vel = get_block(cov, 3, 3), gra = get_block(cov, 15, 15);
  M3 R = qmat(q), Rt = mtrans(R);  // q.inverse() * M * q on matrices == R^T M R
  return {mmul(mmul(Rt, vel), R), get_block(cov, 9, 9), get_block(cov, 12, 12), mmul(mmul(Rt, gra), R)};
}
LINS_HD void reset1_store(double* cov, const ResetBlocks& b, const double* pos_var, const double* att_var) {
  for (int i = 0; i < 3; ++i) cov[(0 + i) * 18 + 0 + i] = pos_var[i], cov[(6 + i) * 18 + 6 + i] = att_var[i];
  set_block(cov, 3, 3, b.vel);
  set_block(cov, 9, 9, b.accb);
  set_block(cov, 12, 12, b.gyrb);
  set_block(cov, 15, 15, b.gra);
}
LINS_HD void reset1_state(St& s) {
  using namespace lins;
  s.p = {0, 0, 0};
  s.v = qrot(qinverse(s.q), s.v);
  s.q = {1, 0, 0, 0};
  s.g = qrot(qinverse(s.q), s.g);
  s.g = (9.81 / norm(s.g)) * s.g;
}

// calculateRPfromGravity (SE:602-605) on the reset filter's gravity, then correctRollPitch (SE:427-431): the yaw of
// Q2rpy (R2rpy of toRotationMatrix, math_utils.h) kept, roll and pitch replaced; rpy2Quat does not normalise.
LINS_HD void rp_from_gravity(V3 fbib, double& roll, double& pitch) {
  const double sg = fbib.z >= 0.0 ? 1.0 : -1.0;
  pitch = -sg * asin(fbib.x / kG0);
  roll = sg * asin(fbib.y / kG0);
}
LINS_HD void correct_roll_pitch(St& g, V3 gn) {
  using namespace lins;
  double roll, pitch;
  rp_from_gravity(gn, roll, pitch);
  const M3 R = qmat(g.q);
  const double p1 = atan2(-R.m[6], sqrt(R.m[7] * R.m[7] + R.m[8] * R.m[8]));
  const double yaw = atan2(R.m[3] / cos(p1), R.m[0] / cos(p1));
  g.q = rpy2quat(V3{roll, pitch, yaw});
}

}  // namespace lins_filt
