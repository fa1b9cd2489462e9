// odom_math.h — the scalar definition of the seam between the filter and the mapping node, host + device (DESIGN.md §5.3
// "Streams end to end"): updatePointCloud's XYZ -> YZX change of globalState_ (SE:1150-1154) as publishOdometryYZX sends
// it (EC:294-305), the mapping node's laserOdometryHandler (LM:711-724, identical at TF:217-231) and the quaternion the
// transform fusion node publishes (TF:235-242, LM:752-759).  odom_kernels.hip runs it on the device, host/odom.cpp on
// the CPU: one text, so the two cannot drift apart.  Built with -ffp-contract=off on both sides; the only arithmetic the
// two do not share is libm's / ocml's f64 sin, cos, asin, atan2.
//
// tf is not part of the reference's text (the oracle's stand-in getRPY returns zeros), so the contract is this
// project's own statement of tf's documented arithmetic — tf::Matrix3x3::setRotation, getRPY (getEulerYPR, first
// solution) and tf::Quaternion::setRPY — in f64, operand for operand as written below.  quaternionTFToMsg's
// re-normalisation (only beyond a squared-norm error of 0.1) never triggers on setRPY's output and is not stated.
//
// Departures:
//   odom_yzx is the EXACT axis permutation.  Q_xyz_to_yzx is the quaternion of a pure axis permutation, (0.5, 0.5, 0.5,
//   0.5) up to sign; Eigen's two quaternion products (SE:1153-1154) and its rotation of rn_ (SE:1152) give the permuted
//   components up to their f64 rounding (each quaternion component a sum of four products of exact halves: within
//   8 x 2^-53 of the permutation for a unit quaternion).  The permutation is what those products round towards.
//   The fused pose is mp_associate (map_pose_math.h): TF:91-215 is LM:411-536 operand for operand with transformMapped
//   in the place of transformTobeMapped — the one regrouping is the difference transformBefMapped - transformSum, which
//   the node's text forms inside x1 / z1 and mp_associate forms once (same operands, same bits).  The fusion node reads
//   transformAftMapped back through the quaternion of /aft_mapped_to_init (TF:256-268); here it is the resident
//   transformAftMapped itself, without that round trip.
#pragma once
#include <math.h>

#include "../../include/lins_host.h"
#include "lins_math.h"
#include "map_pose_math.h"

namespace lins_od {

constexpr double kHalfPi = 3.14159265358979323846 / 2.0;  // TFSIMD_HALF_PI

LINS_HD bool od_finite(double x) { return fabs(x) <= __DBL_MAX__; }

// globalStateYZX_ of globalState_ (19 doubles: rn_ 0-2, qbn_ 6-9 as w, x, y, z): rn_ and qbn_ as (x, y, z, w)
LINS_HD void odom_yzx(const double gs[19], double pos[3], double q_xyzw[4]) {
  pos[0] = gs[1], pos[1] = gs[2], pos[2] = gs[0];
  q_xyzw[0] = gs[8], q_xyzw[1] = gs[9], q_xyzw[2] = gs[7], q_xyzw[3] = gs[6];
}

// transformSum of /laser_odom_to_init (LM:711-724): tf::Matrix3x3(tf::Quaternion(q.z, -q.x, -q.y, q.w)).getRPY, then
// (-pitch, -yaw, roll, x, y, z) rounded to float
LINS_HD void odom_transform_sum(const double pos[3], const double q_xyzw[4], float sum[6]) {
  const double x = q_xyzw[2], y = -q_xyzw[0], z = -q_xyzw[1], w = q_xyzw[3];
  // Matrix3x3::setRotation
  const double d = x * x + y * y + z * z + w * w;
  const double s = 2.0 / d;
  const double xs = x * s, ys = y * s, zs = z * s;
  const double wx = w * xs, wy = w * ys, wz = w * zs;
  const double xx = x * xs, xy = x * ys, xz = x * zs;
  const double yy = y * ys, yz = y * zs, zz = z * zs;
  const double m00 = 1.0 - (yy + zz), m01 = xy - wz, m02 = xz + wy;
  const double m10 = xy + wz;
  const double m20 = xz - wy, m21 = yz + wx, m22 = 1.0 - (xx + yy);
  // Matrix3x3::getRPY (getEulerYPR, solution 1)
  double roll, pitch, yaw;
  if (fabs(m20) >= 1.0) {  // gimbal lock
    yaw = 0.0;
    if (m20 < 0.0) {
      pitch = kHalfPi;
      roll = atan2(m01, m02);
    } else {
      pitch = -kHalfPi;
      roll = atan2(-m01, -m02);
    }
  } else {
    pitch = -asin(m20);
    roll = atan2(m21 / cos(pitch), m22 / cos(pitch));
    yaw = atan2(m10 / cos(pitch), m00 / cos(pitch));
  }
  sum[0] = (float)-pitch, sum[1] = (float)-yaw, sum[2] = (float)roll;
  sum[3] = (float)pos[0], sum[4] = (float)pos[1], sum[5] = (float)pos[2];
}

// The orientation published with a pose t = (rx, ry, rz, tx, ty, tz) (TF:235-242, LM:752-759):
// createQuaternionMsgFromRollPitchYaw(t[2], -t[0], -t[1]) — tf::Quaternion::setRPY — sent as (-y, -z, x, w)
LINS_HD void pose_quat(const float t[6], double q_xyzw[4]) {
  const double roll = (double)t[2], pitch = -(double)t[0], yaw = -(double)t[1];
  const double hy = yaw * 0.5, hp = pitch * 0.5, hr = roll * 0.5;
  const double cy = cos(hy), sy = sin(hy), cp = cos(hp), sp = sin(hp), cr = cos(hr), sr = sin(hr);
  const double x = sr * cp * cy - cr * sp * sy;
  const double y = cr * sp * cy + sr * cp * sy;
  const double z = cr * cp * sy - sr * sp * cy;
  const double w = cr * cp * cy + sr * sp * sy;
  q_xyzw[0] = -y, q_xyzw[1] = -z, q_xyzw[2] = x, q_xyzw[3] = w;
}

// One stream's record.  has_state == 0 (no globalState_ yet), a non-finite rn_ / qbn_ or a non-finite transformSum (a
// zero quaternion: tf's 2 / d) leave valid = 0 and everything else zero.
LINS_HD void odom_record(const double gs[19], int has_state, lins_stream_odom* out) {
  lins_stream_odom r;
  for (int i = 0; i < 3; ++i) r.position[i] = 0.0, r.transform_sum[i] = r.transform_sum[3 + i] = 0.f;
  for (int i = 0; i < 4; ++i) r.orientation[i] = 0.0;
  r.valid = 0, r.reserved = 0;
  bool ok = has_state != 0;
  if (ok) {
    double pos[3], q[4];
    float sum[6];
    odom_yzx(gs, pos, q);
    for (int i = 0; i < 3; ++i) ok = ok && od_finite(pos[i]);
    for (int i = 0; i < 4; ++i) ok = ok && od_finite(q[i]);
    if (ok) {
      odom_transform_sum(pos, q, sum);
      for (int i = 0; i < 6; ++i) ok = ok && od_finite((double)sum[i]);
    }
    if (ok) {
      for (int i = 0; i < 3; ++i) r.position[i] = pos[i];
      for (int i = 0; i < 4; ++i) r.orientation[i] = q[i];
      for (int i = 0; i < 6; ++i) r.transform_sum[i] = sum[i];
      r.valid = 1;
    }
  }
  *out = r;
}

// /integrated_to_init (TF:217-254): transformMapped = transformAssociateToMap of (bef, aft, sum) and its orientation
LINS_HD void odom_fuse(const float bef[6], const float aft[6], const float sum[6], lins_fused_pose* out) {
  float tm[6];
  double q[4];
  lins_mp::mp_associate(bef, aft, sum, tm);
  pose_quat(tm, q);
  for (int i = 0; i < 6; ++i) out->transform_mapped[i] = tm[i];
  for (int i = 0; i < 4; ++i) out->orientation[i] = q[i];
}

}  // namespace lins_od
