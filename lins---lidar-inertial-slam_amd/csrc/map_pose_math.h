// map_pose_math.h — the scalar definition of the mapping node's own pose arithmetic, host + device (DESIGN.md §5.3
// "Mapping node's step"): transformAssociateToMap (LM:411-536), the tail of transformUpdate (LM:567-576) and the
// key-frame rule (LM:1655-1671).  map_pose_kernels.hip runs it on the device, host/map_pose.cpp on the CPU: one text, so
// the two cannot drift apart.  Built with -ffp-contract=off on both sides; the only arithmetic the two do not share is
// libm's / ocml's sinf, cosf, asinf, atan2f.
//
// Everything is f32 in the reference's order of operations.  Its unqualified sin / cos / asin / atan2 act on float
// members in a translation unit that includes <cmath>: they are the float overloads (the reading DESIGN.md §5.3 makes
// for updateTransformPointCloudSinCos).  A product of the reference's text that appears more than once is formed once
// here — the same operands in the same order give the same bits.  transformIncre is a local.
//
// Pose vectors are (rx, ry, rz, tx, ty, tz) as transformTobeMapped.  |rx| of the result near pi / 2 is outside the
// contract: the reference divides by cos(rx) there.
#pragma once
#include <math.h>

#include "lins_math.h"

namespace lins_mp {

// transformTobeMapped from transformBefMapped, transformAftMapped and transformSum (LM:411-536)
LINS_HD void mp_associate(const float bef[6], const float aft[6], const float sum[6], float tobe[6]) {
  const float sbcx = sinf(sum[0]), cbcx = cosf(sum[0]), sbcy = sinf(sum[1]), cbcy = cosf(sum[1]), sbcz = sinf(sum[2]), cbcz = cosf(sum[2]);
  const float sblx = sinf(bef[0]), cblx = cosf(bef[0]), sbly = sinf(bef[1]), cbly = cosf(bef[1]), sblz = sinf(bef[2]), cblz = cosf(bef[2]);
  const float salx = sinf(aft[0]), calx = cosf(aft[0]), saly = sinf(aft[1]), caly = cosf(aft[1]), salz = sinf(aft[2]), calz = cosf(aft[2]);

  // the increment since the last mapped scan, in the odometry's frame (LM:412-426)
  const float dx = bef[3] - sum[3], dy = bef[4] - sum[4], dz = bef[5] - sum[5];
  const float x1 = cbcy * dx - sbcy * dz;
  const float y1 = dy;
  const float z1 = sbcy * dx + cbcy * dz;
  const float x2 = x1;
  const float y2 = cbcx * y1 + sbcx * z1;
  const float z2 = -sbcx * y1 + cbcx * z1;
  const float inc3 = cbcz * x2 + sbcz * y2;
  const float inc4 = -sbcz * x2 + cbcz * y2;
  const float inc5 = z2;

  // the factors of R_aft R_bef^T the five sums below share (LM:449-515)
  const float b1 = cbly * sblz - cblz * sblx * sbly;
  const float b2 = cbly * cblz + sblx * sbly * sblz;
  const float b3 = cblz * sbly - cbly * sblx * sblz;
  const float b4 = sbly * sblz + cbly * cblz * sblx;
  const float a1 = caly * salz - calz * salx * saly;
  const float a2 = caly * calz + salx * saly * salz;
  const float a3 = calz * saly - caly * salx * salz;
  const float a4 = saly * salz + caly * calz * salx;
  const float mA = salx * sblx + calx * cblx * salz * sblz + calx * calz * cblx * cblz;
  const float mB = calx * calz * b1 - calx * salz * b2 + cblx * salx * sbly;
  const float mC = calx * salz * b3 - calx * calz * b4 + cblx * cbly * salx;

  const float srx = -sbcx * mA - cbcx * sbcy * mB - cbcx * cbcy * mC;
  tobe[0] = -asinf(srx);

  const float srycrx = sbcx * (cblx * cblz * a1 - cblx * sblz * a2 + calx * saly * sblx) -
                       cbcx * cbcy * (a2 * b3 + a1 * b4 - calx * cblx * cbly * saly) +
                       cbcx * sbcy * (a2 * b2 + a1 * b1 + calx * cblx * saly * sbly);
  const float crycrx = sbcx * (cblx * sblz * a3 - cblx * cblz * a4 + calx * caly * sblx) +
                       cbcx * cbcy * (a4 * b4 + a3 * b3 + calx * caly * cblx * cbly) -
                       cbcx * sbcy * (a4 * b1 + a3 * b2 - calx * caly * cblx * sbly);
  tobe[1] = atan2f(srycrx / cosf(tobe[0]), crycrx / cosf(tobe[0]));

  const float srzcrx = (cbcz * sbcy - cbcy * sbcx * sbcz) * mC - (cbcy * cbcz + sbcx * sbcy * sbcz) * mB + cbcx * sbcz * mA;
  const float crzcrx = (cbcy * sbcz - cbcz * sbcx * sbcy) * mB - (sbcy * sbcz + cbcy * cbcz * sbcx) * mC + cbcx * cbcz * mA;
  tobe[2] = atan2f(srzcrx / cosf(tobe[0]), crzcrx / cosf(tobe[0]));

  // the increment turned into the map frame and taken off transformAftMapped's translation (LM:519-535)
  const float u1 = cosf(tobe[2]) * inc3 - sinf(tobe[2]) * inc4;
  const float v1 = sinf(tobe[2]) * inc3 + cosf(tobe[2]) * inc4;
  const float w1 = inc5;
  const float u2 = u1;
  const float v2 = cosf(tobe[0]) * v1 - sinf(tobe[0]) * w1;
  const float w2 = sinf(tobe[0]) * v1 + cosf(tobe[0]) * w1;
  tobe[3] = aft[3] - (cosf(tobe[1]) * u2 + sinf(tobe[1]) * w2);
  tobe[4] = aft[4] - v2;
  tobe[5] = aft[5] - (-sinf(tobe[1]) * u2 + cosf(tobe[1]) * w2);
}

// The tail of transformUpdate (LM:567-576); imuHandler's interpolation (LM:539-565) is the caller's, its results come
// in as imu_roll / imu_pitch.  0.998 and 0.002 are double literals: the blend is an f64 expression rounded once to f32.
LINS_HD void mp_transform_update(float tobe[6], int has_imu, float imu_roll, float imu_pitch, const float sum[6], float bef[6], float aft[6]) {
  if (has_imu) {
    tobe[0] = (float)(0.998 * (double)tobe[0] + 0.002 * (double)imu_pitch);
    tobe[2] = (float)(0.998 * (double)tobe[2] + 0.002 * (double)imu_roll);
  }
  for (int i = 0; i < 6; ++i) bef[i] = sum[i], aft[i] = tobe[i];
}

// The key-frame rule (LM:1655-1671): 1 when this scan becomes a key frame, and then prev takes transformAftMapped's
// position.  f32 differences, f32 sum in the written order, the float sqrt, compared with the double literal 0.3; a
// node without key frames (have_frames == 0) saves whatever the distance.
LINS_HD int mp_key_rule(float prev[3], const float aft[6], int have_frames) {
  const float ex = prev[0] - aft[3], ey = prev[1] - aft[4], ez = prev[2] - aft[5];
  const float d = sqrtf(ex * ex + ey * ey + ez * ez);
  const bool save = !((double)d < 0.3);
  if (!save && have_frames) return 0;
  prev[0] = aft[3], prev[1] = aft[4], prev[2] = aft[5];
  return 1;
}

// saveKeyFramesAndFactor's pose bookkeeping with iSAM2 as the identity (the departure DESIGN.md §5.3 documents): the
// first key frame takes transformTobeMapped (LM:1676-1686), every later one transformAftMapped (LM:1699-1704), and for
// every frame after the first transformLast = transformTobeMapped = transformAftMapped (LM:1737-1749).
LINS_HD void mp_key_pose(float tobe[6], const float aft[6], float last[6], int* n_frames, float key_pose[6]) {
  if (*n_frames == 0) {
    for (int i = 0; i < 6; ++i) key_pose[i] = last[i] = tobe[i];
  } else {
    for (int i = 0; i < 6; ++i) key_pose[i] = last[i] = tobe[i] = aft[i];
  }
  *n_frames += 1;
}

}  // namespace lins_mp
