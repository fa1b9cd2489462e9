// boot_math.h — the scalar definition of the two-scan bootstrap (processFirstScan / processSecondScan, SE:331-425), host
// + device (DESIGN.md §5.3 "Two-scan bootstrap"): one row of the IMU pre-integration between the two scans (IB:53-81,
// 161-188, the part estimateInitialState reads), the pose estimateTransform starts from, and what the second scan makes of
// the ICP's pose — the filter's initial state and globalState_.  boot_kernels.hip runs it on the device, host/boot.cpp on
// the CPU: one text.  Built with -ffp-contract=off on both sides; the pre-integration and the start pose are +, -, x, /
// and sqrt only (bit-equal on both sides), the finish also asin / sin / cos (libm against ocml).
#pragma once
#include <math.h>

#include "filter_math.h"

namespace lins_boot {

using lins::Q4;
using lins::V3;
using lins_filt::kG0;
using lins_filt::St;

// the pre-integration record of a stream between its first and its second scan: the layout of lins_preintegration
// (include/lins_streams_filter.h) — sum_dt, delta_p, delta_q (w x y z), delta_v, acc_0, gyr_0
constexpr int kPre = 17;
struct Pre {
  double sum_dt;
  V3 dp;
  Q4 dq;
  V3 dv, acc0, gyr0;
};
LINS_HD Pre pre_load(const double* r) {
  return {r[0], {r[1], r[2], r[3]}, {r[4], r[5], r[6], r[7]}, {r[8], r[9], r[10]}, {r[11], r[12], r[13]}, {r[14], r[15], r[16]}};
}
LINS_HD void pre_store(const Pre& p, double* r) {
  r[0] = p.sum_dt, r[1] = p.dp.x, r[2] = p.dp.y, r[3] = p.dp.z;
  r[4] = p.dq.w, r[5] = p.dq.x, r[6] = p.dq.y, r[7] = p.dq.z;
  r[8] = p.dv.x, r[9] = p.dv.y, r[10] = p.dv.z;
  r[11] = p.acc0.x, r[12] = p.acc0.y, r[13] = p.acc0.z, r[14] = p.gyr0.x, r[15] = p.gyr0.y, r[16] = p.gyr0.z;
}
// IntegrationBase(imu_last_.acc, imu_last_.gyr, ...) of processFirstScan (SE:355-356, IB:35-51)
LINS_HD Pre pre_reset(V3 acc, V3 gyr) { return {0.0, {0, 0, 0}, {1, 0, 0, 0}, {0, 0, 0}, acc, gyr}; }

// push_back -> propagate -> midPointIntegration (IB:70-78, 179-187) with linearized_ba / bg = INIT_BA / INIT_BW: the
// quaternion increment (1, w dt / 2) is NOT a unit quaternion, delta_q is normalised after the row.  The 15 x 15
// jacobian and covariance of the reference are never read on the live path and are not formed.
LINS_HD void pre_step(Pre& r, double dt, V3 acc, V3 gyr, V3 ba, V3 bg) {
  using namespace lins;
  const V3 un_acc_0 = qrot(r.dq, r.acc0 - ba);
  const V3 un_gyr = 0.5 * (r.gyr0 + gyr) - bg;
  const Q4 q1 = qmul(r.dq, Q4{1.0, un_gyr.x * dt / 2, un_gyr.y * dt / 2, un_gyr.z * dt / 2});
  const V3 un_acc_1 = qrot(q1, acc - ba);
  const V3 un_acc = 0.5 * (un_acc_0 + un_acc_1);
  r.dp = (r.dp + dt * r.dv) + dt * (dt * (0.5 * un_acc));
  r.dv = r.dv + dt * un_acc;
  r.dq = qnormalized(q1);
  r.sum_dt += dt;
  r.acc0 = acc, r.gyr0 = gyr;
}

// the state rows are those of lins_filt::St: p, v, q (w x y z), ba, bw, g
LINS_HD St identity_state() { return {{0, 0, 0}, {0, 0, 0}, {1, 0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, -kG0}}; }

// the pose estimateTransform starts from (SE:392-396; ba0 = 0 there, so the third term is exactly zero), as the row the
// ICP kernel reads: linState_ of the first scan (identity, SE:352) with rn_, qbn_ replaced (SE:1165-1166)
LINS_HD St start_row(const Pre& r) {
  using namespace lins;
  St s = identity_state();
  s.p = r.dp + r.sum_dt * (r.sum_dt * (0.5 * s.g));
  s.q = r.dq;
  return s;
}

// processSecondScan behind estimateTransform (SE:401-415): estimateInitialState (SE:1408-1419), the filter's
// initialization (KF:234-245: identity attitude, position pl), roll / pitch from the last IMU sample and globalState_.
// lin: linState_ (the ICP's pose in the first scan's identity state), what updatePointCloud re-projects with.
struct Second {
  St filter, global, lin;
};
LINS_HD Second second_scan(V3 pl, Q4 ql, double sum_dt, V3 imu_acc, V3 ba, V3 bw) {
  using namespace lins;
  Second o;
  const V3 v1 = pl / sum_dt;
  o.filter = identity_state();
  o.filter.p = pl, o.filter.v = v1, o.filter.ba = ba, o.filter.bw = bw;
  double roll, pitch;
  lins_filt::rp_from_gravity(imu_acc - ba, roll, pitch);
  o.global = o.filter;
  o.global.q = rpy2quat(V3{roll, pitch, 0.0});
  o.lin = identity_state();
  o.lin.p = pl, o.lin.q = ql;
  return o;
}

// ---- the template a bootstrapping filter is initialised from (host side; uploaded once per context) -------------------
// [covariance 324 | noise 144 | init_pos_std^2 3 | (init_att_std deg2rad)^2 3 | INIT_BA 3 | INIT_BW 3]
constexpr int kTmplCov = 0, kTmplNoise = 324, kTmplPosVar = 468, kTmplAttVar = 471, kTmplBa = 474, kTmplBw = 477, kTmpl = 480;

}  // namespace lins_boot
