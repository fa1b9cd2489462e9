// boot.cpp — CPU restatement of the two-scan bootstrap (processFirstScan / processSecondScan, SE:331-425) around the ICP:
// the IMU pre-integration between the two scans, the pose estimateTransform starts from, and the initialisation of the
// filter and of globalState_ from the ICP's pose.  The arithmetic is csrc/boot_math.h, the text the device kernels
// (boot_kernels.hip) compile too; the ICP itself is not restated (oracle ref_icp, the device kernel).  Part of both
// libraries: liblins_ieskf.so forms the streams' filter template with the same code.
#include <cstring>

#include "../../../include/lins_host.h"
#include "../boot_math.h"
#include "../filter_init.h"

using namespace lins;
using namespace lins_boot;

namespace {
V3 v3(const double* p) { return {p[0], p[1], p[2]}; }
// StatePredictor::initialization (KF:234-245) of `f` with the state row `s`
void filter_initialise(lins_filter* f, const St& s, const double* imu_last, double time, const lins_boot_params* prm) {
  std::memset(f, 0, sizeof *f);
  f->prm = prm->filter;
  lins_filt::store(s, f->state);
  lins_filt_init::cov_noise(&prm->filter, f->cov, f->noise);
  std::memcpy(f->acc_last, imu_last, 3 * sizeof(double));
  std::memcpy(f->gyr_last, imu_last + 3, 3 * sizeof(double));
  f->time = time, f->has_imu = 1;
}
}  // namespace

extern "C" {

void lins_boot_default_params(lins_boot_params* p) {
  lins_filt_init::default_params(&p->filter);
  // exp_port.yaml:65-76
  p->init_ba[0] = -0.015774, p->init_ba[1] = 0.143237, p->init_ba[2] = -0.0263845;
  p->init_bw[0] = -0.00275058, p->init_bw[1] = -0.000165954, p->init_bw[2] = 0.00262913;
}

void lins_host_preintegrate(lins_preintegration* pre, int n_rows, const double* rows, const double* init_ba, const double* init_bw) {
  Pre r = pre_load(&pre->sum_dt);
  for (int i = 0; i < n_rows; ++i) pre_step(r, rows[i * 7], v3(rows + i * 7 + 1), v3(rows + i * 7 + 4), v3(init_ba), v3(init_bw));
  pre_store(r, &pre->sum_dt);
}

void lins_host_boot_start(const lins_preintegration* pre, double* t, double* q) {
  const St s = start_row(pre_load(&pre->sum_dt));
  t[0] = s.p.x, t[1] = s.p.y, t[2] = s.p.z;
  q[0] = s.q.w, q[1] = s.q.x, q[2] = s.q.y, q[3] = s.q.z;
}

void lins_host_boot_first(lins_filter* f, double* global_state, double* lin_state19, lins_preintegration* pre, const double imu_last[6],
                          double time, const lins_boot_params* prm) {
  (void)global_state;  // (globalState_ is not touched by processFirstScan)
  filter_initialise(f, identity_state(), imu_last, time, prm);
  lins_filt::store(identity_state(), lin_state19);
  pre_store(pre_reset(v3(imu_last), v3(imu_last + 3)), &pre->sum_dt);
}

void lins_host_boot_second(lins_filter* f, double* global_state, double* lin_state19, const lins_preintegration* pre, const double icp_t[3],
                           const double icp_q[4], const double imu_last[6], double time, const lins_boot_params* prm) {
  const Second o = second_scan(v3(icp_t), Q4{icp_q[0], icp_q[1], icp_q[2], icp_q[3]}, pre->sum_dt, v3(imu_last), v3(prm->init_ba), v3(prm->init_bw));
  filter_initialise(f, o.filter, imu_last, time, prm);
  lins_filt::store(o.global, global_state);
  lins_filt::store(o.lin, lin_state19);
}

}  // extern "C"
