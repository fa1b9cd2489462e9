// filter_finish.cpp — what processScan does to the filter and to globalState_ after performIESKF, on the CPU:
// filter_->update (SE:585-598), integrateTransformation (SE:608-617), reset(1) (KF:320-352), calculateRPfromGravity +
// correctRollPitch (SE:602-605, 427-431).  The restatement filter_finish_kernel (csrc/filter_kernels.hip) is checked
// against; the arithmetic is csrc/filter_math.h in both libraries.

#include <cstring>

#include "../../../include/lins_host.h"
#include "../filter_math.h"

using namespace lins_filt;

extern "C" void lins_filter_finish(lins_filter* f, double* global_state, const lins_result* posterior, int used_prior_cov) {
  // filter_->update(state, Pk_): a diverged update hands over the ICP pose with Pk_ un-updated, which is the
  // covariance the filter already holds
  std::memcpy(f->state, posterior->state, sizeof f->state);
  if (!used_prior_cov) std::memcpy(f->cov, posterior->cov, sizeof f->cov);
  St s = load(f->state), g = load(global_state);
  const ResetBlocks rb = reset1_blocks(f->cov, s.q);
  double pos_var[3], att_var[3];
  for (int i = 0; i < 3; ++i) {
    pos_var[i] = f->prm.init_pos_std[i] * f->prm.init_pos_std[i];
    const double a = f->prm.init_att_std[i] * kDeg;
    att_var[i] = a * a;
  }
  std::memset(f->cov, 0, sizeof f->cov);
  reset1_store(f->cov, rb, pos_var, att_var);
  integrate(g, s);
  reset1_state(s);
  correct_roll_pitch(g, s.g);
  store(s, f->state);
  store(g, global_state);
}
