// filter_init.h — the yaml's filter parameters, initializeCovariance(0) and noise_ (KF:247-311) of a lins_filter, host code: lins_filter_init
// (host/state_predictor.cpp, liblins_host.so) and the template of the streams' bootstrap (lins_capi_boot.hip,
// liblins_ieskf.so) both form them here.  Unit constants: parameters.h:63-71.
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/lins_host.h"

namespace lins_filt_init {

inline void default_params(lins_filter_params* p) {
  // lins/config/exp_config/exp_port.yaml:29-62
  p->acc_n = 70000, p->gyr_n = 0.1, p->acc_w = 500, p->gyr_w = 0.05;
  for (int i = 0; i < 3; ++i) p->init_pos_std[i] = p->init_vel_std[i] = p->init_att_std[i] = 0.0;
  p->init_acc_std[0] = 0.01, p->init_acc_std[1] = 0.01, p->init_acc_std[2] = 0.02;
  p->init_gyr_std[0] = p->init_gyr_std[1] = p->init_gyr_std[2] = 0.002;
}

inline void cov_noise(const lins_filter_params* p, double* C, double* noise) {
  constexpr double kG0 = 9.81;
  constexpr double kDeg = M_PI / 180.0;
  constexpr double kDph = kDeg / 3600.0;
  const double kDpsh = kDeg / std::sqrt(3600.0);
  constexpr double kUg = kG0 / 1000.0 / 1000.0;
  std::memset(C, 0, 324 * sizeof(double));
  std::memset(noise, 0, 144 * sizeof(double));
  // initializeCovariance(0), KF:247-286
  for (int i = 0; i < 3; ++i) {
    C[(0 + i) * 18 + 0 + i] = p->init_pos_std[i] * p->init_pos_std[i];
    C[(3 + i) * 18 + 3 + i] = p->init_vel_std[i] * p->init_vel_std[i];
    double a = p->init_att_std[i] * kDeg;
    C[(6 + i) * 18 + 6 + i] = a * a;
    C[(9 + i) * 18 + 9 + i] = p->init_acc_std[i] * p->init_acc_std[i];
    C[(12 + i) * 18 + 12 + i] = p->init_gyr_std[i] * p->init_gyr_std[i];
    C[(15 + i) * 18 + 15 + i] = 0.01;
  }
  // noise_, KF:263-266, 307-311
  double peba = std::pow(p->acc_n * kUg, 2), pebg = std::pow(p->gyr_n * kDph, 2);
  double pweba = std::pow(p->acc_w * kUg, 2), pwebg = std::pow(p->gyr_w * kDpsh, 2);
  for (int i = 0; i < 3; ++i) {
    noise[(0 + i) * 12 + 0 + i] = peba;
    noise[(3 + i) * 12 + 3 + i] = pebg;
    noise[(6 + i) * 12 + 6 + i] = pweba;
    noise[(9 + i) * 12 + 9 + i] = pwebg;
  }
}

}  // namespace lins_filt_init
