// filter_kernels.hip — the streams' device-resident filter (DESIGN.md §5.3 "Device-resident filter"; scalar text:
// filter_math.h).
//
// filter_predict_kernel   StatePredictor::predict (KF:125-186) of every stream over the stream's own IMU rows
//                         (dt, acc, gyr), in place.  One workgroup of two waves per stream; the samples of a stream are
//                         strictly sequential.  P, Ft, F, F P, the un-symmetrised sum, Gt, Gt Q and Q live in LDS (18 KB);
//                         lane 0 propagates the state and writes the blocks of Ft / Gt that change, every lane then owns
//                         output elements (i, j) = lane, lane + 128, lane + 256 of each 18 x 18 product.  Every dot product
//                         runs left to right over k in f64 as host/state_predictor.cpp's does, no contraction: the host
//                         mirror and the kernel differ only where ocml's sin / cos differ from libm's.
// filter_finish_kernel    after the update (and the ICP fallback): filter_->update, integrateTransformation, reset(1),
//                         calculateRPfromGravity + correctRollPitch, per stream, by one wave.  Reads the posterior rows,
//                         never writes them (the re-projection that follows still reads linState_ there).
// Every store is a vector store.
#include <hip/hip_runtime.h>

#include "filter_math.h"
#include "lins_launch.h"

namespace lins {
namespace {

using namespace lins_filt;

constexpr int kPredictThreads = 128;

__global__ __launch_bounds__(kPredictThreads) void filter_predict_kernel(int n, const int* __restrict__ n_imu, const int* __restrict__ imu_off,
                                                                         const double* __restrict__ imu, double* __restrict__ state,
                                                                         double* __restrict__ cov, const double* __restrict__ noise,
                                                                         double* __restrict__ aux) {
  const int k = blockIdx.x, tid = threadIdx.x;
  if (k >= n) return;
  const int cnt = n_imu[k];
  if (cnt <= 0) return;  // (uniform over the workgroup) no sample: the stream stays bit for bit as it is
  __shared__ double P[324], Ft[324], F[324], T[324], Pn[324], Gt[216], GQ[216], Q[144];
  double* gP = cov + (size_t)k * 324;
  for (int o = tid; o < 324; o += kPredictThreads) P[o] = gP[o], Ft[o] = 0.0;
  for (int o = tid; o < 216; o += kPredictThreads) Gt[o] = 0.0;
  for (int o = tid; o < 144; o += kPredictThreads) Q[o] = noise[(size_t)k * 144 + o];
  __syncthreads();
  // lane 0's registers across the samples
  St s{};
  V3 acc_last{}, gyr_last{};
  double time = 0.0;
  bool has_imu = false;
  const double* rows = imu + (size_t)imu_off[k] * 7;
  double* a = aux + (size_t)k * kAux;
  if (tid == 0) {
    s = load(state + (size_t)k * 19);
    acc_last = {a[kAuxAcc], a[kAuxAcc + 1], a[kAuxAcc + 2]}, gyr_last = {a[kAuxGyr], a[kAuxGyr + 1], a[kAuxGyr + 2]};
    time = a[kAuxTime], has_imu = a[kAuxHasImu] != 0.0;
    // the constant blocks of Ft (KF:149-160)
    for (int i = 0; i < 3; ++i) Ft[(0 + i) * 18 + 3 + i] = 1.0, Ft[(3 + i) * 18 + 15 + i] = 1.0, Ft[(6 + i) * 18 + 12 + i] = -1.0;
  }
  for (int it = 0; it < cnt; ++it) {
    const double dt = rows[it * 7];
    if (tid == 0) {
      const V3 acc{rows[it * 7 + 1], rows[it * 7 + 2], rows[it * 7 + 3]}, gyr{rows[it * 7 + 4], rows[it * 7 + 5], rows[it * 7 + 6]};
      if (!has_imu) has_imu = true, acc_last = acc, gyr_last = gyr;  // KF:129-133
      const Blocks b = propagate(s, acc_last, gyr_last, dt, acc, gyr);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          Ft[(3 + i) * 18 + 6 + j] = b.f36.m[i * 3 + j];
          Ft[(3 + i) * 18 + 9 + j] = b.negR.m[i * 3 + j];
          Ft[(6 + i) * 18 + 6 + j] = b.f66.m[i * 3 + j];
          Gt[(3 + i) * 12 + 0 + j] = dt * b.negR.m[i * 3 + j];
        }
      for (int i = 0; i < 3; ++i) Gt[(6 + i) * 12 + 3 + i] = -dt, Gt[(9 + i) * 12 + 6 + i] = dt, Gt[(12 + i) * 12 + 9 + i] = dt;
      time += dt, acc_last = acc, gyr_last = gyr;
    }
    __syncthreads();
    // F = I + Ft dt + 0.5 Ft Ft dt dt (KF:173);  GQ = Gt Q
    for (int o = tid; o < 324; o += kPredictThreads) {
      const int i = o / 18, j = o - i * 18;
      double acc2 = 0;
      for (int c = 0; c < 18; ++c) acc2 += Ft[i * 18 + c] * Ft[c * 18 + j];
      F[o] = (i == j ? 1.0 : 0.0) + Ft[o] * dt + 0.5 * acc2 * dt * dt;
    }
    for (int o = tid; o < 216; o += kPredictThreads) {
      const int i = o / 12, j = o - i * 12;
      double g = 0;
      for (int c = 0; c < 12; ++c) g += Gt[i * 12 + c] * Q[c * 12 + j];
      GQ[o] = g;
    }
    __syncthreads();
    for (int o = tid; o < 324; o += kPredictThreads) {  // T = F P
      const int i = o / 18, j = o - i * 18;
      double t = 0;
      for (int c = 0; c < 18; ++c) t += F[i * 18 + c] * P[c * 18 + j];
      T[o] = t;
    }
    __syncthreads();
    for (int o = tid; o < 324; o += kPredictThreads) {  // T F^T + GQ Gt^T (KF:176)
      const int i = o / 18, j = o - i * 18;
      double t = 0;
      for (int c = 0; c < 18; ++c) t += T[i * 18 + c] * F[j * 18 + c];
      double g = 0;
      for (int c = 0; c < 12; ++c) g += GQ[i * 12 + c] * Gt[j * 12 + c];
      Pn[o] = t + g;
    }
    __syncthreads();
    for (int o = tid; o < 324; o += kPredictThreads) {  // enforceSymmetry (KF:178)
      const int i = o / 18, j = o - i * 18;
      P[o] = 0.5 * (Pn[o] + Pn[j * 18 + i]);
    }
    // (the next sample's lane-0 stage writes Ft / Gt only: their last readers are behind the barrier above; P is next
    // read two barriers on)
  }
  __syncthreads();
  for (int o = tid; o < 324; o += kPredictThreads) gP[o] = P[o];
  if (tid == 0) {
    store(s, state + (size_t)k * 19);
    a[kAuxAcc] = acc_last.x, a[kAuxAcc + 1] = acc_last.y, a[kAuxAcc + 2] = acc_last.z;
    a[kAuxGyr] = gyr_last.x, a[kAuxGyr + 1] = gyr_last.y, a[kAuxGyr + 2] = gyr_last.z;
    a[kAuxTime] = time, a[kAuxHasImu] = has_imu ? 1.0 : 0.0;
  }
}

// mode[k]: 0 = leave the stream's filter as it is (gated scan; a diverged stream that keeps the whole prior),
//          1 = the posterior state and covariance rows, 2 = the posterior state row with the PRIOR covariance (Pk_
//          un-updated, SE:585-592: what the filter holds — the covariance is then already in place)
__global__ __launch_bounds__(64) void filter_finish_kernel(int n, const int* __restrict__ mode, const double* __restrict__ post_state,
                                                           const double* __restrict__ post_cov, double* __restrict__ state,
                                                           double* __restrict__ cov, const double* __restrict__ aux,
                                                           double* __restrict__ gstate) {
  const int k = blockIdx.x, tid = threadIdx.x;
  if (k >= n) return;
  const int m = mode[k];
  if (m == 0) return;
  __shared__ double C[324];
  const double* src = m == 1 ? post_cov + (size_t)k * 324 : cov + (size_t)k * 324;
  for (int o = tid; o < 324; o += 64) C[o] = src[o];
  __syncthreads();
  St f = load(post_state + (size_t)k * 19);  // filter_->update(linState_ / filterState, Pk_)
  ResetBlocks rb{};
  if (tid == 0) rb = reset1_blocks(C, f.q);
  __syncthreads();
  for (int o = tid; o < 324; o += 64) C[o] = 0.0;
  __syncthreads();
  if (tid == 0) {
    const double* a = aux + (size_t)k * kAux;
    reset1_store(C, rb, a + kAuxPosVar, a + kAuxAttVar);
    St g = load(gstate + (size_t)k * 19);
    integrate(g, f);
    reset1_state(f);
    correct_roll_pitch(g, f.g);
    store(f, state + (size_t)k * 19);
    store(g, gstate + (size_t)k * 19);
  }
  __syncthreads();
  double* dst = cov + (size_t)k * 324;
  for (int o = tid; o < 324; o += 64) dst[o] = C[o];
}

}  // namespace

void launch_filter_predict(hipStream_t stream, int n, const int* n_imu, const int* imu_off, const double* imu, double* state, double* cov, const double* noise, double* aux) {
  hipLaunchKernelGGL(filter_predict_kernel, dim3(n), dim3(kPredictThreads), 0, stream, n, n_imu, imu_off, imu, state, cov, noise, aux);
}
void launch_filter_finish(hipStream_t stream, int n, const int* mode, const double* post_state, const double* post_cov, double* state, double* cov, const double* aux, double* gstate) {
  hipLaunchKernelGGL(filter_finish_kernel, dim3(n), dim3(64), 0, stream, n, mode, post_state, post_cov, state, cov, aux, gstate);
}

}  // namespace lins
