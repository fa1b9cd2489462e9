// boot_kernels.hip — the two-scan bootstrap of the device-resident streams (DESIGN.md §5.3 "Two-scan bootstrap"; scalar
// text: boot_math.h).
//
// boot_preintegrate_kernel  IntegrationBase::push_back (IB:53-81, 161-188) of every FIRST_SCAN stream over its own rows,
//                           and filter_->time_ += dt (SE:247-248).  One lane per stream, the rows of a stream strictly in
//                           order; the rows arrive component-major ([row][component][stream]), so that the lanes of a
//                           wave read one contiguous run per load.  Workgroups of one wave: a 1024-stream batch is 16
//                           full waves on 16 compute units.
// boot_start_kernel         the pose estimateTransform starts from (SE:392-396) as the ICP kernel's state row, one lane
//                           per stream taking its second scan.
// boot_finish_kernel        per stream by one wave: first scan (SE:339-361) — the zero-initialised filter from the
//                           template, the pre-integration record reset, linState_ = identity —; second scan (SE:401-415)
//                           — filter and globalState_ from the ICP's pose, linState_ = (pl, ql) in the row the
//                           re-projection reads.  Mode 0 writes nothing.
// Every store is a vector store.
#include <hip/hip_runtime.h>

#include "boot_math.h"
#include "lins_launch.h"

namespace lins {
namespace {

using namespace lins_boot;
using namespace lins_filt;

constexpr int kBootThreads = 64;

__global__ __launch_bounds__(kBootThreads) void boot_preintegrate_kernel(int n, const int* __restrict__ n_rows, const double* __restrict__ rows,
                                                                         const double* __restrict__ tmpl, double* __restrict__ pre,
                                                                         double* __restrict__ aux) {
  const int k = blockIdx.x * kBootThreads + threadIdx.x;
  if (k >= n) return;
  const int cnt = n_rows[k];
  if (cnt <= 0) return;  // no row (or not in FIRST_SCAN): the stream's record keeps its bits
  const V3 ba{tmpl[kTmplBa], tmpl[kTmplBa + 1], tmpl[kTmplBa + 2]}, bg{tmpl[kTmplBw], tmpl[kTmplBw + 1], tmpl[kTmplBw + 2]};
  Pre r = pre_load(pre + (size_t)k * kPre);
  double time = aux[(size_t)k * kAux + kAuxTime];
  for (int it = 0; it < cnt; ++it) {
    const double* c = rows + (size_t)it * 7 * n + k;  // component j of this row: c[j * n]
    const double dt = c[0];
    pre_step(r, dt, V3{c[(size_t)n], c[(size_t)2 * n], c[(size_t)3 * n]}, V3{c[(size_t)4 * n], c[(size_t)5 * n], c[(size_t)6 * n]}, ba, bg);
    time += dt;
  }
  pre_store(r, pre + (size_t)k * kPre);
  aux[(size_t)k * kAux + kAuxTime] = time;
}

// list[i]: the stream of the i-th second scan; row i of state_in is what the batched ICP launch reads for it
__global__ __launch_bounds__(kBootThreads) void boot_start_kernel(int m, const int* __restrict__ list, const double* __restrict__ pre,
                                                                  double* __restrict__ state_in) {
  const int i = blockIdx.x * kBootThreads + threadIdx.x;
  if (i >= m) return;
  store(start_row(pre_load(pre + (size_t)list[i] * kPre)), state_in + (size_t)i * 19);
}

// mode[k]: 0 nothing, 1 first scan, 2 second scan (icp_slot[k]: its row of icp_state);  scan[k]: imu_last_ (acc, gyr) and
// the scan's time, 8 doubles per stream
__global__ __launch_bounds__(kBootThreads) void boot_finish_kernel(int n, const int* __restrict__ mode, const int* __restrict__ icp_slot,
                                                                   const double* __restrict__ icp_state, const double* __restrict__ scan,
                                                                   const double* __restrict__ tmpl, double* __restrict__ pre,
                                                                   double* __restrict__ state, double* __restrict__ cov,
                                                                   double* __restrict__ noise, double* __restrict__ aux,
                                                                   double* __restrict__ gstate, double* __restrict__ lin) {
  const int k = blockIdx.x, tid = threadIdx.x;
  if (k >= n) return;
  const int m = mode[k];
  if (m == 0) return;
  // initializeCovariance(0) and noise_ (KF:247-311): the template
  for (int o = tid; o < 324; o += kBootThreads) cov[(size_t)k * 324 + o] = tmpl[kTmplCov + o];
  for (int o = tid; o < 144; o += kBootThreads) noise[(size_t)k * 144 + o] = tmpl[kTmplNoise + o];
  if (tid != 0) return;
  const double* sc = scan + (size_t)k * 8;
  const V3 acc{sc[0], sc[1], sc[2]}, gyr{sc[3], sc[4], sc[5]};
  double* a = aux + (size_t)k * kAux;
  a[kAuxAcc] = acc.x, a[kAuxAcc + 1] = acc.y, a[kAuxAcc + 2] = acc.z;
  a[kAuxGyr] = gyr.x, a[kAuxGyr + 1] = gyr.y, a[kAuxGyr + 2] = gyr.z;
  a[kAuxTime] = sc[6], a[kAuxHasImu] = 1.0;
  for (int i = 0; i < 3; ++i) a[kAuxPosVar + i] = tmpl[kTmplPosVar + i], a[kAuxAttVar + i] = tmpl[kTmplAttVar + i];
  a[14] = 0.0, a[15] = 0.0;
  if (m == 1) {
    store(identity_state(), state + (size_t)k * 19);
    store(identity_state(), lin + (size_t)k * 19);
    pre_store(pre_reset(acc, gyr), pre + (size_t)k * kPre);
  } else {
    const double* is = icp_state + (size_t)icp_slot[k] * 19;
    const V3 ba{tmpl[kTmplBa], tmpl[kTmplBa + 1], tmpl[kTmplBa + 2]}, bw{tmpl[kTmplBw], tmpl[kTmplBw + 1], tmpl[kTmplBw + 2]};
    const Second o = second_scan(V3{is[0], is[1], is[2]}, Q4{is[6], is[7], is[8], is[9]}, pre[(size_t)k * kPre], acc, ba, bw);
    store(o.filter, state + (size_t)k * 19);
    store(o.global, gstate + (size_t)k * 19);
    store(o.lin, lin + (size_t)k * 19);
  }
}

}  // namespace

void launch_boot_preintegrate(hipStream_t stream, int n, const int* n_rows, const double* rows, const double* tmpl, double* pre, double* aux) {
  hipLaunchKernelGGL(boot_preintegrate_kernel, dim3((n + kBootThreads - 1) / kBootThreads), dim3(kBootThreads), 0, stream, n, n_rows, rows, tmpl, pre, aux);
}
void launch_boot_start(hipStream_t stream, int m, const int* list, const double* pre, double* state_in) {
  if (m <= 0) return;
  hipLaunchKernelGGL(boot_start_kernel, dim3((m + kBootThreads - 1) / kBootThreads), dim3(kBootThreads), 0, stream, m, list, pre, state_in);
}
void launch_boot_finish(hipStream_t stream, int n, const int* mode, const int* icp_slot, const double* icp_state, const double* scan, const double* tmpl,
                        double* pre, double* state, double* cov, double* noise, double* aux, double* gstate, double* lin) {
  hipLaunchKernelGGL(boot_finish_kernel, dim3(n), dim3(kBootThreads), 0, stream, n, mode, icp_slot, icp_state, scan, tmpl, pre, state, cov, noise, aux,
                     gstate, lin);
}

}  // namespace lins
