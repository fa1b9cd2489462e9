// pose_graph_kernels.hip — the pose graph's solve on the device (include/lins_map.h lins_pose_graph_solve).  The text of
// the solve is pose_graph.h's, shared with the CPU restatement: a problem is one workgroup of lins_pg::kThreads lanes,
// a phase is `fn(lane); __syncthreads();`.  f64 throughout, contraction off.  The graphs, S and the per-frame blocks live
// in global memory sized at init; LDS holds the phase scratch (the chunk sums of the span being reduced, the 6 x 6 sum,
// the lanes' partial costs).  Every loop bound in front of a barrier is the problem's (n_frames, n_loops) and so uniform
// over the workgroup; there is no return in front of a barrier.
#include <hip/hip_runtime.h>

#include "lins_launch.h"
#include "pose_graph.h"

using namespace lins_pg;

namespace {

struct DevExec {  // a phase on the device
  template <class F>
  __device__ __forceinline__ void operator()(F f) const {
    f((int)threadIdx.x);
    __syncthreads();
  }
};

}  // namespace

__global__ __launch_bounds__(kThreads) void pose_graph_begin_kernel(const Prob* __restrict__ probs) {
  __shared__ double sh[kShared];
  const Prob P = probs[blockIdx.x];
  solve_begin(DevExec{}, P, sh);
}

__global__ __launch_bounds__(kThreads) void pose_graph_trial_kernel(const Prob* __restrict__ probs, lins_pose_graph_params prm,
                                                                    int* __restrict__ still_running) {
  __shared__ double sh[kShared];
  const Prob P = probs[blockIdx.x];
  // (every lane reads the word before lane 0 of this workgroup can write it: that is behind the trial's barriers)
  if (P.st->active) {
    solve_trial(DevExec{}, P, prm, sh);
    if (threadIdx.x == 0 && P.st->active && still_running) atomicAdd(still_running, 1);
  }
}

namespace lins {

void launch_pose_graph_begin(hipStream_t s, int n_problems, const Prob* probs) {
  hipLaunchKernelGGL(pose_graph_begin_kernel, dim3(n_problems), dim3(kThreads), 0, s, probs);
}
void launch_pose_graph_trial(hipStream_t s, int n_problems, const Prob* probs, const lins_pose_graph_params& prm, int* still_running) {
  hipLaunchKernelGGL(pose_graph_trial_kernel, dim3(n_problems), dim3(kThreads), 0, s, probs, prm, still_running);
}

}  // namespace lins
