// team_graph_kernels.hip — the team graph's solve on the device (include/lins_team.h lins_team_graph_solve).  The text is
// pose_graph_team.h's, shared with the CPU restatement: a GROUP of robots is one workgroup of lins_pg::kThreads lanes, a
// phase is `fn(lane); __syncthreads();`.  f64 throughout, contraction off.  The group's concatenated rows, S and the loop
// records live in the team workspace in global memory; LDS holds the phase scratch and the group's member table.  Every
// loop bound in front of a barrier is the group's own (n_members, n_frames, n_loops, the member table's counts) and so
// uniform over the workgroup; there is no return in front of a barrier.
#include <hip/hip_runtime.h>

#include "lins_launch.h"
#include "pose_graph_team.h"

using namespace lins_pg;

namespace {

struct DevExec {  // a phase on the device
  template <class F>
  __device__ __forceinline__ void operator()(F f) const {
    f((int)threadIdx.x);
    __syncthreads();
  }
};

// the group's member table into LDS (n_members <= kTeamMaxMembers is the launcher's caller's check)
__device__ __forceinline__ void load_members(const TeamProb& G, TeamMember* mt) {
  const int nm = G.n_members < kTeamMaxMembers ? G.n_members : kTeamMaxMembers;
  for (int m = (int)threadIdx.x; m < nm; m += kThreads) mt[m] = G.members[m];
  __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(kThreads) void team_graph_begin_kernel(const TeamProb* __restrict__ probs) {
  __shared__ double sh[kTeamShared];
  __shared__ TeamMember mt[kTeamMaxMembers];
  const TeamProb G = probs[blockIdx.x];
  load_members(G, mt);
  team_begin(DevExec{}, G, mt, sh);
}

__global__ __launch_bounds__(kThreads) void team_graph_trial_kernel(const TeamProb* __restrict__ probs, lins_pose_graph_params prm,
                                                                    int* __restrict__ still_running) {
  __shared__ double sh[kTeamShared];
  __shared__ TeamMember mt[kTeamMaxMembers];
  const TeamProb G = probs[blockIdx.x];
  // (every lane reads the word before lane 0 of this workgroup can write it: that is behind the trial's barriers)
  if (G.st->active) {
    load_members(G, mt);
    team_trial(DevExec{}, G, mt, prm, sh);
    if (threadIdx.x == 0 && G.st->active && still_running) atomicAdd(still_running, 1);
  }
}

// One workgroup per member.  gather: the member's Z and D rows into the group's rows, the root row of D from the prior
// (the root's estimate starts at its measurement; the anchor's is never read).  scatter: the solved D rows 1 .. n - 1 and
// the T rows back, and with root != 0 the solved root into the member's prior row Z[0].
__global__ __launch_bounds__(kThreads) void team_graph_copy_kernel(const TeamCopy* __restrict__ recs, int scatter) {
  const TeamCopy c = recs[blockIdx.x];
  const int n12 = 12 * c.n;
  if (!scatter) {
    for (int i = (int)threadIdx.x; i < n12; i += kThreads) {
      c.gZ[i] = c.mZ[i];
      c.gD[i] = i < 12 ? c.mZ[i] : c.mD[i];
    }
  } else if (c.store) {
    for (int i = (int)threadIdx.x; i < n12; i += kThreads) {
      if (i >= 12) c.mD[i] = c.gD[i];
      else if (c.root) c.mZ[i] = c.gD[i];
      c.mT[i] = c.gT[i];
    }
  }
}

namespace lins {

void launch_team_graph_begin(hipStream_t s, int n_groups, const TeamProb* probs) {
  hipLaunchKernelGGL(team_graph_begin_kernel, dim3(n_groups), dim3(kThreads), 0, s, probs);
}
void launch_team_graph_trial(hipStream_t s, int n_groups, const TeamProb* probs, const lins_pose_graph_params& prm, int* still_running) {
  hipLaunchKernelGGL(team_graph_trial_kernel, dim3(n_groups), dim3(kThreads), 0, s, probs, prm, still_running);
}
void launch_team_graph_copy(hipStream_t s, int n_members, const TeamCopy* recs, bool scatter) {
  hipLaunchKernelGGL(team_graph_copy_kernel, dim3(n_members), dim3(kThreads), 0, s, recs, scatter ? 1 : 0);
}

}  // namespace lins
