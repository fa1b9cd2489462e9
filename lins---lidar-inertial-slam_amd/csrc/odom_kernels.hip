// odom_kernels.hip — the seam between the streams' filter and their mapping step, on the device (DESIGN.md §5.3 "Streams
// end to end"; scalar text: odom_math.h).
//
// odom_record_kernel   per stream, from the resident globalState_ row: globalStateYZX_ as publishOdometryYZX sends it
//                      (SE:1150-1154, EC:294-305) and the mapping node's transformSum (LM:711-724) — one record per
//                      stream, valid = 0 where the stream has no globalState_ yet or it is not finite.
// odom_fuse_kernel     the transform fusion node (TF:91-254) per entry: transformMapped from the resident
//                      transformBefMapped / transformAftMapped of the entry's stream and its record's transformSum, and the
//                      published orientation.  Reads only.
// One lane per stream / entry, no LDS, no cross-lane operation: a lane beyond n does nothing.  Every store is a vector store.
#include <hip/hip_runtime.h>

#include "lins_launch.h"
#include "odom_math.h"

namespace lins {
namespace {

constexpr int kOdomThreads = 64;

__global__ __launch_bounds__(kOdomThreads) void odom_record_kernel(int n, const double* __restrict__ gstate, const int* __restrict__ has,
                                                                   lins_stream_odom* __restrict__ recs) {
  const int k = blockIdx.x * kOdomThreads + threadIdx.x;
  if (k < n) {
    double gs[19];
#pragma unroll
    for (int i = 0; i < 19; ++i) gs[i] = gstate[(size_t)k * 19 + i];
    lins_stream_odom r;
    lins_od::odom_record(gs, has[k], &r);
    recs[k] = r;
  }
}

__global__ __launch_bounds__(kOdomThreads) void odom_fuse_kernel(int n, const int* __restrict__ list, const MapPoseRec* __restrict__ poses,
                                                                 const lins_stream_odom* __restrict__ recs, lins_fused_pose* __restrict__ out) {
  const int k = blockIdx.x * kOdomThreads + threadIdx.x;
  if (k < n) {
    const int s = list[k];
    float bef[6], aft[6], sum[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) bef[i] = poses[s].bef[i], aft[i] = poses[s].aft[i], sum[i] = recs[s].transform_sum[i];
    lins_fused_pose f;
    lins_od::odom_fuse(bef, aft, sum, &f);
    out[k] = f;
  }
}

}  // namespace

void launch_odom_records(hipStream_t stream, int n, const double* gstate, const int* has, lins_stream_odom* recs) {
  hipLaunchKernelGGL(odom_record_kernel, dim3((n + kOdomThreads - 1) / kOdomThreads), dim3(kOdomThreads), 0, stream, n, gstate, has, recs);
}
void launch_odom_fuse(hipStream_t stream, int n, const int* list, const MapPoseRec* poses, const lins_stream_odom* recs, lins_fused_pose* out) {
  hipLaunchKernelGGL(odom_fuse_kernel, dim3((n + kOdomThreads - 1) / kOdomThreads), dim3(kOdomThreads), 0, stream, n, list, poses, recs, out);
}

}  // namespace lins
