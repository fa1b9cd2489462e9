// map_pose_kernels.hip — the mapping node's own pose arithmetic around scan-to-map, for streams (DESIGN.md §5.3
// "Mapping node's step"; scalar text: map_pose_math.h).
//
// map_associate_kernel     transformAssociateToMap (LM:411-536): per entry, from the resident transformBefMapped /
//                          transformAftMapped of the entry's stream and transformSum — the entry's uploaded one, or with
//                          `odom` the resident record's of the entry's stream (odom_kernels.hip) —, transformTobeMapped —
//                          into the pose record, into the step's result record (tobe_start) and into the scan-to-map
//                          result record the rounds start from (transform; counters zeroed).
// map_pose_finish_kernel   behind the last round: transformUpdate's tail (LM:567-576) where the precondition of LM:1636
//                          held, the key-frame rule (LM:1655-1671) and the key pose with iSAM2 as the identity
//                          (LM:1676-1686, 1699-1704, 1737-1749); one result record per entry.
// map_pose_correct_kernel  a loop closure's write-back (LM:1737-1749): per entry, transformAftMapped = transformLast =
//                          transformTobeMapped = the uploaded newest pose of the entry's stream; the rest of the record stays.
// One lane per entry, no LDS, no cross-lane operation: a lane beyond n does nothing.  MapDev::pad of an entry carries
// what the host knew when it queued the rounds: < 0 the build entry's status (nothing is touched), 1 the precondition
// of LM:1636 held, 0 it did not (null probs: 0).  Every store is a vector store.
#include <hip/hip_runtime.h>

#include "lins_launch.h"
#include "map_pose_math.h"

namespace lins {
namespace {

using namespace lins_mp;

constexpr int kPoseThreads = 64;

__global__ __launch_bounds__(kPoseThreads) void map_associate_kernel(int n, const MapPoseEntry* __restrict__ entries, const MapDev* __restrict__ probs,
                                                                     MapPoseRec* __restrict__ poses, lins_map_result* __restrict__ results,
                                                                     lins_map_step_result* __restrict__ out, const lins_stream_odom* __restrict__ odom) {
  const int k = blockIdx.x * kPoseThreads + threadIdx.x;
  if (k < n) {
    const MapPoseEntry e = entries[k];
    const int flag = probs ? probs[k].pad : 0;
    MapPoseRec* rec = poses + e.stream;
    float bef[6], aft[6], sum[6], tobe[6];
    const float* src = odom ? odom[e.stream].transform_sum : e.sum;
#pragma unroll
    for (int i = 0; i < 6; ++i) bef[i] = rec->bef[i], aft[i] = rec->aft[i], sum[i] = src[i];
    mp_associate(bef, aft, sum, tobe);
#pragma unroll
    for (int i = 0; i < 6; ++i) out[k].tobe_start[i] = tobe[i];
    if (flag >= 0) {
#pragma unroll
      for (int i = 0; i < 6; ++i) rec->tobe[i] = tobe[i];
    }
    if (results) {
      lins_map_result r;
#pragma unroll
      for (int i = 0; i < 6; ++i) r.transform[i] = tobe[i];
      r.iters = 0, r.converged = 0, r.degenerate = 0, r.n_sel = 0;
      results[k] = r;
    }
  }
}

__global__ __launch_bounds__(kPoseThreads) void map_pose_finish_kernel(int n, const MapPoseEntry* __restrict__ entries, const MapDev* __restrict__ probs,
                                                                       MapPoseRec* __restrict__ poses, const lins_map_result* __restrict__ results,
                                                                       lins_map_step_result* __restrict__ out, const lins_stream_odom* __restrict__ odom) {
  const int k = blockIdx.x * kPoseThreads + threadIdx.x;
  if (k < n) {
    const MapPoseEntry e = entries[k];
    float sum[6];
    const float* src = odom ? odom[e.stream].transform_sum : e.sum;
#pragma unroll
    for (int i = 0; i < 6; ++i) sum[i] = src[i];
    const int flag = probs[k].pad;
    const lins_map_result r = results[k];
    lins_map_step_result o = out[k];  // (tobe_start is the associate kernel's)
    o.iters = r.iters, o.converged = r.converged, o.degenerate = r.degenerate, o.n_sel = r.n_sel;
    o.key_frame = 0, o.ring_age = -1, o.archive_id = -1;
    MapPoseRec rec = poses[e.stream];
    if (flag < 0) {  // the build refused the entry: its status, the pose as it was
      o.status = flag;
      o.iters = 0, o.converged = 0, o.degenerate = 0, o.n_sel = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) o.transform[i] = rec.aft[i], o.key_pose[i] = 0.f;
    } else {
      o.status = LINS_OK;
#pragma unroll
      for (int i = 0; i < 6; ++i) rec.tobe[i] = r.transform[i];
      if (flag > 0) mp_transform_update(rec.tobe, e.has_imu, e.imu_roll, e.imu_pitch, sum, rec.bef, rec.aft);
      float key[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (mp_key_rule(rec.prev, rec.aft, rec.n_frames > 0)) {
        mp_key_pose(rec.tobe, rec.aft, rec.last, &rec.n_frames, key);
        o.key_frame = 1;
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) o.transform[i] = rec.aft[i], o.key_pose[i] = key[i];
      poses[e.stream] = rec;
    }
    out[k] = o;
  }
}

__global__ __launch_bounds__(kPoseThreads) void map_pose_correct_kernel(int n, const MapPoseFix* __restrict__ fixes, MapPoseRec* __restrict__ poses) {
  const int k = blockIdx.x * kPoseThreads + threadIdx.x;
  if (k < n) {
    const MapPoseFix f = fixes[k];
    MapPoseRec* rec = poses + f.stream;
#pragma unroll
    for (int i = 0; i < 6; ++i) rec->aft[i] = f.p[i], rec->last[i] = f.p[i], rec->tobe[i] = f.p[i];
  }
}

}  // namespace

void launch_map_associate(hipStream_t stream, int n, const MapPoseEntry* entries, const MapDev* probs, MapPoseRec* poses, lins_map_result* results,
                          lins_map_step_result* out, const lins_stream_odom* odom) {
  hipLaunchKernelGGL(map_associate_kernel, dim3((n + kPoseThreads - 1) / kPoseThreads), dim3(kPoseThreads), 0, stream, n, entries, probs, poses,
                     results, out, odom);
}
void launch_map_pose_finish(hipStream_t stream, int n, const MapPoseEntry* entries, const MapDev* probs, MapPoseRec* poses,
                            const lins_map_result* results, lins_map_step_result* out, const lins_stream_odom* odom) {
  hipLaunchKernelGGL(map_pose_finish_kernel, dim3((n + kPoseThreads - 1) / kPoseThreads), dim3(kPoseThreads), 0, stream, n, entries, probs, poses,
                     results, out, odom);
}

void launch_map_pose_correct(hipStream_t stream, int n, const MapPoseFix* fixes, MapPoseRec* poses) {
  hipLaunchKernelGGL(map_pose_correct_kernel, dim3((n + kPoseThreads - 1) / kPoseThreads), dim3(kPoseThreads), 0, stream, n, fixes, poses);
}

}  // namespace lins
