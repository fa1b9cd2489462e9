// local_map.h — the device records of the local-map build (local_map_kernels.hip, lins_local_map_capi.hip).
//
// A build runs VoxelGrid "jobs": per entry five in stage A (corner map, surf map, cornerDS, surfDS, outlierDS) and one
// in stage B (surfTotalDS over surfDS ++ outlierDS).  Job j owns [off_in, off_in + cap) of the staging arena (input
// points) and of the sort's key / value / run-start scratch, and [tile0, tile0 + ntiles) of its stage's tile grid.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lins_map.h"
#include "../../include/lins_streams_map.h"
#include "../../include/lins_streams_slam.h"

namespace lins {

constexpr int kLmTile = 512;   // points per tile = threads per workgroup of the tile kernels
constexpr int kLmDigit = 8;    // radix bits per pass
constexpr int kLmPasses = 4;   // keys < 2^31 need at most four 8-bit passes

struct LmJob {
  long long off_in;   // staging offset of the input points (and of the key / value / start scratch)
  long long off_out;  // output offset in the cloud arena
  int cap;            // upper bound of the input count (host-known)
  int tile0, ntiles;  // tiles of this job in its stage's grid (ntiles = ceil(cap / kLmTile))
  float inv;          // 1.0f / leaf, formed on the host as the restatement forms it
  int out_after;      // job whose voxel count is added to off_out (surfTotalDS behind cornerDS), -1: none
  int src_a, src_b;   // stage B: the jobs whose centroids are its input, -1: none
  int feed;           // stage A: the stage-B job this job's centroids also feed, -1: none
  int feed_after;     // ... written behind the centroids of this job, -1: at 0
  int map;            // 1: a map cloud — the 1 m box of its output is folded
  int pad;
};
static_assert(sizeof(LmJob) == 64, "LmJob layout");

struct LmState {      // written by the kernels, read back once per build
  unsigned mn[3], mx[3];  // f32 box of the input, order-preserving unsigned encoding (atomic min / max)
  int n;                  // input points
  int flags;              // bit 0: a transformed map point outside the input contract
  int minb[3];
  unsigned d0, d01;       // div0, div0 * div1
  int passes;             // radix passes this job needs
  int nvox;               // output points
  int status;             // 0, LINS_E_INPUT or LINS_E_CAPACITY
  int bmin[3], bmax[3];   // 1 m box of the output (map jobs)
};
static_assert(sizeof(LmState) == 88, "LmState layout");

struct LmSeg {  // one cloud of one window frame moved into the map frame
  long long src, dst;  // frame store offset, staging offset
  int n, job;
  float t[9];          // ctRoll, stRoll, ctPitch, stPitch, ctYaw, stYaw, tInX, tInY, tInZ
  int pad;
};
static_assert(sizeof(LmSeg) == 64, "LmSeg layout");

struct LmScanSeg {  // one scan cloud of one entry taken from a stream where it lies (lins_local_map_build_streams)
  const float4* src;   // the stream's cloud, sensor axes
  long long dst;       // staging offset (the job's off_in)
  int n, job;
};
static_assert(sizeof(LmScanSeg) == 24, "LmScanSeg layout");

inline __host__ __device__ unsigned lm_enc(float f) {  // order-preserving float -> unsigned
  unsigned u;
  __builtin_memcpy(&u, &f, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline __host__ __device__ float lm_dec(unsigned u) {
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// (host side) the clouds of the last build where scan-to-map reads them: cloud c of entry k starts at
// d_out + off[6 k + c] and holds sizes[k].n[c] points; cloud LINS_LOCAL_SCAN_TOTAL follows cloud LINS_LOCAL_SCAN_CORNER
// directly — the query layout of map_upload.  LINS_E_STATE when there was no build.
struct LocalMapView {
  const float4* d_out;
  int n;
  const long long* off;
  const lins_local_map_sizes* sizes;
  const int* slots;  // the slot of entry k
};
int local_map_view(lins_ctx* ctx, LocalMapView* v);
int local_map_slots(lins_ctx* ctx);  // n_slots of lins_local_map_init (0 before it)
int local_map_ring(lins_ctx* ctx, int slot, int* window);  // frames on the ring of slot (-1: no such slot) and the rings' window
// lins_map_capi.hip: what the scan-to-map state holds for the other mapping files and frees with itself, in this order —
// the local map (lins_local_map_capi.hip), the key-frame archive (lins_archive_capi.hip), the loop-closure ICP
// (lins_loop_icp_capi.hip), the streams' map poses (lins_streams_map_capi.hip), the pose graphs
// (lins_pose_graph_capi.hip), the loop thread's step (lins_loop_step_capi.hip)
enum MapSlot { kSlotLocal, kSlotArchive, kSlotLoop, kSlotPose, kSlotGraph, kSlotLoopStep, kSlotCount };
void** map_slot(lins_ctx* ctx, MapSlot which, void (*free_fn)(void*));

// lins_streams_map_capi.hip, for the write-back of a loop closure and the loop thread's step
int streams_map_streams(lins_ctx* ctx);  // streams of lins_streams_map_init (0 before it)
int streams_map_centre(lins_ctx* ctx, int stream, float centre[3]);  // currentRobotPosPoint; LINS_E_STATE: the stream has not completed a step
// aft = last = tobe = six[6 k ..] of streams[k] (each in range, at most once; n <= streams): one upload, one launch of
// map_pose_correct_kernel, one synchronisation
int streams_map_correct(lins_ctx* ctx, int n, const int32_t* streams, const float* six);
// lins_pose_graph_capi.hip: n_slots (0 before lins_pose_graph_init); of a slot in range the frames and loops it still
// takes and the pair of its most recent loop factor (-1, -1: none); every refusal of lins_pose_graph_apply_batch
int pose_graph_slots(lins_ctx* ctx);
void pose_graph_room(lins_ctx* ctx, int slot, int* frames_left, int* loops_left, int* last_latest, int* last_closest);
int pose_graph_apply_check(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* streams);

// lins_map_capi.hip: scan-to-map over the last local-map build (n entries, as LINS_MAP_LOCAL) between the two pose
// kernels of map_pose_kernels.hip — entry k works on d_poses[d_entries[k].stream]; h_out receives the n result records
// (pinned or pageable), one synchronisation.  ev: four events, recorded around the associate and the finish kernel.
// d_odom: null — transformSum is each entry's uploaded one —, or the resident records of lins_streams_odometry, indexed
// by stream, which the two pose kernels then read it from.
struct MapPoseEntry;  // lins_records.h
struct MapPoseRec;
int scan2map_local_resident(lins_ctx* ctx, int n, const MapPoseEntry* d_entries, MapPoseRec* d_poses, lins_map_step_result* d_out,
                            lins_map_step_result* h_out, hipEvent_t* ev, const lins_stream_odom* d_odom = nullptr);

// lins_streams_map_capi.hip: the body lins_streams_map_step and lins_streams_map_step_resident share.  An entry's
// transformSum, time and IMU angles come either from the caller's rows (odom) or — odom null — from the resident records
// (d_odom on the device, h_odom their host copy: an entry whose record is not valid gets LINS_E_INPUT and is left out of
// the batch), time[k] and imu[k] (imu may be null: no entry has IMU angles).
struct MapStepIn {
  const lins_map_odom* odom;
  const lins_stream_odom *d_odom, *h_odom;
  const double* time;
  const lins_slam_imu* imu;
};
int streams_map_step_run(lins_ctx* ctx, int n, const int32_t* streams, const MapStepIn& in, lins_map_step_result* out);
// the resident map poses (null before lins_streams_map_init), for the fusion kernel
const MapPoseRec* streams_map_poses(lins_ctx* ctx);

}  // namespace lins
