// lins_records.h — the records the host fills (or reads) and the kernels read (or fill): ONE definition each, plain
// host + device C++.  The kernel files and the C API files both include it, so a launcher takes a typed pointer and a
// changed field is a compile error on the other side, not a layout that no longer matches.
#pragma once

#include "../../include/lins_host.h"

namespace lins {

struct OutRec {  // what an update leaves per scan besides the posterior (every IESKF kernel family)
  double residual_norm, update_norm;
  int iters, converged, diverged, m_surf, m_corner, pad[3];
};
static_assert(sizeof(OutRec) == 48, "OutRec layout");

// The carry records of the batch kernel's queries (ieskf_lds_impl.h KernelArgs::relay_lane, ieskf_lds_lean.h): what the
// context allocates per scan and the kernels index by.
constexpr int kRelayLanes = 512;                       // query slots of a scan's carry records
constexpr int kRelayRegionInts = 4 * kRelayLanes * 4;  // ints per scan in KernelArgs::relay_lane: [4][512] 16-byte words, by QUERY slot
constexpr int kRelayLaneInts = kRelayRegionInts;

struct FeScan {  // device view of one lins_segmented_scan + its outputs (frontend_kernels.hip; head filled by segment_kernels.hip)
  long long off;     // first point in the point / range / col / ground arenas
  int n;
  int start_ring[LINS_LINE_NUM], end_ring[LINS_LINE_NUM];
  float start_ori, end_ori, ori_diff;
  int pad;
  long long o_sharp, o_less_sharp, o_flat, o_less_flat;  // where the four feature clouds go (points from `out`)
};
static_assert(sizeof(FeScan) == 192, "FeScan layout");

struct SgRaw {  // one raw cloud of the image_projection stage (segment_kernels.hip)
  long long off;  // first raw point of the scan
  int n;
  int o_slot;     // slot of the outlier arena this scan's outlier cloud goes to (launch_segment)
};
static_assert(sizeof(SgRaw) == 16, "SgRaw layout");

struct ReprojectJob {  // one cloud of lins_transform_to_end_batch (ieskf_kernels.hip)
  long long off;  // first point of the cloud in the in / out arenas
  int n, has_yzx;
  double t[3], q[4];
  double inv_period;
};
static_assert(sizeof(ReprojectJob) == 80, "ReprojectJob layout");

struct StreamCloud {  // one resident cloud of the in-place re-projection (lins_streams_step)
  long long off;  // first point in the stream arena
  int n, stream;  // points, index of the state to use
};
static_assert(sizeof(StreamCloud) == 16, "StreamCloud layout");

// ---- scan-to-map row (map_kernels.hip / lins_map_capi.hip); MapRoundParams and LmCarry live in lm_math.h ----
struct MapGrid {  // one cloud of one problem
  long long off_pts;    // first sorted point (x, y, z, original index bits) in the point arena
  long long off_cells;  // first of (ncell + 1) cell starts in the cell arena (positions relative to off_pts)
  int cmin[3], cdim[3];
};
struct MapDev {  // one problem
  MapGrid g[2];      // 0 corner map, 1 surf map
  long long off_q;   // queries: corner scan points, then surf scan points
  long long off_rec; // lins_map_corr records, same order
  int n_q[2];
  int active;        // 0: finished / precondition not met — its blocks return at once
  int pad;
};
static_assert(sizeof(MapDev) == 112, "MapDev layout");
struct MapGridJob {
  long long off_raw;   // raw points of this cloud in the staging arena
  long long off_pts;   // sorted points
  long long off_cells; // ncell + 1 starts (relative to off_pts), followed by ncell + 1 scratch cursors
  int n, ncell;
  int cmin[3], cdim[3];
};
static_assert(sizeof(MapGridJob) == 56, "MapGridJob layout");

// ---- the mapping node's step for streams (map_pose_kernels.hip / lins_streams_map_capi.hip) ----
struct MapPoseRec {  // one stream's resident map pose: lins_map_pose_state without the host's last_time
  float bef[6], aft[6], tobe[6], last[6], prev[3];
  int n_frames;
};
static_assert(sizeof(MapPoseRec) == 112, "MapPoseRec layout");
struct MapPoseEntry {  // one entry of a step's batch (uploaded per call)
  float sum[6];
  float imu_roll, imu_pitch;
  int has_imu;
  int stream;  // the MapPoseRec it works on
};
static_assert(sizeof(MapPoseEntry) == 40, "MapPoseEntry layout");
struct MapPoseFix {  // one entry of a write-back's batch (lins_pose_graph_apply_batch): the newest pose of a slot's graph
  int stream;  // the MapPoseRec it goes to
  float p[6];  // aft = last = tobe (LM:1737-1749)
  int pad;
};
static_assert(sizeof(MapPoseFix) == 32, "MapPoseFix layout");

}  // namespace lins
