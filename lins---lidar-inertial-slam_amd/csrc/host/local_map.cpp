// local_map.cpp — the mapping node's local map on the CPU (include/lins_host.h lins_host_local_map): the restatement the
// device build of lins_local_map_build (local_map_kernels.hip) is checked against, bit for bit.
//   extractSurroundingKeyFrames  LM:1201-1324  last min(window, K) key frames -> map frame (transformPointCloud,
//                                              LM:627-650), concatenated oldest first, VoxelGrid 0.2 / 0.4 m
//                                              (each frame once: where the node's deque doubles its newest frame,
//                                              LM:1225-1239 with a stale latestFrameID, is a stated departure,
//                                              include/lins_map.h; the caller may pass any list of frames)
//   downsampleCurrentScan        LM:1326-1349  corner 0.2, surf 0.4, outlier 0.4, surfTotal = 0.4 of (surfDS ++ outlierDS)
// VoxelGrid is the contract of frontend.cpp's voxel_grid with the leaf as an argument.
#include <algorithm>
#include <vector>

#include "../../../include/lins_host.h"
#include "voxel_map.h"  // the contract checks, transformPointCloud and VoxelGrid, shared with the archive's restatement

using namespace lins_hostmap;

extern "C" int lins_host_local_map(const lins_keyframe* frames, int n_frames, int window, const lins_local_scan* scan,
                                   lins_point* const* out, lins_local_map_sizes* sizes) {
  if (n_frames < 0 || (n_frames && !frames) || window < 1 || !scan || !out || !sizes) return LINS_E_ARG;
  const int k0 = std::max(0, n_frames - window);
  for (int k = k0; k < n_frames; ++k) {
    const lins_keyframe& f = frames[k];
    if (!cloud_ok(f.corner, f.n_corner) || !cloud_ok(f.surf, f.n_surf) || !cloud_ok(f.outlier, f.n_outlier) || !pose_ok(f.pose))
      return LINS_E_INPUT;
  }
  if (!cloud_ok(scan->corner, scan->n_corner) || !cloud_ok(scan->surf, scan->n_surf) || !cloud_ok(scan->outlier, scan->n_outlier))
    return LINS_E_INPUT;
  std::vector<lins_point> cat[2], res[6];
  for (int k = k0; k < n_frames; ++k) {  // LM:1242-1246: corner_i; surf_i then outlier_i
    const lins_keyframe& f = frames[k];
    const Trig t = trig_of(f.pose);
    transform_into(f.corner, f.n_corner, t, cat[0]);
    transform_into(f.surf, f.n_surf, t, cat[1]);
    transform_into(f.outlier, f.n_outlier, t, cat[1]);
  }
  *sizes = lins_local_map_sizes{};
  sizes->frames = n_frames - k0;
  bool ok = true;
  for (int c = 0; c < 2; ++c)
    for (const lins_point& p : cat[c]) ok = ok && point_ok(p);
  if (!ok) sizes->status = LINS_E_INPUT;
  if (ok) {
    const std::vector<lins_point> sc(scan->corner, scan->corner + scan->n_corner), ss(scan->surf, scan->surf + scan->n_surf),
        so(scan->outlier, scan->outlier + scan->n_outlier);
    ok = voxel_grid(cat[0], 0.2f, res[0]) && voxel_grid(cat[1], 0.4f, res[1]) && voxel_grid(sc, 0.2f, res[2]) &&
         voxel_grid(ss, 0.4f, res[3]) && voxel_grid(so, 0.4f, res[4]);
    if (ok) {
      std::vector<lins_point> total(res[3]);
      total.insert(total.end(), res[4].begin(), res[4].end());
      ok = voxel_grid(total, 0.4f, res[5]);
    }
    if (!ok) sizes->status = LINS_E_CAPACITY;
  }
  for (int c = 0; c < 6; ++c) {
    if (!ok) res[c].clear();
    sizes->n[c] = (int32_t)res[c].size();
    if (!res[c].empty()) std::copy(res[c].begin(), res[c].end(), out[c]);
  }
  for (int w = 0; w < 2; ++w) box_1m(res[w], sizes->box_min[w], sizes->box_dim[w]);
  return LINS_OK;
}
