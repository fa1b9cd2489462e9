// keyframe_archive.cpp — the key-frame archive's selection and assembly on the CPU (include/lins_host.h
// lins_host_select_radius / _find_loop / _submap): the restatement lins_archive_assemble (archive_kernels.hip) is checked
// against, bit for bit.
//   publishGlobalMap    LM:984-1031   radius search + VoxelGrid of the key poses -> frames; corner, surf, outlier of each
//                                     into the map frame (transformPointCloud, LM:654-686), VoxelGrid 0.4 m
//   detectLoopClosure   LM:1043-1112  the candidate rule; latest corner + surf without (int)intensity < 0; the +-25 frames
//                                     around the candidate, corner + surf, VoxelGrid 0.4 m
// The selection is host/keyframe_select.h (one definition for both libraries); transform and VoxelGrid are voxel_map.h.
#include <vector>

#include "../../../include/lins_host.h"
#include "keyframe_select.h"
#include "voxel_map.h"

using namespace lins_hostmap;

extern "C" int lins_host_select_radius(const lins_key_pose* poses, int n, const float centre[3], float radius, float pose_leaf,
                                       int32_t* ids, int cap) {
  if (n < 0 || (n && !poses) || cap < 0 || !lins_select::query_ok(centre, radius) || !(pose_leaf > 0.f)) return LINS_E_ARG;
  for (int i = 0; i < n; ++i)
    if (!pose_ok(poses[i])) return LINS_E_INPUT;
  std::vector<int> sel;
  if (!lins_select::select_radius(poses, n, centre, radius, pose_leaf, sel)) return LINS_E_CAPACITY;
  if ((int)sel.size() > cap) return LINS_E_CAPACITY;
  if (!sel.empty() && !ids) return LINS_E_ARG;
  for (size_t i = 0; i < sel.size(); ++i) ids[i] = sel[i];
  return (int)sel.size();
}

extern "C" int lins_host_find_loop(const lins_key_pose* poses, const double* times, int n, const float centre[3], float radius,
                                   double now, double min_gap_s, int32_t* closest) {
  if (n < 0 || (n && (!poses || !times)) || !lins_select::query_ok(centre, radius) || !closest) return LINS_E_ARG;
  for (int i = 0; i < n; ++i)
    if (!pose_ok(poses[i])) return LINS_E_INPUT;
  *closest = lins_select::find_loop(poses, times, n, centre, radius, now, min_gap_s);
  return LINS_OK;
}

extern "C" int lins_host_submap(const lins_keyframe* frames, int n_frames, const int32_t* ids, int n_ids, int clouds, float leaf,
                                int flags, lins_point* out, lins_submap_info* info) {
  const int all = LINS_SUBMAP_CORNER | LINS_SUBMAP_SURF | LINS_SUBMAP_OUTLIER;
  if (n_frames < 0 || (n_frames && !frames) || n_ids < 0 || (n_ids && !ids) || !info) return LINS_E_ARG;
  if (clouds <= 0 || (clouds & ~all) || (flags & ~LINS_SUBMAP_DROP_NEGATIVE) || !(leaf >= 0.f) || !std::isfinite(leaf)) return LINS_E_ARG;
  if ((flags & LINS_SUBMAP_DROP_NEGATIVE) && leaf != 0.f) return LINS_E_ARG;
  for (int i = 0; i < n_ids; ++i)
    if (ids[i] < 0 || ids[i] >= n_frames) return LINS_E_ARG;
  for (int i = 0; i < n_ids; ++i) {
    const lins_keyframe& f = frames[ids[i]];
    if (!cloud_ok(f.corner, f.n_corner) || !cloud_ok(f.surf, f.n_surf) || !cloud_ok(f.outlier, f.n_outlier) || !pose_ok(f.pose))
      return LINS_E_INPUT;
  }
  std::vector<lins_point> cat, res;
  for (int i = 0; i < n_ids; ++i) {  // within a frame always corner, surf, outlier (LM:1008-1015, 1070-1075, 1092-1097)
    const lins_keyframe& f = frames[ids[i]];
    const Trig t = trig_of(f.pose);
    if (clouds & LINS_SUBMAP_CORNER) transform_into(f.corner, f.n_corner, t, cat);
    if (clouds & LINS_SUBMAP_SURF) transform_into(f.surf, f.n_surf, t, cat);
    if (clouds & LINS_SUBMAP_OUTLIER) transform_into(f.outlier, f.n_outlier, t, cat);
  }
  *info = lins_submap_info{};
  info->frames = n_ids, info->points_in = cat.size();
  bool ok = true;
  for (const lins_point& p : cat) ok = ok && point_ok(p);
  if (!ok) {
    info->status = LINS_E_INPUT;
  } else if (leaf > 0.f) {
    if (!voxel_grid(cat, leaf, res)) info->status = LINS_E_CAPACITY, res.clear();
  } else if (flags & LINS_SUBMAP_DROP_NEGATIVE) {
    for (const lins_point& p : cat)
      if (keeps_nonnegative(p.intensity)) res.push_back(p);
  } else {
    res = cat;
  }
  info->n = (int32_t)res.size();
  if (!res.empty() && !out) return LINS_E_ARG;
  for (size_t i = 0; i < res.size(); ++i) out[i] = res[i];
  if (leaf > 0.f) {
    box_1m(res, info->box_min, info->box_dim);
  } else {
    for (int a = 0; a < 3; ++a) info->box_min[a] = 0, info->box_dim[a] = 1;
  }
  return LINS_OK;
}
