// keyframe_archive.cpp — the key-frame archive's selection and assembly on the CPU (include/lins_host.h
// lins_host_select_radius / _find_loop / _submap / _surround_update / _surround_map): the restatement lins_archive_assemble (archive_kernels.hip) is checked
// against, bit for bit.
//   publishGlobalMap    LM:984-1031   radius search + VoxelGrid of the key poses -> frames; corner, surf, outlier of each
//                                     into the map frame (transformPointCloud, LM:654-686), VoxelGrid 0.4 m
//   detectLoopClosure   LM:1043-1112  the candidate rule; latest corner + surf without (int)intensity < 0; the +-25 frames
//                                     around the candidate, corner + surf, VoxelGrid 0.4 m
//   extractSurroundingKeyFrames, loop closure off  LM:1247-1315  the list rule (keyframe_select.h surround_update); the
//                                     map clouds are two submaps over the list, the scan clouds the local map's
//   the team map (no counterpart in the node)     the selection over the slots of a team (host/team_select.h) and the
//                                     surround map over a list of (slot, id) pairs: lins_host_team_select / _team_map
// The selection is host/keyframe_select.h (one definition for both libraries); transform and VoxelGrid are voxel_map.h.
#include <vector>

#include "../../../include/lins_host.h"
#include "keyframe_select.h"
#include "team_select.h"
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

extern "C" int lins_host_surround_update(int32_t* list, int n_list, int cap, const int32_t* ds, int n_ds) {
  if (n_list < 0 || cap < n_list || (n_list && !list) || n_ds < 0 || (n_ds && !ds)) return LINS_E_ARG;
  std::vector<int> l(list, list + n_list);
  lins_select::surround_update(l, std::vector<int>(ds, ds + n_ds));
  if ((int)l.size() > cap) return LINS_E_CAPACITY;
  if (!l.empty() && !list) return LINS_E_ARG;
  for (size_t i = 0; i < l.size(); ++i) list[i] = l[i];
  return (int)l.size();
}

extern "C" int lins_host_surround_map(const lins_keyframe* frames, int n_frames, const int32_t* list, int n_list,
                                      const lins_local_scan* scan, lins_point* const* out, lins_local_map_sizes* sizes) {
  if (n_frames < 0 || (n_frames && !frames) || n_list < 0 || (n_list && !list) || !scan || !out || !sizes) return LINS_E_ARG;
  for (int i = 0; i < n_list; ++i)
    if (list[i] < 0 || list[i] >= n_frames) return LINS_E_ARG;
  // the two map clouds first (they refuse a frame outside the input contract before anything is written) ...
  lins_submap_info info[2];
  const int clouds[2] = {LINS_SUBMAP_CORNER, LINS_SUBMAP_SURF | LINS_SUBMAP_OUTLIER};
  const float leaf[2] = {0.2f, 0.4f};
  std::vector<lins_point> map[2];
  for (int w = 0; w < 2; ++w) {
    size_t room = 0;
    for (int i = 0; i < n_list; ++i) {
      const lins_keyframe& f = frames[list[i]];
      if (f.n_corner < 0 || f.n_surf < 0 || f.n_outlier < 0) return LINS_E_INPUT;
      room += w ? (size_t)f.n_surf + f.n_outlier : (size_t)f.n_corner;
    }
    map[w].resize(room + 1);
    if (int rc = lins_host_submap(frames, n_frames, list, n_list, clouds[w], leaf[w], 0, map[w].data(), &info[w])) return rc;
  }
  // ... then the scan's four clouds: the local map over no frames
  lins_local_map_sizes z;
  if (int rc = lins_host_local_map(nullptr, 0, 1, scan, out, &z)) return rc;
  z.frames = n_list;
  for (int w = 0; w < 2; ++w)  // an entry's status as the build folds it: LINS_E_INPUT first, else the first one set
    if (info[w].status == LINS_E_INPUT || (info[w].status && !z.status)) z.status = info[w].status;
  for (int w = 0; w < 2; ++w) {
    z.n[w] = z.status ? 0 : info[w].n;
    if (z.n[w]) std::copy(map[w].begin(), map[w].begin() + z.n[w], out[w]);
    for (int a = 0; a < 3; ++a) z.box_min[w][a] = z.n[w] ? info[w].box_min[a] : 0, z.box_dim[w][a] = z.n[w] ? info[w].box_dim[a] : 1;
  }
  if (z.status)
    for (int c = 2; c < 6; ++c) z.n[c] = 0;
  *sizes = z;
  return LINS_OK;
}

extern "C" int lins_host_team_select(int n_targets, const int32_t* slots, const lins_key_pose* const* poses, const int32_t* counts,
                                     const float centre[3], float radius, float pose_leaf, int32_t* pairs, int cap) {
  if (n_targets < 0 || (n_targets && (!slots || !poses || !counts)) || cap < 0 || !lins_select::query_ok(centre, radius) ||
      !lins_team_select::leaf_ok(pose_leaf))
    return LINS_E_ARG;
  for (int t = 0; t < n_targets; ++t)
    if (slots[t] < 0 || counts[t] < 0 || (counts[t] && !poses[t])) return LINS_E_ARG;
  for (int t = 0; t < n_targets; ++t)
    for (int i = 0; i < counts[t]; ++i)
      if (!pose_ok(poses[t][i])) return LINS_E_INPUT;
  std::vector<lins_team_select::Pair> sel;
  const int rc = lins_team_select::select(n_targets, slots, poses, counts, centre, radius, pose_leaf, sel, nullptr);
  if (rc == lins_team_select::kDuplicate) return LINS_E_ARG;
  if (rc == lins_team_select::kTooManyCells || (int)sel.size() > cap) return LINS_E_CAPACITY;
  if (!sel.empty() && !pairs) return LINS_E_ARG;
  for (size_t i = 0; i < sel.size(); ++i) pairs[2 * i] = sel[i].slot, pairs[2 * i + 1] = sel[i].id;
  return (int)sel.size();
}

extern "C" int lins_host_team_map(int n_slots, const lins_keyframe* const* frames, const int32_t* n_frames, const int32_t* pairs, int n_pairs,
                                  const lins_local_scan* scan, lins_point* const* out, lins_local_map_sizes* sizes) {
  if (n_slots < 0 || (n_slots && (!frames || !n_frames)) || n_pairs < 0 || (n_pairs && !pairs)) return LINS_E_ARG;
  for (int s = 0; s < n_slots; ++s)
    if (n_frames[s] < 0 || (n_frames[s] && !frames[s])) return LINS_E_ARG;
  // the listed frames in list order as one frame array: the surround map over ids 0 .. n_pairs - 1 of it
  std::vector<lins_keyframe> listed((size_t)n_pairs);
  std::vector<int32_t> ids((size_t)n_pairs);
  for (int i = 0; i < n_pairs; ++i) {
    const int32_t slot = pairs[2 * i], id = pairs[2 * i + 1];
    if (slot < 0 || slot >= n_slots || id < 0 || id >= n_frames[slot]) return LINS_E_ARG;
    listed[i] = frames[slot][id], ids[i] = i;
  }
  return lins_host_surround_map(listed.data(), n_pairs, ids.data(), n_pairs, scan, out, sizes);
}
