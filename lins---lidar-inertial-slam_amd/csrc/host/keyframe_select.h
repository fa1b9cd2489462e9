// keyframe_select.h — which key frames a global map or a loop closure takes (LM:989-1007, 1050-1067), defined ONCE and
// compiled into both libraries (lins_archive_select_radius / _find_loop and lins_host_select_radius / _find_loop).  Key
// poses are a few thousand points: for one robot this is host work, and this text is the definition.  For a batch of
// streams the same selection runs on the device, one workgroup per entry, with the bits of this text
// (keypose_select_kernels.hip, lins_keyposes_*; profiles/keypose_select_rate.txt says where that pays); an entry the
// kernels do not take is served by this text inside the same call.  The contract:
//   radius search  the poses with f32 ((dx*dx + dy*dy) + dz*dz) <= radius*radius, ordered by ascending (that squared
//                  distance, id).  PCL's FLANN radius search is not in the reference's text and cannot be pinned here —
//                  like the 5-NN of scan-to-map it is restated as the exact search with a fixed order.
//   selection      the hits as points (x, y, z, (float)id) in that order through the project's VoxelGrid at pose_leaf
//                  (stable order, sequential f32 sums over all four fields); the frame of output voxel v is (int) of its
//                  averaged intensity — the mean of the ids in the voxel, truncated (LM:1007), which may name a frame that
//                  is not itself in the voxel; frames are visited in ascending voxel order.
//   loop candidate the first hit, in the radius search's order, with fabs(time - now) > min_gap_s; -1: none.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "voxel_map.h"

namespace lins_select {

// ids of the poses (n x lins_key_pose: x, y, z used) within radius of centre, ascending (squared distance, id)
inline void radius_search(const lins_key_pose* poses, int n, const float centre[3], float radius, std::vector<int>& ids) {
  struct Hit {
    float d;
    int id;
  };
  std::vector<Hit> hits;
  const float r2 = radius * radius;
  for (int i = 0; i < n; ++i) {
    const float dx = poses[i].x - centre[0], dy = poses[i].y - centre[1], dz = poses[i].z - centre[2];
    const float d = (dx * dx + dy * dy) + dz * dz;
    if (d <= r2) hits.push_back({d, i});
  }
  std::sort(hits.begin(), hits.end(), [](const Hit& a, const Hit& b) { return a.d < b.d || (a.d == b.d && a.id < b.id); });
  ids.clear();
  for (const Hit& h : hits) ids.push_back(h.id);
}

// false: the hits' pose_leaf box has more than 2^31 cells
inline bool select_radius(const lins_key_pose* poses, int n, const float centre[3], float radius, float pose_leaf, std::vector<int>& ids) {
  std::vector<int> hits;
  radius_search(poses, n, centre, radius, hits);
  std::vector<lins_point> pts, ds;
  for (int id : hits) pts.push_back({poses[id].x, poses[id].y, poses[id].z, (float)id});
  if (!lins_hostmap::voxel_grid(pts, pose_leaf, ds)) return false;
  ids.clear();
  for (const lins_point& p : ds) ids.push_back((int)p.intensity);
  return true;
}

inline int find_loop(const lins_key_pose* poses, const double* times, int n, const float centre[3], float radius, double now, double min_gap_s) {
  std::vector<int> hits;
  radius_search(poses, n, centre, radius, hits);
  for (int id : hits)
    if (std::fabs(times[id] - now) > min_gap_s) return id;
  return -1;
}

// surroundingExistingKeyPosesID after one extractSurroundingKeyFrames with the loop closure off (LM:1261-1308), ds = the
// frames select_radius chose: entries whose id is not among ds are erased in place (the survivors keep their order),
// then each ds[i], in order, is appended unless the list — earlier appends included — holds it already.  An id of ds is
// taken as it is (the truncated mean id of a voxel, which may name a frame outside the radius).
inline void surround_update(std::vector<int>& list, const std::vector<int>& ds) {
  for (int i = 0; i < (int)list.size(); ++i) {
    bool existing = false;
    for (size_t j = 0; j < ds.size() && !existing; ++j) existing = list[i] == ds[j];
    if (!existing) list.erase(list.begin() + i), --i;
  }
  for (size_t i = 0; i < ds.size(); ++i) {
    bool existing = false;
    for (size_t j = 0; j < list.size() && !existing; ++j) existing = list[j] == ds[i];
    if (!existing) list.push_back(ds[i]);
  }
}

inline bool query_ok(const float centre[3], float radius) {
  return centre && std::isfinite(centre[0]) && std::isfinite(centre[1]) && std::isfinite(centre[2]) && std::isfinite(radius) && radius >= 0.f;
}

}  // namespace lins_select
