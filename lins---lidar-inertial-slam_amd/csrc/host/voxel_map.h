// voxel_map.h — the host routines the mapping node's restatements share (host/local_map.cpp, host/keyframe_archive.cpp,
// host/keyframe_select.h): the input contract, transformPointCloud in f32 and the project's VoxelGrid.
// One definition each, so the local map, the archive's submaps and the key-pose selection cannot drift apart.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../../include/lins_map.h"

namespace lins_hostmap {

struct Trig {
  float cr, sr, cp, sp, cy, sy, tx, ty, tz;
};

// updateTransformPointCloudSinCos (LM:612-624): cos / sin of a float — the float overloads
inline Trig trig_of(const lins_key_pose& p) {
  return {std::cos(p.roll), std::sin(p.roll), std::cos(p.pitch), std::sin(p.pitch), std::cos(p.yaw), std::sin(p.yaw), p.x, p.y, p.z};
}

inline bool point_ok(const lins_point& p) {
  return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z) && std::fabs(p.x) <= 1e6f && std::fabs(p.y) <= 1e6f &&
         std::fabs(p.z) <= 1e6f;
}
inline bool cloud_ok(const lins_point* p, int n) {
  if (n < 0 || (n && !p)) return false;
  for (int i = 0; i < n; ++i)
    if (!point_ok(p[i])) return false;
  return true;
}
inline bool pose_ok(const lins_key_pose& p) {
  const float v[6] = {p.x, p.y, p.z, p.roll, p.pitch, p.yaw};
  for (float x : v)
    if (!std::isfinite(x)) return false;
  return std::fabs(p.x) <= 1e6f && std::fabs(p.y) <= 1e6f && std::fabs(p.z) <= 1e6f;
}

// transformPointCloud (LM:627-650), f32 in the order written
inline void transform_into(const lins_point* in, int n, const Trig& t, std::vector<lins_point>& out) {
  for (int i = 0; i < n; ++i) {
    const lins_point& p = in[i];
    const float x1 = t.cy * p.x - t.sy * p.y;
    const float y1 = t.sy * p.x + t.cy * p.y;
    const float z1 = p.z;
    const float x2 = x1;
    const float y2 = t.cr * y1 - t.sr * z1;
    const float z2 = t.sr * y1 + t.cr * z1;
    out.push_back({t.cp * x2 + t.sp * z2 + t.tx, y2 + t.ty, -t.sp * x2 + t.cp * z2 + t.tz, p.intensity});
  }
}

// pcl::VoxelGrid with all-field averaging (frontend.cpp voxel_grid, leaf as an argument); false: more than 2^31 cells
inline bool voxel_grid(const std::vector<lins_point>& in, float leaf, std::vector<lins_point>& out) {
  out.clear();
  if (in.empty()) return true;
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (auto& p : in) {
    mn[0] = std::min(mn[0], p.x), mn[1] = std::min(mn[1], p.y), mn[2] = std::min(mn[2], p.z);
    mx[0] = std::max(mx[0], p.x), mx[1] = std::max(mx[1], p.y), mx[2] = std::max(mx[2], p.z);
  }
  const float inv = 1.0f / leaf;
  long long minb[3], div[3];
  for (int a = 0; a < 3; ++a) {
    minb[a] = (long long)std::floor(mn[a] * inv);
    div[a] = (long long)std::floor(mx[a] * inv) - minb[a] + 1;
  }
  if (div[0] * div[1] > (1ll << 31) || div[0] * div[1] * div[2] > (1ll << 31)) return false;  // (each < 2^25: no overflow)
  struct Key {
    long long idx;
    int pt;
  };
  std::vector<Key> keys(in.size());
  for (size_t i = 0; i < in.size(); ++i) {
    const long long ix = (long long)std::floor(in[i].x * inv) - minb[0];
    const long long iy = (long long)std::floor(in[i].y * inv) - minb[1];
    const long long iz = (long long)std::floor(in[i].z * inv) - minb[2];
    keys[i] = {ix + iy * div[0] + iz * div[0] * div[1], (int)i};
  }
  std::stable_sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.idx < b.idx; });
  size_t i = 0;
  while (i < keys.size()) {
    size_t j = i;
    float sx = 0, sy = 0, sz = 0, si = 0;
    while (j < keys.size() && keys[j].idx == keys[i].idx) {
      const lins_point& p = in[keys[j].pt];
      sx += p.x, sy += p.y, sz += p.z, si += p.intensity;
      ++j;
    }
    const float n = (float)(j - i);
    out.push_back({sx / n, sy / n, sz / n, si / n});
    i = j;
  }
  return true;
}

// map_upload's 1 m box (lins_map_capi.hip cloud_box): floor of the coordinates; an empty cloud: min 0, dim 1
inline void box_1m(const std::vector<lins_point>& c, int32_t* bmin, int32_t* bdim) {
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (size_t i = 0; i < c.size(); ++i) {
    const int v[3] = {(int)std::floor(c[i].x), (int)std::floor(c[i].y), (int)std::floor(c[i].z)};
    for (int a = 0; a < 3; ++a) lo[a] = i ? std::min(lo[a], v[a]) : v[a], hi[a] = i ? std::max(hi[a], v[a]) : v[a];
  }
  for (int a = 0; a < 3; ++a) bmin[a] = lo[a], bdim[a] = hi[a] - lo[a] + 1;
}

// (int)intensity >= 0 as x86 evaluates the cast, for every float: NaN and values the cast cannot represent give
// INT_MIN there, so exactly -1 < w < 2^31 is kept (include/lins_map.h LINS_SUBMAP_DROP_NEGATIVE)
inline bool keeps_nonnegative(float w) { return w > -1.0f && w < 2147483648.0f; }

}  // namespace lins_hostmap
