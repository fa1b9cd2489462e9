// local_map.cpp — the mapping node's local map on the CPU (include/lins_host.h lins_host_local_map): the restatement the
// device build of lins_local_map_build (local_map_kernels.hip) is checked against, bit for bit.
//   extractSurroundingKeyFrames  LM:1201-1324  last min(window, K) key frames -> map frame (transformPointCloud,
//                                              LM:627-650), concatenated oldest first, VoxelGrid 0.2 / 0.4 m
//   downsampleCurrentScan        LM:1326-1349  corner 0.2, surf 0.4, outlier 0.4, surfTotal = 0.4 of (surfDS ++ outlierDS)
// VoxelGrid is the contract of frontend.cpp's voxel_grid with the leaf as an argument.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "../../../include/lins_host.h"

namespace {

struct Trig {
  float cr, sr, cp, sp, cy, sy, tx, ty, tz;
};

// updateTransformPointCloudSinCos (LM:612-624): cos / sin of a float — the float overloads
Trig trig_of(const lins_key_pose& p) {
  return {std::cos(p.roll), std::sin(p.roll), std::cos(p.pitch), std::sin(p.pitch), std::cos(p.yaw), std::sin(p.yaw), p.x, p.y, p.z};
}

bool point_ok(const lins_point& p) {
  return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z) && std::fabs(p.x) <= 1e6f && std::fabs(p.y) <= 1e6f &&
         std::fabs(p.z) <= 1e6f;
}
bool cloud_ok(const lins_point* p, int n) {
  if (n < 0 || (n && !p)) return false;
  for (int i = 0; i < n; ++i)
    if (!point_ok(p[i])) return false;
  return true;
}
bool pose_ok(const lins_key_pose& p) {
  const float v[6] = {p.x, p.y, p.z, p.roll, p.pitch, p.yaw};
  for (float x : v)
    if (!std::isfinite(x)) return false;
  return std::fabs(p.x) <= 1e6f && std::fabs(p.y) <= 1e6f && std::fabs(p.z) <= 1e6f;
}

// transformPointCloud (LM:627-650), f32 in the order written
void transform_into(const lins_point* in, int n, const Trig& t, std::vector<lins_point>& out) {
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
bool voxel_grid(const std::vector<lins_point>& in, float leaf, std::vector<lins_point>& out) {
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
void box_1m(const std::vector<lins_point>& c, int32_t* bmin, int32_t* bdim) {
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (size_t i = 0; i < c.size(); ++i) {
    const int v[3] = {(int)std::floor(c[i].x), (int)std::floor(c[i].y), (int)std::floor(c[i].z)};
    for (int a = 0; a < 3; ++a) lo[a] = i ? std::min(lo[a], v[a]) : v[a], hi[a] = i ? std::max(hi[a], v[a]) : v[a];
  }
  for (int a = 0; a < 3; ++a) bmin[a] = lo[a], bdim[a] = hi[a] - lo[a] + 1;
}

}  // namespace

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
