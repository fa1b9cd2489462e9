// keypose_select_math.h — the scalar pieces of the key-pose selection on the device (keypose_select_kernels.hip,
// lins_archive_capi.hip lins_keyposes_*), for host and device.  The contract is host/keyframe_select.h + host/voxel_map.h
// voxel_grid, bit for bit; what stands here is the form the kernels use, each piece small enough to be held against
// that text on the CPU (tests/native/keyposes_check.cpp):
//   kp_dist2          the hit test's squared distance, f32 in the order written (the tree is built with contraction off)
//   kp_key            a hit as one unsigned 64-bit word that orders as (d, id): d is a finite non-negative float, so its
//                     bits order as an unsigned
//   kp_cell           floor(coord * inv) as voxel_grid takes it
//   kp_cells_fit      voxel_grid's 2^31-cell rule, without the products that could overflow
//   kp_surround_list  surround_update in linear time: a serial function; the kernel is its parallel form
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KP_HD __host__ __device__ inline
#else
#define KP_HD inline
#endif

namespace lins_kp {

constexpr int kSortCap = 8192;   // hits an entry sorts in LDS; above it the host text serves the entry
constexpr int kUnmarked = INT_MAX;  // kp_surround_list's scratch: an id that ds does not name

KP_HD float kp_dist2(float px, float py, float pz, float cx, float cy, float cz) {
  const float dx = px - cx, dy = py - cy, dz = pz - cz;
  return (dx * dx + dy * dy) + dz * dz;
}

KP_HD uint32_t kp_float_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}

KP_HD uint64_t kp_key(float d, int id) { return ((uint64_t)kp_float_bits(d) << 32) | (uint32_t)id; }
KP_HD int kp_key_id(uint64_t key) { return (int)(uint32_t)key; }

KP_HD long long kp_cell(float coord, float inv) { return (long long)floorf(coord * inv); }

// div0 * div1 > 2^31 || div0 * div1 * div2 > 2^31 is false (every div >= 1)
KP_HD bool kp_cells_fit(long long div0, long long div1, long long div2) {
  const long long lim = 1ll << 31;
  if (div0 > lim || div1 > lim || div2 > lim) return false;
  const long long plane = div0 * div1;  // <= 2^62
  if (plane > lim) return false;
  return plane * div2 <= lim;           // <= 2^62
}

// surround_update(list, ds) into out; returns the new length.  mark: nf ints of scratch, nf the frames of the slot; every
// id of list and of ds lies in [0, nf) (the caller's check).  out holds up to n_list + n_ds ids and is not list.
//   1 mark[id] = the first position of id in ds
//   2 the survivors: the list entries whose id is marked, in order; their ids are then marked -1
//   3 each ds[i], in order, that is the first occurrence of its id and no survivor's
KP_HD int kp_surround_list(const int* list, int n_list, const int* ds, int n_ds, int* mark, int nf, int* out) {
  for (int i = 0; i < nf; ++i) mark[i] = kUnmarked;
  for (int i = 0; i < n_ds; ++i)
    if (i < mark[ds[i]]) mark[ds[i]] = i;
  int n = 0;
  for (int j = 0; j < n_list; ++j)
    if (mark[list[j]] != kUnmarked) out[n++] = list[j];
  for (int j = 0; j < n; ++j) mark[out[j]] = -1;
  for (int i = 0; i < n_ds; ++i)
    if (mark[ds[i]] == i) out[n++] = ds[i];
  return n;
}

}  // namespace lins_kp
