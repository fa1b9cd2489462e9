// team_select.h — which key frames of a team of slots a merged local map takes, defined ONCE and compiled into both
// libraries (lins_host_team_select; lins_keyposes_team_select_batch's host path).  The device form is
// team_select_kernels.hip, with the bits of this text.  The contract (DESIGN.md §5.3 "Team map"):
//   candidates  every frame of every target slot; a slot is named once, a slot without frames is allowed
//   hit         kp_dist2(pose, centre) <= radius * radius (keypose_select_math.h: f32, in the order written)
//   cell        kp_cell per axis with inv = 1 / pose_leaf
//   box         the min / max of the hits' cells per axis; more than 2^31 cells (kp_cells_fit, voxel_grid's rule as
//               kp_select_kernel applies it): nothing is selected
//   thinning    of the hits of one cell exactly one survives: the smallest (d, slot, id) — a total order, so neither the
//               order of the target list nor the order of the scan shows
//   output      the survivors as (slot, id) in ascending (slot, id)
// The node's rule (VoxelGrid of the poses, the truncated MEAN id of a voxel) is not carried over a team: a mean of ids of
// two robots names nothing.  There is no persistent list: the answer is a pure function of the poses and the centre.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>

#include "../../../include/lins_map.h"
#include "../keypose_select_math.h"

namespace lins_team_select {

struct Pair {
  int32_t slot, id;
};

enum { kOk = 0, kDuplicate = 1, kTooManyCells = 2 };

// the target list in ascending slot order (positions into the list); false: a slot is named twice
inline bool order_targets(int n_targets, const int32_t* slots, std::vector<int>& order) {
  order.resize((size_t)n_targets);
  for (int t = 0; t < n_targets; ++t) order[t] = t;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return slots[a] < slots[b]; });
  for (int t = 1; t < n_targets; ++t)
    if (slots[order[t]] == slots[order[t - 1]]) return false;
  return true;
}

// target t: slot slots[t] with the counts[t] key poses at poses[t] (by frame id).  hits (may be null): the poses within
// the radius.  Returns kOk with the survivors in out, kDuplicate, or kTooManyCells (out empty).
inline int select(int n_targets, const int32_t* slots, const lins_key_pose* const* poses, const int32_t* counts, const float centre[3],
                  float radius, float pose_leaf, std::vector<Pair>& out, long long* hits) {
  using namespace lins_kp;
  struct Hit {
    float d;
    int32_t slot, id;
    long long c[3], cell;
  };
  out.clear();
  if (hits) *hits = 0;
  std::vector<int> order;
  if (!order_targets(n_targets, slots, order)) return kDuplicate;
  const float r2 = radius * radius, inv = 1.0f / pose_leaf;
  std::vector<Hit> h;
  long long lo[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX}, hi[3] = {LLONG_MIN, LLONG_MIN, LLONG_MIN};
  for (int t : order)
    for (int i = 0; i < counts[t]; ++i) {
      const lins_key_pose& p = poses[t][i];
      const float d = kp_dist2(p.x, p.y, p.z, centre[0], centre[1], centre[2]);
      if (!(d <= r2)) continue;
      Hit x{d, slots[t], i, {kp_cell(p.x, inv), kp_cell(p.y, inv), kp_cell(p.z, inv)}, 0};
      for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], x.c[a]), hi[a] = std::max(hi[a], x.c[a]);
      h.push_back(x);
    }
  if (hits) *hits = (long long)h.size();
  if (h.empty()) return kOk;
  long long div[3];
  for (int a = 0; a < 3; ++a) {
    // (max - min of two long long as an unsigned: exact; anything from 2^32 up is too large whatever the others are)
    const unsigned long long span = (unsigned long long)hi[a] - (unsigned long long)lo[a];
    div[a] = span >= (1ull << 32) ? (1ll << 32) : (long long)span + 1;
  }
  if (!kp_cells_fit(div[0], div[1], div[2])) return kTooManyCells;
  for (Hit& x : h) x.cell = (x.c[0] - lo[0]) + (x.c[1] - lo[1]) * div[0] + (x.c[2] - lo[2]) * div[0] * div[1];  // < 2^31
  std::sort(h.begin(), h.end(), [](const Hit& a, const Hit& b) {
    if (a.cell != b.cell) return a.cell < b.cell;
    if (a.d != b.d) return a.d < b.d;
    return a.slot != b.slot ? a.slot < b.slot : a.id < b.id;
  });
  for (size_t i = 0; i < h.size(); ++i)
    if (i == 0 || h[i].cell != h[i - 1].cell) out.push_back(Pair{h[i].slot, h[i].id});
  std::sort(out.begin(), out.end(), [](const Pair& a, const Pair& b) { return a.slot != b.slot ? a.slot < b.slot : a.id < b.id; });
  return kOk;
}

inline bool leaf_ok(float pose_leaf) { return pose_leaf > 0.f && std::isfinite(1.0f / pose_leaf); }

}  // namespace lins_team_select
