// place.cpp — place recognition on the CPU (include/lins_host.h lins_host_place_*): the DEFINITION the device calls of
// include/lins_place.h are held to.  The scalar text is place_math.h, compiled into both libraries; here it runs in
// the contract's own order, one pair and one shift at a time.  DESIGN.md §5.3 "Place recognition".
#include <cmath>
#include <cstring>
#include <vector>

#include "../../../include/lins_host.h"
#include "place_guess.h"
#include "place_math.h"
#include "rendezvous_consensus.h"
#include "voxel_map.h"

using namespace lins_place;
using lins_hostmap::cloud_ok;

namespace {

// the normalised columns of D, column-major: U[s * kNR + r]; valid[s]
void columns_of(const float* D, float* U, bool* valid) {
  for (int s = 0; s < kNS; ++s) valid[s] = column(D, s, U + s * kNR) > 0.f;
}

void distances(const float* Uq, const bool* vq, const float* Uc, const bool* vc, float* d) {
  for (int k = 0; k < kNS; ++k) {
    float sim = 0.f;
    int cnt = 0;
    for (int j = 0; j < kNS; ++j) {
      const int jc = (j + k) % kNS;
      if (!vq[j] || !vc[jc]) continue;
      sim += dot_columns(Uq + j * kNR, Uc + jc * kNR);
      cnt += 1;
    }
    d[k] = distance_of(sim, cnt);
  }
}

}  // namespace

extern "C" {

void lins_place_default_params(lins_place_params* p) {
  if (p) default_params(p);
}

int lins_host_place_descriptor(const lins_keyframe* f, const lins_place_params* prm, float* out) {
  if (!f || !out || !params_ok(prm)) return LINS_E_ARG;
  const lins_point* c[3] = {f->corner, f->surf, f->outlier};
  const int n[3] = {f->n_corner, f->n_surf, f->n_outlier};
  for (int q = 0; q < 3; ++q) {
    if (n[q] < 0 || (n[q] && !c[q])) return LINS_E_ARG;
    if (!cloud_ok(c[q], n[q])) return LINS_E_INPUT;
  }
  const int up = prm->up_axis, a = (up + 1) % 3, b = (up + 2) % 3;
  const float inv_r = inv_r_of(prm->r_max);
  for (int i = 0; i < kCells; ++i) out[i] = 0.f;
  for (int q = 0; q < 3; ++q) {
    if (!(prm->clouds & (1 << q))) continue;
    for (int i = 0; i < n[q]; ++i) {
      const float p[3] = {c[q][i].x, c[q][i].y, c[q][i].z};
      float h;
      const int cell = cell_of(p[up], p[a], p[b], prm->r_max, prm->lift, inv_r, &h);
      if (cell >= 0 && h > out[cell]) out[cell] = h;
    }
  }
  return LINS_OK;
}

int lins_host_place_distance(const float* query, const float* candidate, float* d) {
  if (!query || !candidate || !d) return LINS_E_ARG;
  std::vector<float> Uq(kCells), Uc(kCells);
  bool vq[kNS], vc[kNS];
  columns_of(query, Uq.data(), vq), columns_of(candidate, Uc.data(), vc);
  distances(Uq.data(), vq, Uc.data(), vc, d);
  return LINS_OK;
}

int lins_host_place_search(const float* query, const float* descs, const double* times, int n, int skip_id, double now, double min_gap_s,
                           int32_t* id, int32_t* shift, float* distance, int32_t* candidates) {
  if (!query || n < 0 || n > kMaxId || (n && (!descs || !times)) || !id || !shift || !distance) return LINS_E_ARG;
  if (!std::isfinite(now) || std::isnan(min_gap_s)) return LINS_E_INPUT;
  std::vector<float> Uq(kCells), Uc(kCells);
  bool vq[kNS], vc[kNS];
  float d[kNS];
  columns_of(query, Uq.data(), vq);
  unsigned long long best = kNoKey;
  int cnt = 0;
  for (int c = 0; c < n; ++c) {
    if (c == skip_id || !time_admits(times[c], now, min_gap_s)) continue;
    ++cnt;
    columns_of(descs + (size_t)c * kCells, Uc.data(), vc);
    distances(Uq.data(), vq, Uc.data(), vc, d);
    for (int k = 0; k < kNS; ++k) {
      const unsigned long long key = pack_key(d[k], c, k);
      if (key < best) best = key;
    }
  }
  *id = -1, *shift = 0, *distance = 1.f;
  if (best != kNoKey) unpack_key(best, distance, id, shift);
  if (candidates) *candidates = cnt;
  return LINS_OK;
}

int lins_host_place_topk(const float* query, const float* descs, const double* times, int n, int skip_id, double now, double min_gap_s, int k,
                         int min_sep, int32_t* ids, int32_t* shifts, float* dist, int32_t* candidates) {
  if (!query || n < 0 || n > kMaxId || (n && (!descs || !times)) || k < 1 || k > kMaxK || min_sep < 0 || !ids || !shifts || !dist) return LINS_E_ARG;
  if (!std::isfinite(now) || std::isnan(min_gap_s)) return LINS_E_INPUT;
  std::vector<float> Uq(kCells), Uc(kCells);
  bool vq[kNS], vc[kNS];
  float d[kNS];
  columns_of(query, Uq.data(), vq);
  std::vector<unsigned long long> row((size_t)n, kNoKey);
  int cnt = 0;
  for (int c = 0; c < n; ++c) {
    if (c == skip_id || !time_admits(times[c], now, min_gap_s)) continue;
    ++cnt;
    columns_of(descs + (size_t)c * kCells, Uc.data(), vc);
    distances(Uq.data(), vq, Uc.data(), vc, d);
    for (int s = 0; s < kNS; ++s) {
      const unsigned long long key = pack_key(d[s], c, s);
      if (key < row[c]) row[c] = key;
    }
  }
  unsigned long long keys[kMaxK];
  const int filled = select_topk(row.data(), n, k, min_sep, keys);
  for (int j = 0; j < k; ++j) {
    ids[j] = -1, shifts[j] = 0, dist[j] = 1.f;
    if (keys[j] != kNoKey) unpack_key(keys[j], &dist[j], &ids[j], &shifts[j]);
  }
  if (candidates) *candidates = cnt;
  return filled;
}

void lins_place_team_default_params(lins_place_team_params* p) {
  if (p) team_default_params(p);
}

int lins_host_place_ring_key(const float* desc, uint8_t* occ, uint32_t* sumsq) {
  if (!desc || !occ || !sumsq) return LINS_E_ARG;
  RingKey key;
  ring_key(desc, 0.0, &key);
  std::memcpy(occ, key.occ, sizeof key.occ);
  *sumsq = key.sumsq;
  return LINS_OK;
}

int lins_host_place_team_topk(const float* query, int query_slot, int query_id, double now, double min_gap_s, int n_targets,
                              const int32_t* target_slots, const float* const* descs, const double* const* times, const int32_t* counts,
                              const lins_place_team_params* prm, lins_place_team_result* out) {
  if (!query || !out || !team_params_ok(prm) || n_targets < 0 || (n_targets && (!target_slots || !descs || !times || !counts))) return LINS_E_ARG;
  if (query_slot < 0 || query_slot >= kMaxTeamSlots || query_id < 0 || query_id >= kMaxId) return LINS_E_ARG;
  for (int t = 0; t < n_targets; ++t) {
    if (target_slots[t] < 0 || target_slots[t] >= kMaxTeamSlots || counts[t] < 0 || counts[t] > kMaxId) return LINS_E_ARG;
    if (counts[t] && (!descs[t] || !times[t])) return LINS_E_ARG;
    for (int u = 0; u < t; ++u)
      if (target_slots[u] == target_slots[t]) return LINS_E_ARG;
  }
  if (!std::isfinite(now) || std::isnan(min_gap_s)) return LINS_E_INPUT;
  // stage 1: the M smallest shortlist keys, one minimum above the last at a time (the keys are distinct)
  RingKey kq, kc;
  ring_key(query, 0.0, &kq);
  std::vector<unsigned long long> keys;
  for (int t = 0; t < n_targets; ++t)
    for (int c = 0; c < counts[t]; ++c) {
      if (!team_admits(target_slots[t], c, times[t][c], query_slot, query_id, now, min_gap_s)) continue;
      ring_key(descs[t] + (size_t)c * kCells, times[t][c], &kc);
      keys.push_back(pack_team_key(key_distance(kq, kc), target_slots[t], c));
    }
  const int candidates = (int)keys.size();
  unsigned long long shortlist[kMaxShortlist], row[kMaxShortlist];
  int n_short = 0;
  for (; n_short < prm->shortlist; ++n_short) {
    unsigned long long best = kNoKey;
    for (unsigned long long key : keys)
      if (key < best && (!n_short || key > shortlist[n_short - 1])) best = key;
    if (best == kNoKey) break;
    shortlist[n_short] = best;
  }
  // stage 2: the row key of every shortlisted candidate
  std::vector<float> Uq(kCells), Uc(kCells);
  bool vq[kNS], vc[kNS];
  float d[kNS];
  columns_of(query, Uq.data(), vq);
  for (int m = 0; m < n_short; ++m) {
    int dk, slot, id, t = 0;
    unpack_team_key(shortlist[m], &dk, &slot, &id);
    while (target_slots[t] != slot) ++t;
    columns_of(descs[t] + (size_t)id * kCells, Uc.data(), vc);
    distances(Uq.data(), vq, Uc.data(), vc, d);
    row[m] = kNoKey;
    for (int s = 0; s < kNS; ++s) {
      const unsigned long long key = pack_key(d[s], m, s);
      if (key < row[m]) row[m] = key;
    }
  }
  int pos[kMaxK];
  const int filled = select_team(row, shortlist, n_short, prm->k, prm->min_sep, pos);
  team_results(row, shortlist, pos, prm->k, candidates, out);
  return filled;
}

int lins_host_place_guess(const lins_key_pose* pose_q, const lins_key_pose* pose_c, int shift, int up_axis, double* T0) {
  if (!pose_q || !pose_c || !T0 || shift < 0 || shift >= kNS || up_axis < 0 || up_axis > 2) return LINS_E_ARG;
  guess(*pose_q, *pose_c, shift, up_axis, T0);
  return LINS_OK;
}

int lins_host_place_team_guess(const lins_key_pose* pose_q, const lins_key_pose* pose_c, int shift, int up_axis, double* T0) {
  if (!pose_q || !pose_c || !T0 || shift < 0 || shift >= kNS || up_axis < 0 || up_axis > 2) return LINS_E_ARG;
  guess_team(*pose_q, *pose_c, shift, up_axis, T0);
  return LINS_OK;
}

// ---- rendezvous over a window: the consensus rule (rendezvous_consensus.h) ----
void lins_rendezvous_consensus_default_params(lins_consensus_params* p) {
  if (p) lins_consensus::default_params(p);
}

int lins_host_rendezvous_consensus(const lins_consensus_hyp* hyp, int n_hyp, const lins_consensus_params* prm, lins_consensus_result* out) {
  using namespace lins_consensus;
  if (!out || n_hyp < 0 || n_hyp > kMaxHyp || (n_hyp && !hyp) || !bars_ok(prm)) return LINS_E_ARG;
  if (int rc = table_check(hyp, n_hyp)) return rc;
  evaluate(hyp, n_hyp, bars_of(prm->max_translation, prm->min_cos_rotation), out);
  return LINS_OK;
}

}  // extern "C"
