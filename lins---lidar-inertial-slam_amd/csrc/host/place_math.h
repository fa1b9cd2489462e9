// place_math.h — place recognition over the key-frame archive (Scan Context, Kim & Kim, IROS 2018), the ONE scalar text
// of both libraries (host/place.cpp: the definition; place_kernels.hip: held to its bits).  DESIGN.md §5.3 "Place
// recognition" states the contract and its departures from the paper.  Everything is f32 with a fixed operation
// sequence; the files that include this are compiled with -ffp-contract=off, every fused multiply-add is an fmaf here.
//   cell        h = p[up] + lift, rho = sqrtf(p[a] * p[a] + p[b] * p[b]) (a = (up + 1) % 3, b = (up + 2) % 3); the point
//               counts iff rho < r_max and h >= 2^-10; ring min(NR - 1, (int)(rho * inv_r)), sector
//               min(NS - 1, (int)((lins_atan2f(p[b], p[a]) + pi) * inv_s)); D[ring][sector] = the maximum h, 0 when empty
//   columns     n2[s] = the fmaf chain over the rings ascending of D * D from 0, norm = sqrtf(n2), valid iff norm > 0,
//               U = D / norm (an invalid column: U = 0 — a term of exactly +0 wherever it is added)
//   distance    for j ascending, jc = (j + k) % NS, both columns valid: dot = the fmaf chain over the rings ascending of
//               Uq[r][j] * Uc[r][jc] from 0; sim += dot, cnt += 1; d(k) = cnt ? max(0, 1 - sim / (float)cnt) : 1
//   search      the minimum of (d, id, k), lexicographic: as the packed key (bits(d) << 32) | (id << 6) | k — d >= 0, so
//               its bits order as the distances do
//   top-K       a candidate's row key = the minimum over the shifts of its packed keys, kNoKey when it is not admissible.
//               Rank 0 = the minimum row key; rank j = the minimum row key among the candidates c with |c - id_i| > min_sep
//               for every earlier rank i; the ranks end at k or when only kNoKey remains (select_topk; the device takes
//               each rank's minimum in parallel over the same predicate, `separated`)
#pragma once
#include <stdint.h>

#include "../../../include/lins_host.h"
#include "../lins_math.h"

namespace lins_place {

constexpr int kNR = 20, kNS = 60, kCells = kNR * kNS;
constexpr float kPiF = 3.14159265f;
constexpr float kInvS = (float)(kNS / 6.283185307179586476925);  // sectors per radian
constexpr float kFloor = 0x1p-10f;                                // the smallest height that counts
constexpr int kMaxId = 1 << 26;                                   // ids a packed key holds
constexpr unsigned long long kNoKey = ~0ull;
constexpr int kMaxK = 8;                                          // LINS_PLACE_MAX_K: ranks of a top-K search

LINS_HD float inv_r_of(float r_max) { return (float)kNR / r_max; }

// lins_place_default_params and the parameter check of both libraries (host side)
inline void default_params(lins_place_params* p) {
  p->r_max = 80.f, p->lift = 2.f, p->up_axis = 1;
  p->clouds = LINS_SUBMAP_CORNER | LINS_SUBMAP_SURF | LINS_SUBMAP_OUTLIER;
}
inline bool params_ok(const lins_place_params* p) {
  const int all = LINS_SUBMAP_CORNER | LINS_SUBMAP_SURF | LINS_SUBMAP_OUTLIER;
  return p && p->r_max > 0.f && fabsf(p->r_max) <= __FLT_MAX__ && fabsf(inv_r_of(p->r_max)) <= __FLT_MAX__ && fabsf(p->lift) <= __FLT_MAX__ &&
         p->up_axis >= 0 && p->up_axis <= 2 && p->clouds > 0 && !(p->clouds & ~all);
}

// the cell of a point, -1: the point does not count; *h: its height
LINS_HD int cell_of(float pu, float pa, float pb, float r_max, float lift, float inv_r, float* h) {
  *h = pu + lift;
  const float rho = sqrtf(pa * pa + pb * pb);
  if (!(rho < r_max) || !(*h >= kFloor)) return -1;
  int r = (int)(rho * inv_r);
  r = r < kNR - 1 ? r : kNR - 1;
  int s = (int)((lins::lins_atan2f(pb, pa) + kPiF) * kInvS);
  s = s < kNS - 1 ? s : kNS - 1;
  return r * kNS + s;
}

// column s of D (row-major [ring][sector]) -> its norm; u[r] = the normalised column (zeros when the norm is 0)
LINS_HD float column(const float* D, int s, float* u) {
  float n2 = 0.f;
  for (int r = 0; r < kNR; ++r) n2 = fmaf(D[r * kNS + s], D[r * kNS + s], n2);
  const float norm = sqrtf(n2);
  for (int r = 0; r < kNR; ++r) u[r] = norm > 0.f ? D[r * kNS + s] / norm : 0.f;
  return norm;
}

LINS_HD float dot_columns(const float* uq, const float* uc) {
  float d = 0.f;
  for (int r = 0; r < kNR; ++r) d = fmaf(uq[r], uc[r], d);
  return d;
}

LINS_HD float distance_of(float sim, int cnt) {
  if (!cnt) return 1.f;
  const float d = 1.f - sim / (float)cnt;
  return d > 0.f ? d : 0.f;
}

LINS_HD unsigned long long pack_key(float d, int id, int k) {
  unsigned u;
  __builtin_memcpy(&u, &d, 4);
  return ((unsigned long long)u << 32) | ((unsigned long long)(unsigned)id << 6) | (unsigned long long)(unsigned)k;
}
LINS_HD void unpack_key(unsigned long long key, float* d, int* id, int* k) {
  const unsigned u = (unsigned)(key >> 32);
  __builtin_memcpy(d, &u, 4);
  *id = (int)((key & 0xffffffffull) >> 6), *k = (int)(key & 63ull);
}

// top-K: candidate c may still be chosen — it lies more than min_sep ids from every id chosen so far (ids < 2^26, min_sep >= 0)
LINS_HD bool separated(int c, const int* chosen, int n_chosen, int min_sep) {
  for (int i = 0; i < n_chosen; ++i) {
    const int gap = c > chosen[i] ? c - chosen[i] : chosen[i] - c;
    if (gap <= min_sep) return false;
  }
  return true;
}
// row[c] = candidate c's row key, c < n.  out[0 .. k): the ranks' keys, kNoKey behind the last one filled; returns how many are
inline int select_topk(const unsigned long long* row, int n, int k, int min_sep, unsigned long long* out) {
  int chosen[kMaxK], cnt = 0;
  for (int j = 0; j < k; ++j) out[j] = kNoKey;
  while (cnt < k) {
    unsigned long long best = kNoKey;
    int at = -1;
    for (int c = 0; c < n; ++c)
      if (row[c] < best && separated(c, chosen, cnt, min_sep)) best = row[c], at = c;
    if (at < 0) break;
    out[cnt] = best, chosen[cnt] = at, ++cnt;
  }
  return cnt;
}

// find_loop's gate (keyframe_select.h): at equality the candidate is not admissible; gap < 0 admits every time
LINS_HD bool time_admits(double time_c, double now, double gap) { return fabs(time_c - now) > gap; }

// ---- team search (include/lins_team.h; DESIGN.md §5.3 "Rendezvous"): a shortlist over the frames of MANY slots by a
// rotation-invariant integer key, then the distance text above for the shortlist only.
//   ring key    occ[r] = the number of sectors s with D[r][s] > 0 — Scan Context's ring key (the mean occupancy of a
//               ring) kept as an integer; sumsq = the sum of occ[r]^2; the frame's time rides along
//   key dist    dk = the sum over the rings of (occ_q[r] - occ_c[r])^2: an integer <= 20 * 60^2, the same in any order
//               and in the form sumsq_q + sumsq_c - 2 dot the device takes
//   admissible  (s, c) for a query (qs, qid): s != qs, or c != qid and time_admits — the time gate holds inside the
//               query's own slot only
//   shortlist   the M smallest (dk << 42) | (slot << 26) | id over the admissible candidates: a total order
//   row key     of the candidate at shortlist position m: the minimum over the shifts of pack_key(d, m, shift)
//   top-K       rank 0 = the minimum row key; rank j = the minimum among the positions not in conflict with an earlier
//               rank: same slot and |id - id_i| <= min_sep (select_team)
constexpr int kMaxShortlist = 64;        // M of a team search
constexpr int kMaxTeamSlots = 1 << 16;   // slots a shortlist key holds
constexpr int kMaxKeyDist = kNR * kNS * kNS;

struct RingKey {
  uint8_t occ[kNR];
  uint32_t sumsq;
  double time;
};
static_assert(sizeof(RingKey) == 32, "RingKey layout");

LINS_HD void ring_key(const float* D, double time, RingKey* key) {
  uint32_t sq = 0;
  for (int r = 0; r < kNR; ++r) {
    int occ = 0;
    for (int s = 0; s < kNS; ++s) occ += D[r * kNS + s] > 0.f ? 1 : 0;
    key->occ[r] = (uint8_t)occ, sq += (uint32_t)(occ * occ);
  }
  key->sumsq = sq, key->time = time;
}

LINS_HD int key_distance(const RingKey& q, const RingKey& c) {
  int dk = 0;
  for (int r = 0; r < kNR; ++r) {
    const int e = (int)q.occ[r] - (int)c.occ[r];
    dk += e * e;
  }
  return dk;
}

LINS_HD unsigned long long pack_team_key(int dk, int slot, int id) {
  return ((unsigned long long)(unsigned)dk << 42) | ((unsigned long long)(unsigned)slot << 26) | (unsigned long long)(unsigned)id;
}
LINS_HD void unpack_team_key(unsigned long long key, int* dk, int* slot, int* id) {
  *dk = (int)(key >> 42), *slot = (int)((key >> 26) & 0xffffull), *id = (int)(key & 0x3ffffffull);
}

LINS_HD bool team_admits(int slot, int id, double time_c, int query_slot, int query_id, double now, double gap) {
  return slot != query_slot || (id != query_id && time_admits(time_c, now, gap));
}

LINS_HD bool team_conflict(int slot_a, int id_a, int slot_b, int id_b, int min_sep) {
  const int gap = id_a > id_b ? id_a - id_b : id_b - id_a;
  return slot_a == slot_b && gap <= min_sep;
}

// row[m] = the row key of shortlist position m, shortlist[m] = its shortlist key (kNoKey: the position is empty), m < n_short.
// pos[0 .. k): the ranks' shortlist positions, -1 behind the last one filled; returns how many are
inline int select_team(const unsigned long long* row, const unsigned long long* shortlist, int n_short, int k, int min_sep, int* pos) {
  int cnt = 0;
  for (int j = 0; j < k; ++j) pos[j] = -1;
  while (cnt < k) {
    unsigned long long best = kNoKey;
    int at = -1;
    for (int m = 0; m < n_short; ++m) {
      if (shortlist[m] == kNoKey || !(row[m] < best)) continue;
      int dk, slot, id, dk_i, slot_i, id_i;
      unpack_team_key(shortlist[m], &dk, &slot, &id);
      bool free_of_all = true;
      for (int i = 0; i < cnt && free_of_all; ++i) {
        unpack_team_key(shortlist[pos[i]], &dk_i, &slot_i, &id_i);
        free_of_all = !team_conflict(slot, id, slot_i, id_i, min_sep);
      }
      if (free_of_all) best = row[m], at = m;
    }
    if (at < 0) break;
    pos[cnt++] = at;
  }
  return cnt;
}

// lins_place_team_default_params, the parameter check and the result records of both libraries (host side)
inline void team_default_params(lins_place_team_params* p) { p->shortlist = 32, p->k = 4, p->min_sep = 0, p->reserved = 0; }
inline bool team_params_ok(const lins_place_team_params* p) {
  return p && p->shortlist >= 1 && p->shortlist <= kMaxShortlist && p->k >= 1 && p->k <= kMaxK && p->min_sep >= 0;
}
// the k records of one entry from its shortlist keys, its row keys and the positions select_team chose
inline void team_results(const unsigned long long* row, const unsigned long long* shortlist, const int* pos, int k, int candidates,
                         lins_place_team_result* out) {
  for (int j = 0; j < k; ++j) {
    lins_place_team_result& r = out[j];
    r.slot = r.id = -1, r.shift = 0, r.distance = 1.f, r.dk = -1, r.candidates = candidates, r.status = 0, r.reserved = 0;
    if (pos[j] < 0) continue;
    int m;
    unpack_key(row[pos[j]], &r.distance, &m, &r.shift);
    unpack_team_key(shortlist[pos[j]], &r.dk, &r.slot, &r.id);
  }
}

}  // namespace lins_place
