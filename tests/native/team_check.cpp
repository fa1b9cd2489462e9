// team_check.cpp — the team search's scalar text (the lower part of csrc/host/place_math.h) and its definition
// (csrc/host/place.cpp lins_host_place_team_topk) on the CPU, under AddressSanitizer and UBSan
// (tests/test_place_team_host.py builds and runs it; a stand-alone program, never loaded into Python).
//   team_check keys | select | search | layout_b | layout_c      one case each; exit 0 and "ok <case>" when every check holds
// Every descriptor block and every time array lives in a heap block of exactly its size.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <tuple>
#include <vector>

#include "host/place_math.h"

using namespace lins_place;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      return 1;                                                      \
    }                                                                \
  } while (0)

namespace {

// a descriptor with about `fill` of its cells occupied; a few rings left empty or full
void random_desc(std::mt19937& g, float fill, float* D) {
  std::uniform_real_distribution<float> u(0.f, 1.f);
  for (int r = 0; r < kNR; ++r) {
    const float f = u(g) < 0.1f ? 0.f : u(g) < 0.1f ? 1.f : fill;
    for (int s = 0; s < kNS; ++s) D[r * kNS + s] = u(g) < f ? 0.5f + 5.f * u(g) : 0.f;
  }
}

int keys_case() {
  std::mt19937 g(1);
  std::unique_ptr<float[]> A(new float[kCells]), B(new float[kCells]);
  for (int it = 0; it < 200; ++it) {
    random_desc(g, 0.05f + 0.004f * it, A.get()), random_desc(g, 0.3f, B.get());
    RingKey a, b;
    ring_key(A.get(), 1.5, &a), ring_key(B.get(), -2.0, &b);
    CHECK(a.time == 1.5 && b.time == -2.0);
    unsigned sq = 0, dot = 0;
    int want = 0;
    for (int r = 0; r < kNR; ++r) {
      int ca = 0, cb = 0;
      for (int s = 0; s < kNS; ++s) ca += A[r * kNS + s] != 0.f, cb += B[r * kNS + s] != 0.f;
      CHECK(a.occ[r] == ca && b.occ[r] == cb);
      sq += ca * ca, dot += ca * cb, want += (ca - cb) * (ca - cb);
    }
    CHECK(a.sumsq == sq);
    const int dk = key_distance(a, b);
    CHECK(dk == want && dk == key_distance(b, a) && key_distance(a, a) == 0 && dk <= kMaxKeyDist);
    CHECK((unsigned)dk == a.sumsq + b.sumsq - 2u * dot);  // the form the device takes
    // a turn about the vertical moves the columns, not the counts
    std::unique_ptr<float[]> T(new float[kCells]);
    for (int r = 0; r < kNR; ++r)
      for (int s = 0; s < kNS; ++s) T[r * kNS + (s + it) % kNS] = A[r * kNS + s];
    RingKey t;
    ring_key(T.get(), 1.5, &t);
    CHECK(std::memcmp(&t, &a, sizeof t) == 0 || (std::memcmp(t.occ, a.occ, kNR) == 0 && t.sumsq == a.sumsq));
  }
  // the packed order is (dk, slot, id), at the fields' ends too
  const int dks[] = {0, 1, 71999, kMaxKeyDist}, slots[] = {0, 1, kMaxTeamSlots - 1}, ids[] = {0, 1, kMaxId - 1};
  std::vector<std::tuple<int, int, int>> all;
  for (int dk : dks)
    for (int s : slots)
      for (int i : ids) all.emplace_back(dk, s, i);
  for (const auto& x : all)
    for (const auto& y : all) {
      const unsigned long long kx = pack_team_key(std::get<0>(x), std::get<1>(x), std::get<2>(x));
      const unsigned long long ky = pack_team_key(std::get<0>(y), std::get<1>(y), std::get<2>(y));
      CHECK((x < y) == (kx < ky) && kx != kNoKey);
      int dk, s, i;
      unpack_team_key(kx, &dk, &s, &i);
      CHECK(std::make_tuple(dk, s, i) == x);
    }
  CHECK(team_conflict(3, 10, 3, 10, 0) && !team_conflict(3, 10, 4, 10, 1000) && team_conflict(3, 10, 3, 14, 4) && !team_conflict(3, 14, 3, 9, 4));
  CHECK(team_admits(1, 5, 0.0, 2, 5, 0.0, 100.0) && !team_admits(2, 5, 50.0, 2, 5, 0.0, 1.0) && !team_admits(2, 6, 1.0, 2, 5, 0.0, 1.0) &&
        team_admits(2, 6, 1.5, 2, 5, 0.0, 1.0));
  return 0;
}

int select_case() {
  std::mt19937 g(2);
  for (int it = 0; it < 200; ++it) {
    const int n = it < 4 ? it : 1 + (int)(g() % kMaxShortlist), k = 1 + (int)(g() % kMaxK), sep = it % 3 == 0 ? 0 : (int)(g() % 6);
    // shortlist positions over few slots and a narrow id range, so that conflicts are common; some positions empty; few
    // distinct distances, so that the position decides among equals
    std::unique_ptr<unsigned long long[]> sl(new unsigned long long[n]), row(new unsigned long long[n]);
    std::vector<std::tuple<unsigned long long, int, int, int>> order;  // (row key, position, slot, id)
    for (int m = 0; m < n; ++m) {
      const int slot = (int)(g() % 3), id = (int)(g() % 20);
      const bool empty = g() % 8 == 0;
      sl[m] = empty ? kNoKey : pack_team_key((int)(g() % 50), slot, id);
      row[m] = empty ? kNoKey : pack_key(0.125f * (float)(g() % 4), m, (int)(g() % kNS));
      if (!empty) order.emplace_back(row[m], m, slot, id);
    }
    std::sort(order.begin(), order.end());
    std::vector<int> want;
    for (const auto& o : order) {
      if ((int)want.size() == k) break;
      bool ok = true;
      for (int w : want) {
        int dk, slot, id;
        unpack_team_key(sl[w], &dk, &slot, &id);
        ok = ok && !(slot == std::get<2>(o) && std::abs(id - std::get<3>(o)) <= sep);
      }
      if (ok) want.push_back(std::get<1>(o));
    }
    std::unique_ptr<int[]> pos(new int[k]);
    const int filled = select_team(row.get(), sl.get(), n, k, sep, pos.get());
    CHECK(filled == (int)want.size());
    for (int j = 0; j < k; ++j) CHECK(pos[j] == (j < filled ? want[j] : -1));
    std::unique_ptr<lins_place_team_result[]> out(new lins_place_team_result[k]);
    team_results(row.get(), sl.get(), pos.get(), k, 7, out.get());
    for (int j = 0; j < k; ++j) {
      CHECK(out[j].candidates == 7 && out[j].status == 0);
      if (j >= filled) CHECK(out[j].slot == -1 && out[j].id == -1 && out[j].shift == 0 && out[j].distance == 1.f && out[j].dk == -1);
    }
  }
  return 0;
}

int search_case() {
  std::mt19937 g(3);
  for (int it = 0; it < 40; ++it) {
    const int n_targets = (int)(g() % 5);
    std::vector<std::unique_ptr<float[]>> descs;
    std::vector<std::unique_ptr<double[]>> times;
    std::vector<const float*> dp;
    std::vector<const double*> tp;
    std::vector<int32_t> slots, counts;
    std::unique_ptr<float[]> Q(new float[kCells]);
    random_desc(g, 0.3f, Q.get());
    int total = 0;
    for (int t = 0; t < n_targets; ++t) {
      const int n = (int)(g() % 7);
      descs.emplace_back(new float[(size_t)n * kCells]), times.emplace_back(new double[n]);
      for (int c = 0; c < n; ++c) {
        if (g() % 4 == 0) std::memcpy(descs[t].get() + (size_t)c * kCells, Q.get(), kCells * sizeof(float));  // a twin of the query
        else random_desc(g, 0.3f, descs[t].get() + (size_t)c * kCells);
        times[t][c] = (double)c;
      }
      slots.push_back(3 * t + 1), counts.push_back(n), dp.push_back(descs[t].get()), tp.push_back(times[t].get());
      total += n;
    }
    lins_place_team_params prm;
    lins_place_team_default_params(&prm);
    CHECK(prm.shortlist == 32 && prm.k == 4 && prm.min_sep == 0);
    prm.shortlist = it % 2 ? 64 : 1 + (int)(g() % 8), prm.k = 1 + (int)(g() % kMaxK), prm.min_sep = (int)(g() % 3);
    const int qs = n_targets && it % 3 == 0 ? slots[0] : 100, qid = 2;
    std::unique_ptr<lins_place_team_result[]> out(new lins_place_team_result[prm.k]);
    const int filled = lins_host_place_team_topk(Q.get(), qs, qid, 2.0, 1.0, n_targets, slots.data(), dp.data(), tp.data(), counts.data(), &prm, out.get());
    CHECK(filled >= 0 && filled <= prm.k && filled <= prm.shortlist);
    int adm = 0;
    for (int t = 0; t < n_targets; ++t)
      for (int c = 0; c < counts[t]; ++c) adm += slots[t] != qs || (c != qid && std::fabs(times[t][c] - 2.0) > 1.0);
    CHECK(out[0].candidates == adm && (filled > 0) == (adm > 0));
    for (int j = 0; j < filled; ++j) {
      const lins_place_team_result& r = out[j];
      int t = 0;
      while (t < n_targets && slots[t] != r.slot) ++t;
      CHECK(t < n_targets && r.id >= 0 && r.id < counts[t] && (r.slot != qs || (r.id != qid && std::fabs(times[t][r.id] - 2.0) > 1.0)));
      float d[kNS];
      CHECK(lins_host_place_distance(Q.get(), descs[t].get() + (size_t)r.id * kCells, d) == 0);
      CHECK(r.shift >= 0 && r.shift < kNS && d[r.shift] == r.distance);
      for (int s = 0; s < kNS; ++s) CHECK(d[s] > r.distance || (d[s] == r.distance && s >= r.shift));
      if (j) CHECK(out[j - 1].distance <= r.distance);
      for (int i = 0; i < j; ++i) CHECK(!(out[i].slot == r.slot && std::abs(out[i].id - r.id) <= prm.min_sep));
    }
    if (filled && prm.shortlist >= total) {  // everything shortlisted: rank 0 is the exhaustive minimum
      for (int t = 0; t < n_targets; ++t)
        for (int c = 0; c < counts[t]; ++c) {
          if (!(slots[t] != qs || (c != qid && std::fabs(times[t][c] - 2.0) > 1.0))) continue;
          float d[kNS];
          lins_host_place_distance(Q.get(), descs[t].get() + (size_t)c * kCells, d);
          CHECK(*std::min_element(d, d + kNS) >= out[0].distance);
        }
    }
  }
  return 0;
}

// a team of exact-size heap blocks, one per slot
struct Team {
  std::vector<std::unique_ptr<float[]>> descs;
  std::vector<std::unique_ptr<double[]>> times;
  std::vector<const float*> dp;
  std::vector<const double*> tp;
  std::vector<int32_t> slots, counts;
  float* add(int slot, int n) {
    descs.emplace_back(new float[(size_t)n * kCells]), times.emplace_back(new double[n]);
    for (int c = 0; c < n; ++c) times.back()[c] = (double)c;
    slots.push_back(slot), counts.push_back(n), dp.push_back(descs.back().get()), tp.push_back(times.back().get());
    return descs.back().get();
  }
  int topk(const float* Q, int qs, int qid, int M, int k, lins_place_team_result* out) const {
    lins_place_team_params prm;
    lins_place_team_default_params(&prm);
    prm.shortlist = M, prm.k = k, prm.min_sep = 0;
    return lins_host_place_team_topk(Q, qs, qid, 1e6, -1.0, (int)slots.size(), slots.data(), dp.data(), tp.data(), counts.data(), &prm, out);
  }
};

float least_distance(const float* Q, const float* C) {
  float d[kNS];
  lins_host_place_distance(Q, C, d);
  return *std::min_element(d, d + kNS);
}

// tests/team_sizes_cases.py's layout B, built here from cells: slots of 300, 257 and 64 frames (an empty slot between
// them); 63 frames with exactly the query's cells and other heights at places >= 256 of the concatenation, `near` (the
// query less one cell of a column that keeps others: dk 1) and `nearer` (less two cells alone in their columns, in two
// rings: dk 2, d below near's); every other frame far in dk.  The cut of the shortlist at M decides rank 0.
int layout_b_case() {
  std::mt19937 g(4);
  std::uniform_real_distribution<float> u(0.f, 1.f);
  std::unique_ptr<float[]> Q(new float[kCells]);
  std::fill(Q.get(), Q.get() + kCells, 0.f);
  std::vector<int> cells;
  while ((int)cells.size() < 140) {
    const int c = (int)(g() % kCells);
    if (Q[c] == 0.f) Q[c] = 0.5f + 5.5f * u(g), cells.push_back(c);
  }
  int per_col[kNS] = {0};
  for (int c : cells) per_col[c % kNS] += 1;
  int shared = -1, alone_a = -1, alone_b = -1;
  for (int c : cells) {
    if (per_col[c % kNS] >= 3 && shared < 0) shared = c;
    if (per_col[c % kNS] == 1 && alone_a < 0) alone_a = c;
    else if (per_col[c % kNS] == 1 && alone_a >= 0 && alone_b < 0 && c / kNS != alone_a / kNS) alone_b = c;
  }
  CHECK(shared >= 0 && alone_a >= 0 && alone_b >= 0);
  Team T;
  const int n[] = {300, 0, 257, 64}, slot_of[] = {2, 3, 4, 5};
  float* D[4];
  for (int t = 0; t < 4; ++t) {
    D[t] = T.add(slot_of[t], n[t]);
    for (int c = 0; c < n[t]; ++c) random_desc(g, 0.3f, D[t] + (size_t)c * kCells);
  }
  const int same_at[3][2] = {{0, 262}, {2, 215}, {3, 20}};  // (target, first id): 21 frames each
  for (const auto& at : same_at)
    for (int i = 0; i < 21; ++i) {
      float* d = D[at[0]] + (size_t)(at[1] + i) * kCells;
      for (int c = 0; c < kCells; ++c) d[c] = Q[c] != 0.f ? 0.5f + 5.5f * u(g) : 0.f;
    }
  float* near = D[2] + (size_t)250 * kCells;
  float* nearer = D[0] + (size_t)5 * kCells;
  std::memcpy(near, Q.get(), kCells * sizeof(float)), std::memcpy(nearer, Q.get(), kCells * sizeof(float));
  near[shared] = 0.f, nearer[alone_a] = 0.f, nearer[alone_b] = 0.f;
  // the statement: sort the keys
  RingKey kq, kc;
  ring_key(Q.get(), 0.0, &kq);
  std::vector<std::tuple<int, int, int>> order;
  for (int t = 0; t < 4; ++t)
    for (int c = 0; c < n[t]; ++c) ring_key(D[t] + (size_t)c * kCells, 0.0, &kc), order.emplace_back(key_distance(kq, kc), slot_of[t], c);
  std::sort(order.begin(), order.end());
  CHECK(std::get<0>(order[62]) == 0 && order[63] == std::make_tuple(1, 4, 250) && order[64] == std::make_tuple(2, 2, 5) && std::get<0>(order[65]) > 2);
  const float d_near = least_distance(Q.get(), near), d_nearer = least_distance(Q.get(), nearer);
  CHECK(d_nearer < d_near);
  std::unique_ptr<lins_place_team_result[]> out(new lins_place_team_result[kMaxK]);
  CHECK(T.topk(Q.get(), 7, 3, 64, kMaxK, out.get()) == kMaxK);
  CHECK(out[0].slot == 4 && out[0].id == 250 && out[0].dk == 1 && out[0].distance == d_near && out[0].candidates == 621);
  for (int j = 1; j < kMaxK; ++j) CHECK(out[j].dk == 0 && out[j].distance > d_near && out[j - 1].distance <= out[j].distance);
  CHECK(T.topk(Q.get(), 7, 3, 63, kMaxK, out.get()) == kMaxK);
  for (int j = 0; j < kMaxK; ++j) CHECK(out[j].dk == 0);  // near is not among them
  // M <= 8 ranks show the whole shortlist
  for (int M = 1; M <= kMaxK; ++M) {
    CHECK(T.topk(Q.get(), 7, 3, M, kMaxK, out.get()) == M);
    std::vector<std::tuple<int, int, int>> got;
    for (int j = 0; j < M; ++j) got.emplace_back(out[j].dk, out[j].slot, out[j].id);
    std::sort(got.begin(), got.end());
    CHECK(std::equal(got.begin(), got.end(), order.begin()));
  }
  return 0;
}

// layout C: the ends of the key's range — no cell, one cell, one column, every cell, every cell but one ring's — in a pair
// of slots, the second in reverse; each asks in turn
int layout_c_case() {
  const int kinds = 5;
  auto fill = [](int kind, float* d) {
    for (int r = 0; r < kNR; ++r)
      for (int s = 0; s < kNS; ++s) {
        const bool on = kind == 0 ? false : kind == 1 ? (r == 2 && s == 33) : kind == 2 ? s == 32 : kind == 3 ? true : r != 13;
        d[r * kNS + s] = on ? 0.5f + 0.25f * (float)((7 * r + 3 * s) % 11) : 0.f;
      }
  };
  Team T;
  float* A = T.add(8, kinds);
  float* B = T.add(9, kinds);
  for (int i = 0; i < kinds; ++i) fill(i, A + (size_t)i * kCells), fill(i, B + (size_t)(kinds - 1 - i) * kCells);
  RingKey key[kinds];
  for (int i = 0; i < kinds; ++i) ring_key(A + (size_t)i * kCells, 0.0, &key[i]);
  CHECK(key[0].sumsq == 0 && key[1].sumsq == 1 && key[2].sumsq == 20 && key[3].sumsq == (unsigned)kMaxKeyDist && key[4].sumsq == 68400);
  CHECK(key_distance(key[0], key[3]) == kMaxKeyDist && key_distance(key[3], key[4]) == 3600 && key_distance(key[0], key[4]) == 68400);
  for (int i = 0; i < kinds; ++i)
    for (int j = 0; j < kinds; ++j) {
      unsigned dot = 0;
      for (int r = 0; r < kNR; ++r) dot += (unsigned)key[i].occ[r] * key[j].occ[r];
      CHECK((unsigned)key_distance(key[i], key[j]) == key[i].sumsq + key[j].sumsq - 2u * dot);  // the form the device takes, at its ends
    }
  std::unique_ptr<lins_place_team_result[]> out(new lins_place_team_result[kMaxK]);
  for (int i = 0; i < kinds; ++i) {
    CHECK(T.topk(A + (size_t)i * kCells, 8, i, 64, kMaxK, out.get()) == kMaxK);
    for (int j = 0; j < kMaxK; ++j) {
      const lins_place_team_result& r = out[j];
      CHECK(r.candidates == 2 * kinds - 1 && !(r.slot == 8 && r.id == i));
      const int kind = r.slot == 8 ? r.id : kinds - 1 - r.id;
      CHECK(r.dk == key_distance(key[i], key[kind]));
      if (i == 0 || kind == 0) CHECK(r.distance == 1.f && r.shift == 0);  // no column to compare
      if (j) CHECK(out[j - 1].distance <= r.distance);
    }
    if (i) CHECK(out[0].slot == 9 && out[0].id == kinds - 1 - i && out[0].dk == 0 && out[0].distance < 1e-6f);  // its twin
    if (i == 0) {  // every d is 1: the ranks are the shortlist's order
      CHECK(out[0].slot == 9 && out[0].id == kinds - 1 && out[0].dk == 0 && out[kMaxK - 1].dk == kMaxKeyDist);
      for (int j = 1; j < kMaxK; ++j)
        CHECK(std::make_tuple(out[j - 1].dk, out[j - 1].slot, out[j - 1].id) < std::make_tuple(out[j].dk, out[j].slot, out[j].id));
    }
  }
  // a shortlist of one: the full frame's holds its twin, the empty frame's the other empty frame
  CHECK(T.topk(A + (size_t)3 * kCells, 8, 3, 1, 1, out.get()) == 1 && out[0].slot == 9 && out[0].id == 1 && out[0].dk == 0);
  CHECK(T.topk(A, 8, 0, 1, 1, out.get()) == 1 && out[0].slot == 9 && out[0].id == kinds - 1 && out[0].dk == 0 && out[0].distance == 1.f);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const char* name = argc > 1 ? argv[1] : "";
  int rc = 2;
  if (!std::strcmp(name, "keys")) rc = keys_case();
  else if (!std::strcmp(name, "select")) rc = select_case();
  else if (!std::strcmp(name, "search")) rc = search_case();
  else if (!std::strcmp(name, "layout_b")) rc = layout_b_case();
  else if (!std::strcmp(name, "layout_c")) rc = layout_c_case();
  if (rc == 0) std::printf("ok %s\n", name);
  return rc;
}
