// team_select_check.cpp — csrc/host/team_select.h, the team selection's one scalar text, as a stand-alone program; built by
// tests/test_team_select_sanitized.py with -fsanitize=address,undefined.  Every buffer is a heap block of exactly its size.
//   team_select_check edges    the contract's corners: no targets, empty targets, a duplicate, ties, the cell rule
//   team_select_check random   seeded teams on a 0.5 m lattice against a quadratic restatement (a hit survives iff no hit
//                              of its cell is smaller in (d, slot, id)), under every rotation of the target list
// stdout: "ok <mode>"; exit 1 with the reason on stderr.
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "host/team_select.h"

using lins_team_select::Pair;

struct Team {
  std::vector<int32_t> slots, counts;
  std::vector<std::vector<lins_key_pose>> poses;
  std::vector<const lins_key_pose*> ptr;
  void add(int slot, const std::vector<lins_key_pose>& p) {
    slots.push_back(slot), counts.push_back((int32_t)p.size()), poses.push_back(p);
    ptr.clear();
    for (auto& v : poses) ptr.push_back(v.empty() ? nullptr : v.data());
  }
  int select(const float c[3], float radius, float leaf, std::vector<Pair>& out, long long* hits = nullptr) const {
    return lins_team_select::select((int)slots.size(), slots.data(), ptr.data(), counts.data(), c, radius, leaf, out, hits);
  }
};

static lins_key_pose at(float x, float y, float z) { return lins_key_pose{x, y, z, 0.f, 0.f, 0.f}; }

static bool same(const std::vector<Pair>& a, const std::vector<Pair>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].slot != b[i].slot || a[i].id != b[i].id) return false;
  return true;
}

#define CHECK(x)                                          \
  do {                                                    \
    if (!(x)) {                                           \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); \
      return 1;                                           \
    }                                                     \
  } while (0)

static int edges() {
  const float o[3] = {0.f, 0.f, 0.f};
  std::vector<Pair> out;
  long long hits = -1;
  {
    Team t;
    CHECK(t.select(o, 5.f, 1.f, out, &hits) == lins_team_select::kOk && out.empty() && hits == 0);
    t.add(3, {}), t.add(1, {});
    CHECK(t.select(o, 5.f, 1.f, out, &hits) == lins_team_select::kOk && out.empty() && hits == 0);
    t.add(3, {at(0, 0, 0)});
    CHECK(t.select(o, 5.f, 1.f, out) == lins_team_select::kDuplicate && out.empty());
  }
  {  // equal d in one cell: the lower slot; in one slot: the lower id; a nearer pose beats both
    Team t;
    const float c[3] = {0.5f, 0.5f, 0.f};
    t.add(2, {at(0.25f, 0.25f, 0)}), t.add(1, {at(9, 9, 9), at(0.75f, 0.75f, 0), at(0.25f, 0.25f, 0)});
    CHECK(t.select(c, 2.f, 1.f, out, &hits) == lins_team_select::kOk && hits == 3 && same(out, {Pair{1, 1}}));
    t.add(5, {at(0.5f, 0.5f, 0)});
    CHECK(t.select(c, 2.f, 1.f, out, &hits) == lins_team_select::kOk && hits == 4 && same(out, {Pair{5, 0}}));
    CHECK(t.select(c, 0.f, 1.f, out, &hits) == lins_team_select::kOk && hits == 1 && same(out, {Pair{5, 0}}));
  }
  {  // floor, not truncation; d == r2 is a hit
    Team t;
    t.add(0, {at(-0.25f, 0, 0), at(0.25f, 0, 0), at(3, 4, 0), at(3, 4, 0.01f)});
    CHECK(t.select(o, 5.f, 1.f, out, &hits) == lins_team_select::kOk && hits == 3 && same(out, {Pair{0, 0}, Pair{0, 1}, Pair{0, 2}}));
  }
  {  // the cell rule: 2e9 + 1 cells along one axis fit, a plane of twice that does not, nor a volume
    Team t;
    t.add(0, {at(-1e6f, 0, 0)}), t.add(1, {at(1e6f, 0, 0)});
    CHECK(t.select(o, 2e6f, 1e-3f, out) == lins_team_select::kOk && same(out, {Pair{0, 0}, Pair{1, 0}}));
    t.add(2, {at(0, 1, 0)});
    CHECK(t.select(o, 2e6f, 1e-3f, out, &hits) == lins_team_select::kTooManyCells && out.empty() && hits == 3);
    Team v;
    v.add(0, {at(0, 0, 0), at(40, 40, 2)});
    CHECK(v.select(o, 100.f, 1e-3f, out) == lins_team_select::kTooManyCells && out.empty());
    CHECK(v.select(o, 100.f, 1.f, out) == lins_team_select::kOk && out.size() == 2);
  }
  CHECK(lins_team_select::leaf_ok(1.f) && !lins_team_select::leaf_ok(0.f) && !lins_team_select::leaf_ok(-1.f) && !lins_team_select::leaf_ok(1e-45f));
  std::printf("ok edges\n");
  return 0;
}

static int random_teams() {
  std::mt19937 rng(11);
  long long mixed = 0, crowded = 0;
  for (int round = 0; round < 120; ++round) {
    const int n_t = 1 + (int)(rng() % 4);
    std::vector<int> slot_of = {0, 1, 2, 3, 4, 5};
    for (int i = 5; i > 0; --i) std::swap(slot_of[i], slot_of[rng() % (i + 1)]);
    std::vector<std::vector<lins_key_pose>> P(n_t);
    for (int t = 0; t < n_t; ++t) {
      const int n = (int)(rng() % 120);
      for (int i = 0; i < n; ++i)
        P[t].push_back(at(0.5f * (float)((int)(rng() % 25) - 12), 0.5f * (float)((int)(rng() % 25) - 12), 0.5f * (float)((int)(rng() % 5) - 2)));
    }
    const float c[3] = {0.25f * (float)((int)(rng() % 9) - 4), 0.25f * (float)((int)(rng() % 9) - 4), 0.f};
    const float radius = 0.5f * (float)(1 + rng() % 12), leaf = 0.5f * (float)(1 + rng() % 4), inv = 1.0f / leaf, r2 = radius * radius;
    // the quadratic restatement
    struct H {
      float d;
      int slot, id;
      long long c[3];
    };
    std::vector<H> h;
    for (int t = 0; t < n_t; ++t)
      for (int i = 0; i < (int)P[t].size(); ++i) {
        const lins_key_pose& p = P[t][i];
        const float dx = p.x - c[0], dy = p.y - c[1], dz = p.z - c[2], d = (dx * dx + dy * dy) + dz * dz;
        if (d <= r2) h.push_back(H{d, slot_of[t], i, {(long long)std::floor(p.x * inv), (long long)std::floor(p.y * inv), (long long)std::floor(p.z * inv)}});
      }
    std::vector<Pair> want;
    for (const H& a : h) {
      bool beaten = false;
      for (const H& b : h)
        if (b.c[0] == a.c[0] && b.c[1] == a.c[1] && b.c[2] == a.c[2] &&
            (b.d < a.d || (b.d == a.d && (b.slot < a.slot || (b.slot == a.slot && b.id < a.id)))))
          beaten = true;
      if (!beaten) want.push_back(Pair{a.slot, a.id});
    }
    std::sort(want.begin(), want.end(), [](const Pair& a, const Pair& b) { return a.slot != b.slot ? a.slot < b.slot : a.id < b.id; });
    for (int rot = 0; rot < n_t; ++rot) {
      Team t;
      for (int j = 0; j < n_t; ++j) t.add(slot_of[(j + rot) % n_t], P[(j + rot) % n_t]);
      std::vector<Pair> out;
      long long hits = -1;
      CHECK(t.select(c, radius, leaf, out, &hits) == lins_team_select::kOk);
      CHECK(hits == (long long)h.size());
      CHECK(same(out, want));
    }
    crowded += h.size() > want.size();
    int first = want.empty() ? -1 : want[0].slot;
    for (const Pair& p : want) mixed += p.slot != first ? 1 : 0, first = p.slot;
  }
  CHECK(crowded > 60 && mixed > 60);  // (cells with several hits; teams whose answer mixes slots)
  std::printf("ok random\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "edges") return edges();
  if (mode == "random") return random_teams();
  std::fprintf(stderr, "usage: team_select_check edges|random\n");
  return 2;
}
