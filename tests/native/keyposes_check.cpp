// keyposes_check.cpp — csrc/keypose_select_math.h, the scalar form of the key-pose selection's kernels, held against the
// text it restates (csrc/host/keyframe_select.h) as a stand-alone program; built by tests/test_keyposes_host.py with
// -fsanitize=address,undefined.
//   keyposes_check lists   stdin: one case per line, "<list ids> | <ds ids>"; stdout: kp_surround_list's list, one line
//                          per case; exit 1 (and the case on stderr) where surround_update gives another list
//   keyposes_check keys    the packed key orders as (d, id) over a grid of distances and ids, and sorting the keys of the
//                          kp_dist2 hits gives radius_search's ids on seeded poses with ties; stdout: "ok <comparisons>"
#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "host/keyframe_select.h"
#include "keypose_select_math.h"

static int lists() {
  std::string line;
  int bad = 0;
  while (std::getline(std::cin, line)) {
    std::vector<int> list, ds;
    std::istringstream in(line);
    std::string tok;
    bool right = false;
    while (in >> tok) {
      if (tok == "|")
        right = true;
      else
        (right ? ds : list).push_back(std::stoi(tok));
    }
    int nf = 0;
    for (int v : list) nf = std::max(nf, v + 1);
    for (int v : ds) nf = std::max(nf, v + 1);
    std::vector<int> mark(nf), out(list.size() + ds.size());  // (exactly the sizes the function is promised)
    const int n = lins_kp::kp_surround_list(list.data(), (int)list.size(), ds.data(), (int)ds.size(), mark.data(), nf, out.data());
    out.resize(n);
    std::vector<int> want = list;
    lins_select::surround_update(want, ds);
    if (want != out) std::cerr << "differs: " << line << "\n", bad = 1;
    for (size_t i = 0; i < out.size(); ++i) std::cout << (i ? " " : "") << out[i];
    std::cout << "\n";
  }
  return bad;
}

static int keys() {
  long long compared = 0;
  const float ds[] = {0.f, FLT_TRUE_MIN, FLT_MIN, 1e-20f, 0.99999994f, 1.f, 1.0000001f, 25.f, 25.000002f, 1e6f, 3e12f, FLT_MAX};
  const int ids[] = {0, 1, 2, 63, 64, 8191, 8192, 1 << 24, INT_MAX};
  for (float da : ds)
    for (int ia : ids)
      for (float db : ds)
        for (int ib : ids) {
          const bool want = da < db || (da == db && ia < ib);
          if ((lins_kp::kp_key(da, ia) < lins_kp::kp_key(db, ib)) != want || lins_kp::kp_key_id(lins_kp::kp_key(da, ia)) != ia) {
            std::fprintf(stderr, "key order: (%a, %d) against (%a, %d)\n", da, ia, db, ib);
            return 1;
          }
          ++compared;
        }
  std::mt19937 rng(5);
  for (int round = 0; round < 50; ++round) {
    const int n = 1 + (int)(rng() % 300);
    std::vector<lins_key_pose> poses(n);
    for (int i = 0; i < n; ++i) {  // a coarse lattice: many equal distances, coincident poses, negative coordinates
      poses[i] = lins_key_pose{(float)((int)(rng() % 9) - 4), (float)((int)(rng() % 9) - 4), 0.5f * (float)((int)(rng() % 5) - 2), 0.f, 0.f, 0.f};
    }
    const float centre[3] = {0.f, round % 2 ? 0.25f : 0.f, 0.f}, radius = 0.5f * (float)(round % 9);
    std::vector<int> want;
    lins_select::radius_search(poses.data(), n, centre, radius, want);
    std::vector<uint64_t> keys;
    const float r2 = radius * radius;
    for (int i = 0; i < n; ++i) {
      const float d = lins_kp::kp_dist2(poses[i].x, poses[i].y, poses[i].z, centre[0], centre[1], centre[2]);
      if (d <= r2) keys.push_back(lins_kp::kp_key(d, i));
    }
    std::sort(keys.begin(), keys.end());
    std::vector<int> got;
    for (uint64_t k : keys) got.push_back(lins_kp::kp_key_id(k));
    if (got != want) {
      std::fprintf(stderr, "radius search: round %d\n", round);
      return 1;
    }
    compared += n;
  }
  // the 2^31-cell rule as voxel_grid writes it, where its products do not overflow
  const long long dv[] = {1, 2, 3, 1 << 10, 46340, 46341, 65536, 1ll << 20};  // (a * b * c < 2^63)
  for (long long a : dv)
    for (long long b : dv)
      for (long long c : dv) {
        const bool refused = a * b > (1ll << 31) || a * b * c > (1ll << 31);
        if (lins_kp::kp_cells_fit(a, b, c) == refused) {
          std::fprintf(stderr, "cell rule: %lld %lld %lld\n", a, b, c);
          return 1;
        }
        ++compared;
      }
  if (lins_kp::kp_cells_fit(1ll << 32, 1, 1) || lins_kp::kp_cells_fit(1, 1, (1ll << 31) + 1) || !lins_kp::kp_cells_fit(1ll << 31, 1, 1)) return 1;
  std::printf("ok %lld\n", compared);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "lists") return lists();
  if (mode == "keys") return keys();
  std::fprintf(stderr, "usage: keyposes_check lists|keys\n");
  return 2;
}
