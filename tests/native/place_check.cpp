// place_check.cpp — the place-recognition restatement (csrc/host/place.cpp) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_place_sanitized.py.  Every cloud, descriptor and time list lives in a heap
// block of exactly its size: the sanitizers are the witness that nothing reads or writes beyond it, and that the cell
// arithmetic (float -> int conversions, the 60-bit shifts of the packed keys) stays defined at the contract's edges.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/lins_host.h"

#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
      return 1;                                             \
    }                                                       \
  } while (0)

namespace {

struct Frame {
  std::vector<lins_point> c[3];
  lins_keyframe view() {
    lins_keyframe f;
    std::memset(&f, 0, sizeof f);
    f.corner = c[0].empty() ? nullptr : c[0].data(), f.surf = c[1].empty() ? nullptr : c[1].data(), f.outlier = c[2].empty() ? nullptr : c[2].data();
    f.n_corner = (int)c[0].size(), f.n_surf = (int)c[1].size(), f.n_outlier = (int)c[2].size();
    return f;
  }
};

// up = 1: (x, y, z) = (b, up, a)
lins_point pt(float a, float b, float h_raw) { return lins_point{b, h_raw, a, 0.f}; }

int positives(const float* D) {
  int n = 0;
  for (int i = 0; i < LINS_PLACE_CELLS; ++i) n += D[i] > 0.f;
  return n;
}

}  // namespace

int main(int argc, char** argv) {
  const char* name = argc > 1 ? argv[1] : "";
  lins_place_params prm;
  lins_place_default_params(&prm);
  std::vector<float> D(LINS_PLACE_CELLS), D2(LINS_PLACE_CELLS), d(LINS_PLACE_SECTORS);
  if (!std::strcmp(name, "edges")) {
    Frame f;
    lins_keyframe v = f.view();
    CHECK(lins_host_place_descriptor(&v, &prm, D.data()) == LINS_OK && positives(D.data()) == 0);  // the empty frame
    CHECK(lins_host_place_distance(D.data(), D.data(), d.data()) == LINS_OK);
    for (int k = 0; k < LINS_PLACE_SECTORS; ++k) CHECK(d[k] == 1.f);
    const float floor_raw = 0x1p-10f - 2.f;
    f.c[0] = {pt(0.f, 0.f, 1.f)};                                       // rho == 0
    f.c[1] = {pt(80.f, 0.f, 1.f), pt(4.f, 0.f, 1.f), pt(-9.f, 0.f, 1.f), pt(-17.f, -0.f, 1.f), pt(79.99999f, 0.f, 1.f)};
    f.c[2] = {pt(30.f, 1.f, std::nextafter(floor_raw, -3.f)), pt(40.f, 1.f, floor_raw), pt(50.f, 1.f, std::nextafter(floor_raw, 0.f)),
              pt(1e6f, 1e6f, 1e6f), pt(-1e6f, 1e6f, -1e6f)};
    v = f.view();
    CHECK(lins_host_place_descriptor(&v, &prm, D.data()) == LINS_OK);
    CHECK(positives(D.data()) == 7);  // all but the point at r_max, the one below the floor and the two far ones
    CHECK(D[1 * LINS_PLACE_SECTORS + 30] == 3.f);  // azimuth exactly 0: sector 30
    CHECK(D[2 * LINS_PLACE_SECTORS + 59] == 3.f && D[4 * LINS_PLACE_SECTORS + 0] == 3.f);
    CHECK(lins_host_place_distance(D.data(), D.data(), d.data()) == LINS_OK && d[0] <= 1e-6f);
    prm.clouds = LINS_SUBMAP_OUTLIER;
    CHECK(lins_host_place_descriptor(&v, &prm, D2.data()) == LINS_OK && positives(D2.data()) == 2);
    f.c[2][0].x = std::numeric_limits<float>::quiet_NaN();
    v = f.view();
    CHECK(lins_host_place_descriptor(&v, &prm, D2.data()) == LINS_E_INPUT);
    prm.up_axis = 3;
    CHECK(lins_host_place_descriptor(&v, &prm, D2.data()) == LINS_E_ARG);
  } else if (!std::strcmp(name, "search")) {
    Frame f;
    for (int i = 0; i < 200; ++i) {
      const float th = 0.031f * (float)i, rho = 1.f + 0.39f * (float)i;
      f.c[i % 3].push_back(pt(rho * std::cos(th), rho * std::sin(th), 0.01f * (float)(i % 37)));
    }
    lins_keyframe v = f.view();
    CHECK(lins_host_place_descriptor(&v, &prm, D.data()) == LINS_OK);
    const int n = 5;
    std::vector<float> descs((size_t)n * LINS_PLACE_CELLS, 0.f);
    std::vector<double> times = {0.0, 1.0, 2.0, 3.0, 9.0};
    for (int c = 1; c < n; ++c) std::memcpy(descs.data() + (size_t)c * LINS_PLACE_CELLS, D.data(), LINS_PLACE_CELLS * sizeof(float));
    int32_t id = -5, shift = -5, cand = -5;
    float dist = -1.f;
    CHECK(lins_host_place_search(D.data(), descs.data(), times.data(), n, 1, 10.0, 1.0, &id, &shift, &dist, &cand) == LINS_OK);
    CHECK(id == 2 && shift == 0 && dist <= 1e-6f && cand == 3);  // 0: empty (d = 1), 1: skipped, 4: at the gate
    CHECK(lins_host_place_search(D.data(), descs.data(), times.data(), n, -1, 10.0, 20.0, &id, &shift, &dist, &cand) == LINS_OK);
    CHECK(id == -1 && shift == 0 && dist == 1.f && cand == 0);
    CHECK(lins_host_place_search(D.data(), nullptr, nullptr, 0, -1, 10.0, 1.0, &id, &shift, &dist, nullptr) == LINS_OK && id == -1);
    CHECK(lins_host_place_search(D.data(), descs.data(), times.data(), n, -1, 10.0, NAN, &id, &shift, &dist, &cand) == LINS_E_INPUT);
    lins_key_pose a = {1.f, 2.f, 3.f, 0.1f, 0.2f, 0.3f}, b = {-4.f, 0.f, 1.f, -0.2f, 0.1f, 2.f};
    std::vector<double> T(16);
    for (int up = 0; up < 3; ++up)
      for (int k = 0; k < LINS_PLACE_SECTORS; k += 59) CHECK(lins_host_place_guess(&a, &b, k, up, T.data()) == LINS_OK && T[15] == 1.0);
    CHECK(lins_host_place_guess(&a, &b, 60, 1, T.data()) == LINS_E_ARG);
  } else {
    std::printf("usage: place_check edges|search\n");
    return 2;
  }
  std::printf("ok %s\n", name);
  return 0;
}
