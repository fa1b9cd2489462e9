// place_topk_check.cpp — lins_host_place_topk and lins_host_loop_choose (csrc/host/place.cpp, csrc/host/loop_icp.cpp) as a
// stand-alone program, built with -fsanitize=address,undefined by tests/test_place_topk_sanitized.py.  Every descriptor,
// time list and result array lives in a heap block of exactly its size — the k results of an entry whose ranks fall short
// of k included: the sanitizers are the witness that the unfilled ranks are written inside the block and nothing beyond it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// up = 1: (x, y, z) = (b, up, a)
lins_point pt(float a, float b, float h_raw) { return lins_point{b, h_raw, a, 0.f}; }

// a place of 150 points that depends on `seed`
void describe(int seed, const lins_place_params* prm, float* D) {
  std::vector<lins_point> c;
  for (int i = 0; i < 150; ++i) {
    const float th = 0.041f * (float)i + 0.7f * (float)seed, rho = 1.f + 0.5f * (float)((i * (seed + 3)) % 150);
    c.push_back(pt(rho * std::cos(th), rho * std::sin(th), 0.02f * (float)((i + 5 * seed) % 41)));
  }
  lins_keyframe f;
  std::memset(&f, 0, sizeof f);
  f.surf = c.data(), f.n_surf = (int)c.size();
  if (lins_host_place_descriptor(&f, prm, D) != LINS_OK) std::abort();
}

}  // namespace

int main(int argc, char** argv) {
  const char* name = argc > 1 ? argv[1] : "";
  lins_place_params prm;
  lins_place_default_params(&prm);
  if (!std::strcmp(name, "topk")) {
    const int n = 9;
    std::vector<float> q(LINS_PLACE_CELLS), descs((size_t)n * LINS_PLACE_CELLS);
    std::vector<double> times(n);
    describe(2, &prm, q.data());
    for (int c = 0; c < n; ++c) describe(c % 4, &prm, descs.data() + (size_t)c * LINS_PLACE_CELLS), times[c] = c;  // 2 and 6 are the query's twins
    for (int k = 1; k <= LINS_PLACE_MAX_K; ++k) {
      for (int sep : {0, 1, 3, 100}) {
        std::vector<int32_t> ids(k, -7), sh(k, -7);
        std::vector<float> d(k, -7.f);
        int32_t cand = -7;
        const int filled = lins_host_place_topk(q.data(), descs.data(), times.data(), n, -1, 100.0, -1.0, k, sep, ids.data(), sh.data(), d.data(), &cand);
        CHECK(filled >= 1 && filled <= k && cand == n);
        CHECK(ids[0] == 2 && sh[0] == 0 && d[0] <= 1e-6f);  // the lower of the two twins
        if (k > 1 && sep <= 3) CHECK(ids[1] == 6 && d[1] == d[0]);
        if (sep == 100) CHECK(filled == 1);
        for (int j = 0; j < k; ++j) {
          if (j < filled) {
            CHECK(ids[j] >= 0 && ids[j] < n && sh[j] >= 0 && sh[j] < LINS_PLACE_SECTORS && d[j] >= 0.f && d[j] <= 1.f);
            for (int i = 0; i < j; ++i) CHECK(std::abs(ids[j] - ids[i]) > sep && d[i] <= d[j]);
          } else {
            CHECK(ids[j] == -1 && sh[j] == 0 && d[j] == 1.f);
          }
        }
      }
    }
    // the ranks fall short of k: two admissible candidates, then none, then no candidates at all
    {
      const int k = LINS_PLACE_MAX_K;
      std::vector<int32_t> ids(k, -7), sh(k, -7);
      std::vector<float> d(k, -7.f);
      int32_t cand = -7;
      CHECK(lins_host_place_topk(q.data(), descs.data(), times.data(), n, 1, 0.0, 6.5, k, 0, ids.data(), sh.data(), d.data(), &cand) == 2 && cand == 2);
      CHECK((ids[0] == 7 && ids[1] == 8) || (ids[0] == 8 && ids[1] == 7));  // times 7 and 8 lie beyond the gap
      CHECK(ids[2] == -1 && ids[k - 1] == -1 && d[k - 1] == 1.f);
      CHECK(lins_host_place_topk(q.data(), descs.data(), times.data(), n, -1, 4.0, 50.0, k, 0, ids.data(), sh.data(), d.data(), &cand) == 0 && cand == 0);
      CHECK(ids[0] == -1 && sh[0] == 0 && d[0] == 1.f);
      CHECK(lins_host_place_topk(q.data(), nullptr, nullptr, 0, -1, 4.0, -1.0, k, 0, ids.data(), sh.data(), d.data(), nullptr) == 0 && ids[0] == -1);
      CHECK(lins_host_place_topk(q.data(), descs.data(), times.data(), n, -1, 4.0, -1.0, 0, 0, ids.data(), sh.data(), d.data(), &cand) == LINS_E_ARG);
      CHECK(lins_host_place_topk(q.data(), descs.data(), times.data(), n, -1, 4.0, -1.0, k + 1, 0, ids.data(), sh.data(), d.data(), &cand) == LINS_E_ARG);
      CHECK(lins_host_place_topk(q.data(), descs.data(), times.data(), n, -1, 4.0, -1.0, k, -1, ids.data(), sh.data(), d.data(), &cand) == LINS_E_ARG);
      CHECK(lins_host_place_topk(q.data(), descs.data(), times.data(), n, -1, 4.0, NAN, k, 0, ids.data(), sh.data(), d.data(), &cand) == LINS_E_INPUT);
    }
  } else if (!std::strcmp(name, "choose")) {
    std::vector<int32_t> conv = {1, 1, 0, 1};
    std::vector<double> fit = {0.2, 0.1, 0.01, 0.1};
    CHECK(lins_host_loop_choose(4, conv.data(), fit.data(), 0.3f) == 1);  // the tie of ranks 1 and 3 goes to the lower; rank 2 did not converge
    CHECK(lins_host_loop_choose(1, conv.data(), fit.data(), 0.3f) == 0);
    CHECK(lins_host_loop_choose(4, conv.data(), fit.data(), 0.05f) == -1);
    CHECK(lins_host_loop_choose(0, conv.data(), fit.data(), 0.3f) == -1 && lins_host_loop_choose(0, nullptr, nullptr, 0.3f) == -1);
  } else {
    std::printf("usage: place_topk_check topk|choose\n");
    return 2;
  }
  std::printf("ok %s\n", name);
  return 0;
}
