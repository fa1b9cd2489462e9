// team_graph_check.cpp — the team graph's text (csrc/pose_graph_team.h) and its CPU restatement (csrc/host/team_graph.cpp,
// on csrc/host/pose_graph.cpp) as a stand-alone program; built by tests/test_team_graph_sanitized.py with
// -fsanitize=address,undefined.  Every array the solve works on is a heap block of exactly its size.
//   team_graph_check tables   the member table and the loops' supports: the rows, the prefix rows and the first unknowns of
//                             groups of 1 .. 32 members; every pair of supports cut (team_cut) against the signs written out
//                             row by row
//   team_graph_check solve    small groups through lins_host_team_graph_solve: a root alone, a factor at the anchor's frame
//                             0, members around the prefix block with a loop of their own, three members in a chain; a
//                             group of one against lins_host_pose_graph_solve bit for bit
// stdout: "ok <mode>"; exit 1 with the reason on stderr.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "host/pose_graph_host.h"
#include "pose_graph_team.h"

using namespace lins_pg;

#define CHECK(x)                                          \
  do {                                                    \
    if (!(x)) {                                           \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); \
      return 1;                                           \
    }                                                     \
  } while (0)

static int tables() {
  std::mt19937 rng(5);
  for (int nm = 1; nm <= kTeamMaxMembers; ++nm) {
    std::vector<int> counts(nm);
    std::vector<const double*> var(nm, nullptr);
    const double v[6] = {1, 2, 3, 4, 5, 6};
    for (int m = 0; m < nm; ++m) counts[m] = 1 + (int)(rng() % 70), var[m] = (m % 2) ? v : nullptr;
    std::vector<TeamMember> mt(nm);
    int q_rows = -1;
    const int frames = team_members(nm, counts.data(), var.data(), mt.data(), &q_rows);
    int off = 0, qoff = 0;
    for (int m = 0; m < nm; ++m) {
      CHECK(mt[m].off == off && mt[m].n == counts[m] && mt[m].qoff == qoff && mt[m].first == (m ? off : 1));
      CHECK(mt[m].var[2] == ((m % 2) ? 3.0 : 1e-6));
      CHECK(team_root_of(mt.data(), nm, off) == m);  // (0 for the anchor: no unknown)
      if (counts[m] > 1) CHECK(team_root_of(mt.data(), nm, off + 1) == 0);
      off += counts[m], qoff += counts[m] / kPrefixBlock + 2;
    }
    CHECK(frames == off && q_rows == qoff);
    if (nm < 2) continue;
    // supports: loops of the members' own and factors between random members; the signs row by row
    std::vector<TeamSpan> spans;
    std::vector<std::vector<int>> sign;
    for (int i = 0; i < 12; ++i) {
      std::vector<int> s(frames, 0);
      if (i % 3 == 0) {
        const int m = (int)(rng() % nm);
        if (counts[m] < 2) continue;
        LoopRec R{};
        R.latest = mt[m].off + (int)(rng() % counts[m]), R.closest = mt[m].off + (int)(rng() % counts[m]);
        if (R.latest == R.closest) continue;
        spans.push_back(team_span_own(R));
        for (int k = loop_lo(R) + 1; k <= loop_hi(R); ++k) s[k] = 1;
      } else {
        const int ma = (int)(rng() % nm), mb = (ma + 1 + (int)(rng() % (nm - 1))) % nm;
        const int ra = mt[ma].off + (int)(rng() % counts[ma]), rb = mt[mb].off + (int)(rng() % counts[mb]);
        spans.push_back(team_span_factor(mt.data(), mb, rb, ma, ra));
        CHECK(spans.back().lo[0] <= spans.back().lo[1]);  // group order
        for (int k = mt[ma].first; k <= ra; ++k) s[k] = 1;
        for (int k = mt[mb].first; k <= rb; ++k) s[k] = -1;
      }
      sign.push_back(s);
      for (int k = 0; k < frames; ++k) CHECK(team_sign(spans.back(), k) == s[k]);
    }
    for (size_t a = 0; a < spans.size(); ++a)
      for (size_t b = 0; b < spans.size(); ++b) {
        TeamCut c;
        team_cut(spans[a], spans[b], c);
        std::vector<int> got(frames, 0);
        CHECK(c.n[0] >= 0 && c.n[1] >= 0 && (c.n[1] == 0 || (c.n[0] > 0 && c.lo[0] + c.n[0] <= c.lo[1])));
        for (int v2 = 0; v2 < 2; ++v2)
          for (int k = c.lo[v2] + 1; k <= c.lo[v2] + c.n[v2]; ++k) {
            CHECK(k >= 1 && k < frames && got[k] == 0);
            got[k] = c.sg[v2];
            CHECK(team_sign(spans[a], k) == spans[a].sg[c.of[v2]]);
          }
        for (int k = 0; k < frames; ++k) CHECK(got[k] == sign[a][k] * sign[b][k]);
      }
  }
  return 0;
}

static lins_host_pose_graph* chain(int n, unsigned seed, int max_loops) {
  lins_host_pose_graph* g = lins_host_pose_graph_create(n, max_loops);
  std::mt19937 rng(seed);
  std::normal_distribution<float> noise(0.f, 0.01f);
  std::vector<float> aft(6 * (size_t)n);
  for (int k = 0; k < n; ++k) {
    const float yaw = 0.3f + 0.02f * k;
    float* p = &aft[6 * (size_t)k];
    p[0] = 0.01f + noise(rng) * 0.2f, p[1] = yaw, p[2] = -0.01f + noise(rng) * 0.2f;
    p[5] = 30.f + 20.f * std::cos(yaw) + noise(rng), p[3] = -20.f + 20.f * std::sin(yaw) + noise(rng), p[4] = 0.01f * k + noise(rng);
    if (lins_host_pose_graph_push(g, k ? &aft[6 * (size_t)(k - 1)] : nullptr, p) != k) return nullptr;
  }
  return g;
}

// a factor between frame ib of b and frame ia of a: their relative pose as pushed, moved by d
static lins_team_factor factor(lins_host_pose_graph* const* gs, int mb, int ib, int ma, int ia, double metres, double var) {
  double Tb[12], Ta[12];
  lins_host_pose_graph_poses_f64(gs[mb], ib, 1, Tb), lins_host_pose_graph_poses_f64(gs[ma], ia, 1, Ta);
  lins_team_factor f;
  lins_host_team_factor(Tb, Ta, nullptr, var, &f);
  const double d[6] = {0.004, -0.003, 0.005, metres, -0.5 * metres, 0.25 * metres};
  double Z[12];
  retract(f.Z, d, Z);
  pose_copy(Z, f.Z);
  f.slot_b = mb, f.id_b = ib, f.slot_a = ma, f.id_a = ia;
  return f;
}

static int solve_group(const std::vector<int>& frames, const std::vector<int>& own_loop, const std::vector<std::vector<int>>& fac) {
  std::vector<lins_host_pose_graph*> gs;
  for (size_t m = 0; m < frames.size(); ++m) {
    gs.push_back(chain(frames[m], 100 + (unsigned)m, 2));
    CHECK(gs.back());
    if (own_loop[m]) {
      lins_key_pose pf;
      CHECK(lins_host_pose_graph_poses(gs[m], frames[m] - 1, 1, &pf) == LINS_OK);
      pf.x += 0.05f;
      CHECK(lins_host_pose_graph_add_loop(gs[m], frames[m] - 1, 0, &pf, 1e-6) == LINS_OK);
    }
  }
  std::vector<lins_team_factor> f;
  for (const std::vector<int>& x : fac) f.push_back(factor(gs.data(), x[0], x[1], x[2], x[3], 0.05, 1e-4));
  std::vector<double> rv(6 * frames.size());
  for (size_t i = 0; i < rv.size(); ++i) rv[i] = i % 6 < 3 ? 1e-4 : 1e-2;
  lins_pose_graph_params prm;
  lins_pose_graph_default_params(&prm);
  lins_team_graph_result r, again;
  CHECK(lins_host_team_graph_solve((int)gs.size(), gs.data(), rv.data(), (int)f.size(), f.data(), &prm, &r) == LINS_OK);
  CHECK(r.solve.status == LINS_OK && r.solve.iterations > 0 && r.solve.cost_after < r.solve.cost_before);
  CHECK(r.n_factors == (int)f.size());
  CHECK(lins_host_team_graph_solve((int)gs.size(), gs.data(), rv.data(), (int)f.size(), f.data(), &prm, &again) == LINS_OK);
  // (the solved roots are the priors now: the second solve starts without the root factors' share of the cost)
  CHECK(again.solve.status == LINS_OK && again.solve.cost_before < r.solve.cost_after && again.solve.cost_after <= again.solve.cost_before);
  std::vector<double> rf(6 * f.size() + 1), M(36 * f.size() + 1), rr(6 * gs.size()), H(36 * gs.size()), g(6 * gs.size());
  CHECK(lins_host_team_graph_linearize((int)gs.size(), gs.data(), rv.data(), (int)f.size(), f.data(), nullptr, rf.data(), M.data(), rr.data(),
                                       H.data(), g.data()) == LINS_OK);
  for (lins_host_pose_graph* x : gs) lins_host_pose_graph_destroy(x);
  return 0;
}

static int solve() {
  const int B = kPrefixBlock;
  CHECK(solve_group({6, 1}, {0, 0}, {{1, 0, 0, 3}}) == 0);                                 // a root alone
  CHECK(solve_group({5, 7}, {0, 0}, {{1, 3, 0, 0}}) == 0);                                 // the anchor's side is empty
  CHECK(solve_group({B + 1, 2 * B + 1}, {1, 1}, {{1, B, 0, B - 1}, {0, B, 1, 2 * B}}) == 0);  // block edges, loops of their own, both orders
  CHECK(solve_group({4, 5, 3}, {0, 1, 0}, {{1, 4, 0, 2}, {2, 2, 1, 1}}) == 0);             // a chain of three
  CHECK(solve_group({130, 130}, {0, 0}, {{1, 129, 0, 5}, {1, 3, 0, 120}}) == 0);           // past 256 rows, two factors on one pair
  // a group of one against the single solve
  lins_host_pose_graph *a = chain(40, 9, 2), *b = chain(40, 9, 2);
  CHECK(a && b);
  lins_key_pose pf;
  CHECK(lins_host_pose_graph_poses(a, 39, 1, &pf) == LINS_OK);
  pf.y += 0.3f;
  CHECK(lins_host_pose_graph_add_loop(a, 39, 2, &pf, 1e-6) == LINS_OK && lins_host_pose_graph_add_loop(b, 39, 2, &pf, 1e-6) == LINS_OK);
  lins_pose_graph_params prm;
  lins_pose_graph_default_params(&prm);
  lins_pose_graph_result ra;
  lins_team_graph_result rb;
  CHECK(lins_host_pose_graph_solve(a, &prm, &ra) == LINS_OK && lins_host_team_graph_solve(1, &b, nullptr, 0, nullptr, &prm, &rb) == LINS_OK);
  CHECK(ra.iterations > 0 && std::memcmp(&ra, &rb.solve, sizeof ra) == 0);
  std::vector<double> Ta(12 * 40), Tb(12 * 40);
  lins_host_pose_graph_poses_f64(a, 0, 40, Ta.data()), lins_host_pose_graph_poses_f64(b, 0, 40, Tb.data());
  CHECK(std::memcmp(Ta.data(), Tb.data(), Ta.size() * sizeof(double)) == 0);
  lins_host_pose_graph_destroy(a), lins_host_pose_graph_destroy(b);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  int rc = 2;
  if (mode == "tables") rc = tables();
  else if (mode == "solve") rc = solve();
  else std::fprintf(stderr, "usage: team_graph_check tables|solve\n");
  if (rc == 0) std::printf("ok %s\n", mode.c_str());
  return rc;
}
