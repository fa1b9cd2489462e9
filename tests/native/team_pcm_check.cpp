// team_pcm_check.cpp — csrc/host/team_pcm.h, the one scalar text of the pairwise-consistent team factors, as a stand-alone
// program; built by tests/test_team_pcm_sanitized.py with -fsanitize=address,undefined.  Every table is a heap block of
// exactly its size (L = 0: a block of no bytes), the stack a block of exactly kLevels words, every result a block of its
// own.
//   team_pcm_check edges    L = 0 and 1, a pair on each bar and one nextafter beyond — rotation, translation, the drift
//                           term —, one frame pair twice, two member pairs, a factor listed from its larger member
//   team_pcm_check cliques  64 and 33 factors that all agree (depth 64, bit 63, the 31 | 32 word edge), k frame pairs x 3
//                           identical factors at k = 9, 10 (the budget on and one short of 81 739 nodes) and 21
//   team_pcm_check random   seeded tables of every size 0 .. 64 against a restatement with explicit 4 x 4 products, an
//                           explicit adjacency matrix and the search as the contract's recursion, backwards and under a seeded
//                           shuffle whose kept mask is mapped back
// stdout: "ok <mode>"; exit 1 with the reason on stderr.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "host/team_pcm.h"

using namespace lins_pcm;

#define CHECK(x)                                          \
  do {                                                    \
    if (!(x)) {                                           \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); \
      return 1;                                           \
    }                                                     \
  } while (0)

static const double kCos5 = 0.99619469809174555;

static void identity(double* T) {
  for (int i = 0; i < 12; ++i) T[i] = 0.0;
  T[0] = T[4] = T[8] = 1.0;
}

// a factor between members u < v on frames (iu, iv) that claims the translation (x, y, z), turned by the yaw (c, s); the
// robots stand at the origin, so X is Z itself
static Rec shift(double x, double y, double z, int iu, int iv, int u = 0, int v = 1, double c = 1.0, double s = 0.0) {
  Rec r;
  std::memset(&r, 0, sizeof r);
  identity(r.Z), identity(r.Tu), identity(r.Tv);
  r.Z[0] = c, r.Z[1] = -s, r.Z[3] = s, r.Z[4] = c;
  r.Z[9] = x, r.Z[10] = y, r.Z[11] = z;
  r.tag = Tag{u, v, iu, iv};
  return r;
}

static lins_team_pcm_params params(double max_t = 1.0, double min_cos = kCos5, double per_frame = 0.0, int min_support = 1, int max_nodes = 65536) {
  lins_team_pcm_params p;
  default_params(&p);
  p.max_translation = max_t, p.min_cos_rotation = min_cos, p.translation_per_frame = per_frame, p.min_support = min_support, p.max_nodes = max_nodes;
  return p;
}

// the call as lins_host_team_factors_consistent makes it, over heap copies of exactly the sizes
static int run(const std::vector<Rec>& t, const lins_team_pcm_params& prm, lins_team_pcm_result* out) {
  if (!params_ok(&prm)) return LINS_E_ARG;
  std::unique_ptr<Rec[]> block(new Rec[t.size()]);
  if (!t.empty()) std::memcpy(block.get(), t.data(), t.size() * sizeof(Rec));
  std::unique_ptr<uint64_t[]> stack(new uint64_t[kLevels]);
  std::unique_ptr<lins_team_pcm_result> res(new lins_team_pcm_result);
  evaluate(block.get(), (int)t.size(), prm, stack.get(), res.get());
  *out = *res;
  return LINS_OK;
}

static bool kept(const lins_team_pcm_result& r, int f) { return (r.kept[f >> 5] >> (f & 31)) & 1u; }
static bool is(const lins_team_pcm_result& r, int n, int n_kept, int n_pairs, int n_pairs_kept, int exact) {
  return r.n_factors == n && r.n_kept == n_kept && r.n_pairs == n_pairs && r.n_pairs_kept == n_pairs_kept && r.exact == exact;
}

static int edges() {
  const double one = std::nextafter(1.0, 2.0);
  lins_team_pcm_result r;
  CHECK(run({}, params(), &r) == LINS_OK && is(r, 0, 0, 0, 0, 1) && r.nodes_max == 0 && r.kept[0] == 0 && r.kept[1] == 0);
  CHECK(run({shift(1, 2, 3, 4, 5)}, params(), &r) == LINS_OK && is(r, 1, 1, 1, 1, 1) && r.nodes_max == 1 && r.kept[0] == 1);
  CHECK(run({shift(1, 2, 3, 4, 5)}, params(1.0, kCos5, 0.0, 2), &r) == LINS_OK && is(r, 1, 0, 1, 0, 1) && r.kept[0] == 0);
  const lins_team_pcm_params two = params(1.0, kCos5, 0.0, 2);
  {  // the translation bar: integers, so nothing rounds
    CHECK(run({shift(3, 0, 0, 0, 0), shift(4, 0, 0, 1, 1)}, two, &r) == LINS_OK && is(r, 2, 2, 1, 1, 1) && r.kept[0] == 3);
    CHECK(run({shift(0, 0, 0, 0, 0), shift(one, 0, 0, 1, 1)}, two, &r) == LINS_OK && is(r, 2, 0, 1, 0, 1));
    CHECK(run({shift(0, 0, 0, 0, 0), shift(0, 0, 0, 1, 1)}, params(0.0, kCos5, 0.0, 2), &r) == LINS_OK && is(r, 2, 2, 1, 1, 1));  // (a bar of zero admits an equal pair)
    // where the robot stood: a turned claim agrees at the origin and not 100 m from it
    Rec far = shift(0, 0, 0, 1, 1, 0, 1, std::cos(0.02), std::sin(0.02));
    CHECK(run({shift(0, 0, 0, 0, 0), far}, two, &r) == LINS_OK && is(r, 2, 2, 1, 1, 1));
    far.Tv[9] = 100.0, far.Z[9] = 100.0;  // (X = Tu Z Tv^-1 turns about where v stood: p itself does not move, the other's p does)
    Rec at = shift(0, 0, 0, 0, 0);
    at.Tv[10] = 100.0, at.Z[10] = 100.0;
    CHECK(run({at, far}, two, &r) == LINS_OK && is(r, 2, 0, 1, 0, 1));
  }
  {  // the rotation bar
    const Rec a = shift(0, 0, 0, 0, 0), b = shift(0, 0, 0, 1, 1);
    CHECK(run({a, b}, params(1.0, 1.0, 0.0, 2), &r) == LINS_OK && is(r, 2, 2, 1, 1, 1));
    CHECK(run({a, b}, params(1.0, one, 0.0, 2), &r) == LINS_OK && is(r, 2, 0, 1, 0, 1));
    const double c = std::cos(0.1), s = std::sin(0.1);  // the trace of I^T Rz is (c + c) + 1, and 1 + 2 c the same sum
    CHECK(run({a, shift(0, 0, 0, 1, 1, 0, 1, c, s)}, params(1.0, c, 0.0, 2), &r) == LINS_OK && is(r, 2, 2, 1, 1, 1));
    CHECK(run({a, shift(0, 0, 0, 1, 1, 0, 1, c, s)}, params(1.0, std::nextafter(c, 2.0), 0.0, 2), &r) == LINS_OK && is(r, 2, 0, 1, 0, 1));
  }
  {  // the drift term: 2^-5 m a frame over |5 - 13| + |15 - 7| = 16 frames is half a metre exactly, t = 1.5
    const lins_team_pcm_params drift = params(1.0, kCos5, 0.03125, 2);
    CHECK(run({shift(0, 0, 0, 5, 15), shift(1.5, 0, 0, 13, 7)}, drift, &r) == LINS_OK && is(r, 2, 2, 1, 1, 1));
    CHECK(run({shift(0, 0, 0, 13, 7), shift(0, 1.5, 0, 5, 15)}, drift, &r) == LINS_OK && is(r, 2, 2, 1, 1, 1));
    CHECK(run({shift(0, 0, 0, 5, 15), shift(std::nextafter(1.5, 2.0), 0, 0, 13, 7)}, drift, &r) == LINS_OK && is(r, 2, 0, 1, 0, 1));
    CHECK(run({shift(0, 0, 0, 5, 15), shift(1.5, 0, 0, 13, 8)}, drift, &r) == LINS_OK && is(r, 2, 0, 1, 0, 1));  // (15 frames: 1.46875 m)
    CHECK(run({shift(0, 0, 0, 5, 15), shift(1.5, 0, 0, 13, 7)}, two, &r) == LINS_OK && is(r, 2, 0, 1, 0, 1));
    CHECK(run({shift(0, 0, 0, 0, 0), shift(1.5, 0, 0, 2147483647, 2147483647)}, params(1.0, kCos5, 1e-10, 2), &r) == LINS_OK && is(r, 2, 0, 1, 0, 1));
    CHECK(run({shift(0, 0, 0, 0, 0), shift(1.5, 0, 0, 2147483647, 2147483647)}, params(1.0, kCos5, 1e-9, 2), &r) == LINS_OK && is(r, 2, 2, 1, 1, 1));
  }
  {  // one frame pair twice: the earlier one stays; two member pairs do not mix; a factor listed from its larger member
    CHECK(run({shift(0, 0, 0, 5, 5), shift(0, 0, 0, 5, 5), shift(0, 0, 0, 9, 9), shift(0, 0, 0, 5, 9)}, params(1.0, kCos5, 0.0, 3), &r) == LINS_OK &&
          is(r, 4, 3, 1, 1, 1) && r.kept[0] == 0b1101);
    CHECK(run({shift(0, 0, 0, 1, 1, 0, 1), shift(0, 0, 0, 2, 2, 0, 2), shift(0, 0, 0, 3, 3, 0, 1), shift(0, 0, 0, 4, 4, 1, 2)}, two, &r) == LINS_OK &&
          is(r, 4, 2, 3, 1, 1) && r.kept[0] == 0b0101);
    Rec flipped = shift(-7, 0, 0, 2, 2);  // Zn = inverse(Z): the claim is + 7
    flipped.flip = 1;
    CHECK(run({shift(7, 0, 0, 1, 1), flipped}, two, &r) == LINS_OK && is(r, 2, 2, 1, 1, 1));
    flipped.flip = 0;
    CHECK(run({shift(7, 0, 0, 1, 1), flipped}, two, &r) == LINS_OK && is(r, 2, 0, 1, 0, 1));
  }
  {  // the parameters' ranges
    const double nan = std::nan(""), inf = INFINITY;
    for (const lins_team_pcm_params& p : {params(-1.0), params(inf), params(nan), params(1.0, nan), params(1.0, kCos5, -1e-300), params(1.0, kCos5, inf),
                                          params(1.0, kCos5, nan), params(1.0, kCos5, 0.0, 0), params(1.0, kCos5, 0.0, 1, 0)})
      CHECK(run({shift(0, 0, 0, 0, 0)}, p, &r) == LINS_E_ARG);
  }
  std::printf("ok edges\n");
  return 0;
}

static std::vector<Rec> duplicates(int k) {
  std::vector<Rec> t;
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < 3; ++j) t.push_back(shift(0.001 * i, 0, 0, i, 2 * i));
  return t;
}

static int cliques() {
  lins_team_pcm_result r;
  for (int L : {64, 33}) {
    std::vector<Rec> t;
    for (int i = 0; i < L; ++i) t.push_back(shift(0.001 * i, 0, 0, i, 100 - i));
    CHECK(run(t, params(1.0, kCos5, 0.0, 3), &r) == LINS_OK && is(r, L, L, 1, 1, 1) && r.nodes_max == (uint32_t)L);
    CHECK(r.kept[0] == 0xffffffffu && r.kept[1] == (L == 64 ? 0xffffffffu : 1u));
    CHECK(run(t, params(1.0, kCos5, 0.0, L + 1), &r) == LINS_OK && is(r, L, 0, 1, 0, 1));
    // a budget one node short of the deepest chain: the first subproblem stops a vertex short, the second one finds L - 1
    CHECK(run(t, params(1.0, kCos5, 0.0, 3, L - 1), &r) == LINS_OK && is(r, L, L - 1, 1, 1, 0) && r.nodes_max == (uint32_t)L && !kept(r, 0) && kept(r, L - 1));
  }
  const lins_team_pcm_params three = params(1.0, kCos5, 0.0, 3);
  CHECK(run(duplicates(9), three, &r) == LINS_OK && is(r, 27, 9, 1, 1, 1) && r.nodes_max == 23087u);
  for (int f = 0; f < 27; ++f) CHECK(kept(r, f) == (f % 3 == 0));
  CHECK(run(duplicates(10), params(1.0, kCos5, 0.0, 3, 81739), &r) == LINS_OK && is(r, 30, 10, 1, 1, 1) && r.nodes_max == 81739u);
  for (int budget : {81738, 65536}) {
    CHECK(run(duplicates(10), params(1.0, kCos5, 0.0, 3, budget), &r) == LINS_OK && is(r, 30, 10, 1, 1, 0) && r.nodes_max == (uint32_t)budget + 1u);
    for (int f = 0; f < 30; ++f) CHECK(kept(r, f) == (f % 3 == 0));
  }
  CHECK(run(duplicates(21), three, &r) == LINS_OK && is(r, 63, 21, 1, 1, 0) && r.nodes_max == 65537u);
  for (int f = 0; f < 63; ++f) CHECK(kept(r, f) == (f % 3 == 0));
  std::printf("ok cliques\n");
  return 0;
}

// ---- the restatement ----
struct M4 {
  double m[4][4];
};
static M4 of_pose(const double* T) {
  M4 a;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) a.m[i][j] = T[3 * i + j];
    a.m[i][3] = T[9 + i];
  }
  a.m[3][0] = a.m[3][1] = a.m[3][2] = 0.0, a.m[3][3] = 1.0;
  return a;
}
static M4 mul(const M4& a, const M4& b) {  // every sum left to right: the fourth term adds a zero, or the translation as it is
  M4 c;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) c.m[i][j] = ((a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j]) + a.m[i][2] * b.m[2][j]) + a.m[i][3] * b.m[3][j];
  return c;
}
static M4 inv(const M4& a) {
  M4 c = of_pose(std::vector<double>(12, 0.0).data());
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) c.m[i][j] = a.m[j][i];
    c.m[i][3] = -((a.m[0][i] * a.m[0][3] + a.m[1][i] * a.m[1][3]) + a.m[2][i] * a.m[2][3]);
  }
  return c;
}

struct Search {
  const std::vector<char>* adj;
  int n;
  long long nodes, max_nodes;
  std::vector<int> best, cur;
  bool exhausted;
  void visit(const std::vector<int>& P) {
    if (exhausted) return;
    if (++nodes > max_nodes) {
      exhausted = true;
      return;
    }
    if (P.empty()) {
      if (cur.size() > best.size()) best = cur;
      return;
    }
    for (size_t k = 0; k < P.size(); ++k) {
      if (exhausted || cur.size() + (P.size() - k) <= best.size()) return;
      const int w = P[k];
      std::vector<int> next;
      for (size_t j = k + 1; j < P.size(); ++j)
        if ((*adj)[(size_t)w * n + P[j]]) next.push_back(P[j]);
      cur.push_back(w);
      visit(next);
      cur.pop_back();
    }
  }
};

static int random_tables() {
  std::mt19937 rng(29);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  long long cliques_of_three = 0, same_under_shuffle = 0, kept_tables = 0;
  for (int L = 0; L <= kMaxFactors; ++L) {
    std::vector<Rec> t;
    for (int i = 0; i < L; ++i) {
      // three member pairs, two claims 30 m apart, a yaw of up to 4 degrees either way, 0.6 m of scatter, ten frames a chain
      const double yaw = (u(rng) - 0.5) * 0.14, c = std::cos(yaw), s = std::sin(yaw);
      const int pair = (int)(rng() % 3);
      Rec r = shift(30.0 * (double)(rng() % 2) + 0.6 * u(rng), 0.6 * u(rng), 0.6 * u(rng), (int)(rng() % 10), (int)(rng() % 10), pair == 2 ? 1 : 0, pair == 0 ? 1 : 2, c, s);
      const double yv = 6.0 * u(rng), cv = std::cos(yv), sv = std::sin(yv);
      r.Tv[0] = cv, r.Tv[1] = -sv, r.Tv[3] = sv, r.Tv[4] = cv;
      r.Tv[9] = 20.0 * u(rng) - 10.0, r.Tv[10] = 20.0 * u(rng) - 10.0, r.Tv[11] = u(rng);
      r.Tu[9] = 20.0 * u(rng) - 10.0, r.Tu[10] = 20.0 * u(rng) - 10.0;
      // Z so that X = Tu Zn Tv^-1 is the claim: Zn = Tu^-1 claim Tv (formed here in any arithmetic: it is the input)
      const M4 claim = of_pose(r.Z), zn = mul(mul(inv(of_pose(r.Tu)), claim), of_pose(r.Tv));
      r.flip = (int)(rng() % 2);
      const M4 z = r.flip ? inv(zn) : zn;
      for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) r.Z[3 * a + b] = z.m[a][b];
        r.Z[9 + a] = z.m[a][3];
      }
      t.push_back(r);
    }
    const lins_team_pcm_params prm = params(1.0, kCos5, 0.01, 3);
    lins_team_pcm_result got;
    CHECK(run(t, prm, &got) == LINS_OK);
    // the restatement: X by explicit 4 x 4 products, the adjacency matrix, then everything read from it
    std::vector<M4> X(L);
    for (int l = 0; l < L; ++l) {
      const M4 z = of_pose(t[l].Z);
      X[l] = mul(mul(of_pose(t[l].Tu), t[l].flip ? inv(z) : z), inv(of_pose(t[l].Tv)));
    }
    const double trace_min = 1.0 + 2.0 * prm.min_cos_rotation;
    std::vector<char> adj((size_t)L * L, 0);
    for (int a = 0; a < L; ++a)
      for (int b = 0; b < L; ++b) {
        const Tag &ta = t[a].tag, &tb = t[b].tag;
        if (a == b || ta.u != tb.u || ta.v != tb.v || (ta.iu == tb.iu && ta.iv == tb.iv)) continue;
        double tr = 0.0;
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) tr = tr + X[a].m[i][j] * X[b].m[i][j];
        bool ok = tr >= trace_min;
        const double bar = prm.max_translation + prm.translation_per_frame * (double)(std::abs(ta.iu - tb.iu) + std::abs(ta.iv - tb.iv));
        for (const double* p : {t[a].Tv + 9, t[b].Tv + 9}) {
          double d[3];
          for (int i = 0; i < 3; ++i) {
            const double* A = X[a].m[i];
            const double* B = X[b].m[i];
            d[i] = (((A[0] * p[0] + A[1] * p[1]) + A[2] * p[2]) + A[3]) - (((B[0] * p[0] + B[1] * p[1]) + B[2] * p[2]) + B[3]);
          }
          ok = ok && (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= bar * bar;
        }
        adj[(size_t)a * L + b] = ok;
      }
    for (int a = 0; a < L; ++a)
      for (int b = 0; b < L; ++b) CHECK(adj[(size_t)a * L + b] == adj[(size_t)b * L + a]);
    std::vector<std::vector<int>> best(L);
    long long nodes_max = 0;
    for (int s = 0; s < L; ++s) {
      Search q{&adj, L, 0, prm.max_nodes, {s}, {s}, false};
      std::vector<int> P0;
      for (int w = s + 1; w < L; ++w)
        if (adj[(size_t)s * L + w]) P0.push_back(w);
      q.visit(P0);
      CHECK(!q.exhausted);
      best[s] = q.best, nodes_max = std::max(nodes_max, q.nodes);
    }
    std::vector<char> want(kMaxFactors, 0);
    int n_kept = 0, n_pairs = 0, n_pairs_kept = 0;
    std::vector<int> sizes;
    for (int u0 = 0; u0 < 2; ++u0)
      for (int v0 = u0 + 1; v0 < 3; ++v0) {
        int w = -1;
        for (int s = 0; s < L; ++s)
          if (t[s].tag.u == u0 && t[s].tag.v == v0 && (w < 0 || best[s].size() > best[w].size())) w = s;
        if (w < 0) continue;
        ++n_pairs;
        sizes.push_back((int)best[w].size());
        if ((int)best[w].size() < prm.min_support) continue;
        ++n_pairs_kept, n_kept += (int)best[w].size();
        for (int f : best[w]) want[f] = 1;
        cliques_of_three += 1;
      }
    CHECK(is(got, L, n_kept, n_pairs, n_pairs_kept, 1) && got.nodes_max == (uint32_t)nodes_max);
    for (int f = 0; f < kMaxFactors; ++f) CHECK(kept(got, f) == (bool)want[f]);
    // the table backwards: the cliques' sizes do not know the order (which of several largest ones is kept does)
    std::vector<Rec> back(t.rbegin(), t.rend());
    lins_team_pcm_result rev;
    CHECK(run(back, prm, &rev) == LINS_OK);
    CHECK(is(rev, L, n_kept, n_pairs, n_pairs_kept, 1));
    // a seeded shuffle, its kept mask mapped back through the permutation: per member pair a clique of the first table's
    // adjacency matrix, of the size kept there — the same factors wherever that pair's largest clique is the only one
    std::vector<int> perm(L);
    for (int i = 0; i < L; ++i) perm[i] = i;
    for (int i = L - 1; i > 0; --i) std::swap(perm[i], perm[rng() % (i + 1)]);
    std::vector<Rec> mixed(L);
    for (int i = 0; i < L; ++i) mixed[i] = t[perm[i]];
    lins_team_pcm_result mix;
    CHECK(run(mixed, prm, &mix) == LINS_OK);
    CHECK(is(mix, L, n_kept, n_pairs, n_pairs_kept, 1));
    std::vector<int> back_kept;
    for (int i = 0; i < L; ++i)
      if (kept(mix, i)) back_kept.push_back(perm[i]);
    bool same = true;
    for (int a : back_kept) {
      same = same && want[a];
      for (int b : back_kept)
        if (a != b && t[a].tag.u == t[b].tag.u && t[a].tag.v == t[b].tag.v) CHECK(adj[(size_t)a * L + b]);
    }
    same_under_shuffle += same && n_kept > 0;
    kept_tables += n_kept > 0;
  }
  CHECK(cliques_of_three > 60);  // (pairs whose clique reached min_support)
  CHECK(kept_tables > 40 && same_under_shuffle > 0 && same_under_shuffle <= kept_tables);  // (tables whose shuffled copy keeps the very same factors)
  std::printf("ok random\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "edges") return edges();
  if (mode == "cliques") return cliques();
  if (mode == "random") return random_tables();
  std::fprintf(stderr, "usage: team_pcm_check edges|cliques|random\n");
  return 2;
}
