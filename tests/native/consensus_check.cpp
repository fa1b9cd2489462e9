// consensus_check.cpp — csrc/host/rendezvous_consensus.h, the consensus rule's one scalar text, as a stand-alone program;
// built by tests/test_rendezvous_consensus_sanitized.py with -fsanitize=address,undefined.  Every table is a heap block of
// exactly its size (H = 0: a block of no bytes), every result a block of its own.
//   consensus_check edges    H = 0, 1 and 128, a pair on each bar and one nextafter beyond, the ties, the refusals
//   consensus_check random   seeded tables of every size 0 .. 128 against a restatement with the star written as an explicit
//                            adjacency matrix, under a permutation of the table
// stdout: "ok <mode>"; exit 1 with the reason on stderr.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "host/rendezvous_consensus.h"

using namespace lins_consensus;

#define CHECK(x)                                          \
  do {                                                    \
    if (!(x)) {                                           \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); \
      return 1;                                           \
    }                                                     \
  } while (0)

static lins_consensus_hyp shift(double x, double y, double z, int query, int rank = 0, double fitness = 0.1, int slot = 0, int adm = 1) {
  lins_consensus_hyp h;
  std::memset(&h, 0, sizeof h);
  h.X[0] = h.X[5] = h.X[10] = h.X[15] = 1.0;
  h.X[3] = x, h.X[7] = y, h.X[11] = z;
  h.fitness = fitness, h.query = query, h.rank = rank, h.target_slot = slot, h.admissible = adm;
  return h;
}

// the call as lins_host_rendezvous_consensus makes it, over a heap copy of exactly the table's size
static int run(const std::vector<lins_consensus_hyp>& t, double max_t, double min_cos, lins_consensus_result* out) {
  std::unique_ptr<lins_consensus_hyp[]> block(new lins_consensus_hyp[t.size()]);
  if (!t.empty()) std::memcpy(block.get(), t.data(), t.size() * sizeof(lins_consensus_hyp));
  std::unique_ptr<lins_consensus_result> res(new lins_consensus_result);
  lins_consensus_params prm;
  default_params(&prm);
  prm.max_translation = max_t, prm.min_cos_rotation = min_cos;
  if (!bars_ok(&prm)) return LINS_E_ARG;
  if (int rc = table_check(block.get(), (int)t.size())) return rc;
  evaluate(block.get(), (int)t.size(), bars_of(max_t, min_cos), res.get());
  *out = *res;
  return LINS_OK;
}

static bool member(const lins_consensus_result& r, int h) { return (r.members[h >> 5] >> (h & 31)) & 1u; }
static int n_members(const lins_consensus_result& r) {
  int n = 0;
  for (int h = 0; h < kMaxHyp; ++h) n += member(r, h);
  return n;
}

static int edges() {
  const double cos5 = 0.99619469809174555, one = std::nextafter(1.0, 2.0);
  lins_consensus_result r;
  CHECK(run({}, 1.0, cos5, &r) == LINS_OK && r.winner == -1 && r.support == 0 && r.n_admissible == 0 && n_members(r) == 0);
  CHECK(run({shift(1, 2, 3, 4, 2)}, 1.0, cos5, &r) == LINS_OK && r.winner == 0 && r.support == 1 && r.n_admissible == 1 && n_members(r) == 1);
  CHECK(run({shift(1, 2, 3, 4, 2, 0.1, 0, 0)}, 1.0, cos5, &r) == LINS_OK && r.winner == -1 && r.n_admissible == 0 && n_members(r) == 0);
  {  // a full table: ranks 0 agree, the rest scatter
    std::vector<lins_consensus_hyp> t;
    for (int q = 0; q < 16; ++q)
      for (int k = 0; k < 8; ++k) t.push_back(k ? shift(50.0 * k, 7.0 * q, 0, q, k, 0.1 + 0.001 * q + 0.01 * k) : shift(0.01 * q, 0, 0, q, 0, 0.1 + 0.001 * q));
    CHECK(run(t, 1.0, cos5, &r) == LINS_OK && r.winner == 0 && r.support == 16 && r.n_admissible == 128 && n_members(r) == 16 && member(r, 120));
    t[127] = t[5];  // ((query 0, rank 5) twice: there is no 129th (query, rank) to name)
    CHECK(run(t, 1.0, cos5, &r) == LINS_E_ARG);
  }
  {  // on the bars: integers, so nothing rounds
    lins_consensus_hyp a = shift(3, 0, 0, 0, 0, 0.1), b = shift(4, 0, 0, 1, 0, 0.2);
    a.p[0] = 1, a.p[1] = 2, a.p[2] = 3, b.p[0] = -2, b.p[2] = 5;
    CHECK(run({a, b}, 1.0, cos5, &r) == LINS_OK && r.winner == 0 && r.support == 2 && n_members(r) == 2);
    lins_consensus_hyp c = shift(0, 0, 0, 0, 0, 0.1), d = shift(one, 0, 0, 1, 0, 0.2);
    CHECK(run({c, d}, 1.0, cos5, &r) == LINS_OK && r.winner == 0 && r.support == 1 && n_members(r) == 1);
    d = shift(0, 0, 0, 1, 0, 0.2);
    CHECK(run({c, d}, 1.0, 1.0, &r) == LINS_OK && r.support == 2);
    CHECK(run({c, d}, 1.0, one, &r) == LINS_OK && r.support == 1);
    CHECK(run({c, d}, 0.0, 1.0, &r) == LINS_OK && r.support == 2);  // (a bar of zero admits an equal pair)
  }
  {  // ties: support and fitness equal -> the larger query, then the smaller rank; one query is one witness; slots do not mix
    CHECK(run({shift(0, 0, 0, 2, 0, 0.125), shift(0, 0, 0, 7, 0, 0.125), shift(0, 0, 0, 5, 0, 0.125)}, 1.0, cos5, &r) == LINS_OK && r.winner == 1 && r.support == 3);
    CHECK(run({shift(0, 0, 0, 1, 3, 0.125), shift(0, 0, 0, 6, 5, 0.125), shift(0, 0, 0, 6, 2, 0.125), shift(9, 9, 9, 6, 0, 0.125)}, 1.0, cos5, &r) == LINS_OK &&
          r.winner == 2 && r.support == 2 && member(r, 0) && member(r, 2) && !member(r, 1) && !member(r, 3));
    std::vector<lins_consensus_hyp> same;
    for (int k = 0; k < 8; ++k) same.push_back(shift(0, 0, 0, 3, k, 0.2 - 0.01 * k));
    CHECK(run(same, 1.0, cos5, &r) == LINS_OK && r.winner == 7 && r.support == 1 && n_members(r) == 1);
    CHECK(run({shift(0, 0, 0, 0, 0, 0.1, 0), shift(0, 0, 0, 1, 0, 0.2, 1), shift(0, 0, 0, 2, 0, 0.3, 0)}, 1.0, cos5, &r) == LINS_OK && r.winner == 0 &&
          r.support == 2 && !member(r, 1));
  }
  {  // the refusals; an inadmissible hypothesis is not read beyond its integers
    const double nan = std::nan(""), inf = INFINITY;
    lins_consensus_hyp a = shift(0, 0, 0, 0), b = shift(0, 0, 0, 1);
    CHECK(run({a, b}, -1.0, cos5, &r) == LINS_E_ARG && run({a, b}, inf, cos5, &r) == LINS_E_ARG && run({a, b}, nan, cos5, &r) == LINS_E_ARG &&
          run({a, b}, 1.0, nan, &r) == LINS_E_ARG);
    for (int which = 0; which < 7; ++which) {
      lins_consensus_hyp x = b;
      (which == 0 ? x.query = -1 : which == 1 ? x.query = 16 : which == 2 ? x.rank = -1 : which == 3 ? x.rank = 8 : which == 4 ? x.admissible = 2
       : which == 5 ? x.admissible = -1 : x.query = 0);
      CHECK(run({a, x}, 1.0, cos5, &r) == LINS_E_ARG);
    }
    for (int j = 0; j < kDoubles; ++j)
      for (double v : {nan, inf, -inf}) {
        lins_consensus_hyp x = b;
        ((double*)&x)[j] = v;
        CHECK(run({a, x}, 1.0, cos5, &r) == LINS_E_INPUT);
        x.admissible = 0;
        CHECK(run({a, x}, 1.0, cos5, &r) == LINS_OK && r.n_admissible == 1);
      }
    b.fitness = -1e-300;
    CHECK(run({a, b}, 1.0, cos5, &r) == LINS_E_INPUT);
  }
  std::printf("ok edges\n");
  return 0;
}

static int random_tables() {
  std::mt19937 rng(23);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  const double cos5 = 0.99619469809174555;
  long long witnessed = 0;
  for (int H = 0; H <= kMaxHyp; ++H) {
    std::vector<int> qr(kMaxHyp);
    for (int i = 0; i < kMaxHyp; ++i) qr[i] = i;
    for (int i = kMaxHyp - 1; i > 0; --i) std::swap(qr[i], qr[rng() % (i + 1)]);
    std::vector<lins_consensus_hyp> t;
    for (int i = 0; i < H; ++i) {
      // two clusters 30 m apart, a yaw of up to 4 degrees either way, 0.6 m of scatter
      const double yaw = (u(rng) - 0.5) * 0.14, c = std::cos(yaw), s = std::sin(yaw);
      lins_consensus_hyp h = shift(30.0 * (double)(rng() % 2) + 0.6 * u(rng), 0.6 * u(rng), 0.6 * u(rng), qr[i] / 8, qr[i] % 8, 0.3 * u(rng), (int)(rng() % 2),
                                   u(rng) < 0.85);
      h.X[0] = c, h.X[1] = -s, h.X[4] = s, h.X[5] = c;
      h.p[0] = 20.0 * u(rng) - 10.0, h.p[1] = 20.0 * u(rng) - 10.0, h.p[2] = u(rng);
      t.push_back(h);
    }
    lins_consensus_result got;
    CHECK(run(t, 1.0, cos5, &got) == LINS_OK);
    // the restatement: the adjacency matrix first, then everything read from it
    const Bars bars = bars_of(1.0, cos5);
    std::vector<char> adj((size_t)H * H, 0);
    for (int a = 0; a < H; ++a)
      for (int b = 0; b < H; ++b) {
        if (a == b || !t[a].admissible || !t[b].admissible || t[a].target_slot != t[b].target_slot || t[a].query == t[b].query) continue;
        double tr = 0.0;
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) tr = tr + t[a].X[4 * i + j] * t[b].X[4 * i + j];
        bool ok = tr >= bars.trace_min;
        for (const double* p : {t[a].p, t[b].p}) {
          double d2 = 0.0, d[3];
          for (int i = 0; i < 3; ++i) {
            const double* A = t[a].X + 4 * i;
            const double* B = t[b].X + 4 * i;
            d[i] = (((A[0] * p[0] + A[1] * p[1]) + A[2] * p[2]) + A[3]) - (((B[0] * p[0] + B[1] * p[1]) + B[2] * p[2]) + B[3]);
          }
          d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
          ok = ok && d2 <= bars.t2_max;
        }
        adj[(size_t)a * H + b] = ok;
      }
    for (int a = 0; a < H; ++a)
      for (int b = 0; b < H; ++b) CHECK(adj[(size_t)a * H + b] == adj[(size_t)b * H + a]);
    int want = -1, want_support = 0, n_adm = 0;
    std::vector<int> support(H, 0);
    for (int a = 0; a < H; ++a) {
      if (!t[a].admissible) continue;
      ++n_adm;
      bool seen[kMaxWindow] = {false};
      seen[t[a].query] = true;
      for (int b = 0; b < H; ++b)
        if (adj[(size_t)a * H + b]) seen[t[b].query] = true;
      for (bool s : seen) support[a] += s;
    }
    for (int a = 0; a < H; ++a) {
      if (!t[a].admissible) continue;
      bool first = want < 0;
      if (!first) {
        const lins_consensus_hyp &x = t[a], &y = t[want];
        first = support[a] != support[want] ? support[a] > support[want]
                : x.fitness != y.fitness     ? x.fitness < y.fitness
                : x.query != y.query         ? x.query > y.query
                                             : x.rank < y.rank;
      }
      if (first) want = a, want_support = support[a];
    }
    CHECK(got.winner == want && got.support == want_support && got.n_admissible == n_adm);
    for (int b = 0; b < kMaxHyp; ++b) CHECK(member(got, b) == (want >= 0 && b < H && (b == want || adj[(size_t)want * H + b])));
    witnessed += want_support > 1;
    // the table backwards: the same answer up to the index mapping
    std::vector<lins_consensus_hyp> back(t.rbegin(), t.rend());
    lins_consensus_result rev;
    CHECK(run(back, 1.0, cos5, &rev) == LINS_OK);
    CHECK(rev.support == got.support && rev.n_admissible == got.n_admissible && rev.winner == (got.winner < 0 ? -1 : H - 1 - got.winner));
    for (int b = 0; b < H; ++b) CHECK(member(rev, H - 1 - b) == member(got, b));
  }
  CHECK(witnessed > 100);  // (tables whose winner has a second witness)
  std::printf("ok random\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "edges") return edges();
  if (mode == "random") return random_tables();
  std::fprintf(stderr, "usage: consensus_check edges|random\n");
  return 2;
}
