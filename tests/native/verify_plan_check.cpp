// verify_plan_check.cpp — csrc/host/verify_plan.h, the one layout of the steps' assemble-and-align stage, as a stand-alone
// program; built by tests/test_verify_plan_sanitized.py with -fsanitize=address,undefined.  Every array handed to the header
// is a heap block of exactly its size (none: a block of no elements).  The plan is held against a restatement written
// here — a map from an entry's source frame to its spec, windows counted out by hand — that calls nothing of the header.
//   verify_plan_check shapes   the four layouts of the steps: 2i / 2i + 1; first, first + 1 + j for 1 .. LINS_PLACE_MAX_K
//                              targets; the window's W x K up to LINS_RENDEZVOUS_MAX_HYP with queries without a rank and
//                              entries without a hypothesis; window ids against lins_loop::window at both clips and H = 0
//   verify_plan_check status   entry_status and icp_summary with a status in the first, a middle and the last position
//   verify_plan_check random   seeded tables against the restatement
// stdout: "ok <mode>"; exit 1 with the reason on stderr.
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "host/verify_plan.h"

using namespace lins_verify;

#define CHECK(x)                                          \
  do {                                                    \
    if (!(x)) {                                           \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); \
      return 1;                                           \
    }                                                     \
  } while (0)

template <class T>
static std::unique_ptr<T[]> block(const std::vector<T>& v) {
  std::unique_ptr<T[]> b(new T[v.size()]);
  for (size_t i = 0; i < v.size(); ++i) b[i] = v[i];
  return b;
}

struct Table {  // the input: entry e has slot slots[e] and the hypotheses hyps[hyp0[e] .. hyp0[e + 1])
  std::vector<int32_t> slots, hyp0{0};
  std::vector<Hyp> hyps;
  void entry(int slot) { slots.push_back(slot), hyp0.push_back(hyp0.back()); }
  void hyp(int source, int tslot, int tid, int tlatest) { hyps.push_back(Hyp{source, tslot, tid, tlatest}), hyp0.back() += 1; }
};

struct Want {  // one spec of the restatement
  int kind, slot, flags;
  float leaf;
  std::vector<int32_t> ids;
};

struct Plan {  // the header's answer, copied out of its exact blocks
  std::vector<Want> specs;
  std::vector<int32_t> src, tgt, spec0;
};

// the two calls as loop_verify.h makes them, over heap blocks of exactly the sizes the first call names
static int plan_of(const Table& t, int H, float leaf, Plan* out) {
  const int n = (int)t.slots.size(), nh = (int)t.hyps.size();
  auto slots = block(t.slots);
  auto hyp0 = block(t.hyp0);
  auto hyps = block(t.hyps);
  const Sizes z = layout(n, slots.get(), hyp0.get(), hyps.get(), H, leaf, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  CHECK(z.specs >= 0 && z.ids >= 0);
  std::unique_ptr<lins_submap_spec[]> specs(new lins_submap_spec[z.specs]);
  std::unique_ptr<int32_t[]> kind(new int32_t[z.specs]), ids(new int32_t[z.ids]), src(new int32_t[nh]), tgt(new int32_t[nh]), spec0(new int32_t[n + 1]);
  const Sizes again = layout(n, slots.get(), hyp0.get(), hyps.get(), H, leaf, specs.get(), kind.get(), ids.get(), src.get(), tgt.get(), spec0.get());
  CHECK(again.specs == z.specs && again.ids == z.ids);
  out->specs.clear();
  long long at = 0;
  for (long long s = 0; s < z.specs; ++s) {
    const lins_submap_spec& p = specs[s];
    CHECK(p.ids == ids.get() + at && p.n_ids >= 0 && at + p.n_ids <= z.ids);  // the id lists lie back to back, in spec order
    CHECK(p.clouds == (LINS_SUBMAP_CORNER | LINS_SUBMAP_SURF) && p.reserved == 0);
    out->specs.push_back(Want{kind[s], p.slot, p.flags, p.leaf, std::vector<int32_t>(p.ids, p.ids + p.n_ids)});
    at += p.n_ids;
  }
  CHECK(at == z.ids);
  out->src.assign(src.get(), src.get() + nh), out->tgt.assign(tgt.get(), tgt.get() + nh), out->spec0.assign(spec0.get(), spec0.get() + n + 1);
  return 0;
}

// The restatement.  Per entry a map: source frame -> its spec.
static Plan restate(const Table& t, int H, float leaf) {
  Plan p;
  for (size_t e = 0; e < t.slots.size(); ++e) {
    p.spec0.push_back((int32_t)p.specs.size());
    std::map<int, int> spec_of_source;
    for (int x = t.hyp0[e]; x < t.hyp0[e + 1]; ++x) {
      const Hyp& h = t.hyps[x];
      if (!spec_of_source.count(h.source_id)) {
        spec_of_source[h.source_id] = (int)p.specs.size();
        p.specs.push_back(Want{0, t.slots[e], 1, 0.f, {h.source_id}});
      }
      p.src.push_back(spec_of_source[h.source_id]);
      Want w{1, h.target_slot, 0, leaf, {}};
      if (h.target_latest >= 0 && h.target_id >= 0 && h.target_id <= h.target_latest && H >= 0)
        for (long long id = (long long)h.target_id - H; id <= (long long)h.target_id + H; ++id)
          if (id >= 0 && id <= h.target_latest) w.ids.push_back((int32_t)id);
      p.tgt.push_back((int32_t)p.specs.size());
      p.specs.push_back(w);
    }
  }
  p.spec0.push_back((int32_t)p.specs.size());
  return p;
}

static bool same(const Plan& a, const Plan& b) {
  if (a.src != b.src || a.tgt != b.tgt || a.spec0 != b.spec0 || a.specs.size() != b.specs.size()) return false;
  for (size_t s = 0; s < a.specs.size(); ++s) {
    const Want &x = a.specs[s], &y = b.specs[s];
    if (x.kind != y.kind || x.slot != y.slot || x.flags != y.flags || std::memcmp(&x.leaf, &y.leaf, sizeof x.leaf) || x.ids != y.ids) return false;
  }
  return true;
}

static int agrees(const Table& t, int H, float leaf, Plan* got) {
  if (plan_of(t, H, leaf, got)) return 1;
  CHECK(same(*got, restate(t, H, leaf)));
  return 0;
}

static int shapes() {
  Plan p;
  {  // (a) lins_loop_step: one hypothesis an entry, the latest frame against a window of its own slot
    Table t;
    for (int i = 0; i < 7; ++i) t.entry(10 + i), t.hyp(20 + i, 10 + i, i, 20 + i);
    CHECK(!agrees(t, 4, 0.4f, &p));
    for (int i = 0; i < 7; ++i) CHECK(p.src[i] == 2 * i && p.tgt[i] == 2 * i + 1 && p.spec0[i] == 2 * i);
    CHECK(p.spec0[7] == 14 && p.specs[12].kind == kSource && p.specs[13].kind == kTarget && p.specs[13].slot == 16);
  }
  {  // (b) the two top-K steps: one source, 1 .. LINS_PLACE_MAX_K targets
    Table t;
    std::vector<int> first{0};
    for (int k = 1; k <= LINS_PLACE_MAX_K; ++k) {
      t.entry(k);
      for (int j = 0; j < k; ++j) t.hyp(11, (k + j) % 5, 3 + j, 11);
      first.push_back(first.back() + 1 + k);
    }
    CHECK(!agrees(t, 2, 0.25f, &p));
    for (int k = 1, x = 0; k <= LINS_PLACE_MAX_K; ++k)
      for (int j = 0; j < k; ++j, ++x) CHECK(p.src[x] == first[k - 1] && p.tgt[x] == first[k - 1] + 1 + j && p.spec0[k - 1] == first[k - 1]);
    CHECK((int)p.specs.size() == first.back());
  }
  for (int W : {1, 5, LINS_RENDEZVOUS_MAX_WINDOW})  // (c) the window: a source in front of a query's rank 0, none for a query without ranks
    for (int K : {1, 3, LINS_PLACE_MAX_K}) {
      Table t;
      std::vector<int> want_src, want_tgt;
      int s = 0;
      for (int e = 0; e < 5; ++e) {
        t.entry(e);
        if (e == 1 || e == 4) continue;  // entries without a hypothesis
        for (int q = 0; q < W; ++q) {
          const int ranks = (q + e) % 3 == 1 ? 0 : 1 + (q * 5 + e) % K;  // (every third query has none; W = 16, K = 8 reaches 8 ranks)
          const int source = s;  // (taken only when the query has a rank)
          for (int r = 0; r < ranks; ++r) {
            t.hyp(30 - 2 * q, 7 + (r % 3), 2 * r + q, 31);
            want_src.push_back(source), want_tgt.push_back(source + 1 + r);
          }
          s += ranks ? 1 + ranks : 0;
        }
        CHECK(t.hyp0.back() - t.hyp0[t.hyp0.size() - 2] <= LINS_RENDEZVOUS_MAX_HYP);
      }
      CHECK(!agrees(t, 3, 0.4f, &p));
      CHECK(p.src == want_src && p.tgt == want_tgt && p.spec0[1] == p.spec0[2] && p.spec0[4] == p.spec0[5] && p.spec0[5] == s);
    }
  {  // a full table: W * K = LINS_RENDEZVOUS_MAX_HYP
    Table t;
    t.entry(0);
    for (int q = 0; q < LINS_RENDEZVOUS_MAX_WINDOW; ++q)
      for (int r = 0; r < LINS_PLACE_MAX_K; ++r) t.hyp(40 - q, 1 + r % 2, r, 9);
    CHECK(!agrees(t, 25, 0.4f, &p));
    CHECK((int)p.src.size() == LINS_RENDEZVOUS_MAX_HYP && (int)p.specs.size() == LINS_RENDEZVOUS_MAX_HYP + LINS_RENDEZVOUS_MAX_WINDOW);
    CHECK(p.src[127] == 15 * 9 && p.tgt[127] == 15 * 9 + 8);
  }
  {  // (d) a target's ids are lins_loop::window's: clipped below, clipped above, H = 0, and nothing to give
    const int cases[][3] = {{11, 2, 4}, {11, 9, 4}, {11, 5, 0}, {11, 0, 0}, {11, 11, 25}, {0, 0, 3}, {11, 12, 4}, {11, -1, 4}, {-1, 0, 4}};
    for (const auto& c : cases) {
      Table t;
      t.entry(3), t.hyp(11, 6, c[1], c[0]);
      CHECK(!agrees(t, c[2], 0.4f, &p));
      const int n = lins_loop::window_size(c[0], c[1], c[2]);
      std::unique_ptr<int32_t[]> ids(new int32_t[n]);
      CHECK(lins_loop::window(c[0], c[1], c[2], ids.get()) == n);
      CHECK(p.specs[1].ids == std::vector<int32_t>(ids.get(), ids.get() + n) && p.specs[1].slot == 6 && p.specs[1].flags == 0);
      CHECK(p.specs[0].ids == std::vector<int32_t>{11} && p.specs[0].slot == 3 && p.specs[0].flags == LINS_SUBMAP_DROP_NEGATIVE && p.specs[0].leaf == 0.f);
    }
    Table t;
    t.entry(0), t.hyp(11, 0, 2, 11), t.hyp(11, 0, 9, 11), t.hyp(11, 0, 5, 11);
    CHECK(!agrees(t, 4, 0.4f, &p));
    CHECK((p.specs[1].ids == std::vector<int32_t>{0, 1, 2, 3, 4, 5, 6}) && (p.specs[2].ids == std::vector<int32_t>{5, 6, 7, 8, 9, 10, 11}));
    CHECK(!agrees(t, 0, 0.4f, &p));
    CHECK(p.specs[1].ids == std::vector<int32_t>{2} && p.specs[3].ids == std::vector<int32_t>{5});
  }
  {  // no entry at all
    Table t;
    CHECK(!agrees(t, 4, 0.4f, &p));
    CHECK(p.specs.empty() && p.spec0 == std::vector<int32_t>{0});
  }
  return 0;
}

static int status() {
  const int codes[] = {LINS_E_INPUT, LINS_E_CAPACITY};
  for (int n : {1, 2, 5, 9})
    for (int at = -1; at < n; ++at)        // where the first status stands (-1: nowhere)
      for (int second = at; second < n; ++second) {  // ... and one behind it, with another code
        std::unique_ptr<lins_submap_info[]> infos(new lins_submap_info[n]);
        std::unique_ptr<lins_loop_icp_result[]> icp(new lins_loop_icp_result[n]);
        std::unique_ptr<int32_t[]> conv(new int32_t[n]);
        std::unique_ptr<double[]> fit(new double[n]);
        std::memset(infos.get(), 0, n * sizeof(lins_submap_info)), std::memset(icp.get(), 0, n * sizeof(lins_loop_icp_result));
        for (int j = 0; j < n; ++j) icp[j].converged = 1, icp[j].fitness = 0.1 * (j + 1);
        int bad = 0;
        if (at >= 0) infos[at].status = icp[at].status = codes[0], bad = 1;
        if (at >= 0 && second > at) infos[second].status = icp[second].status = codes[1], bad = 2;
        CHECK(entry_status(infos.get(), 0, n) == (at < 0 ? 0 : codes[0]));
        CHECK(entry_status(infos.get(), 0, 0) == 0 && entry_status(infos.get(), n, n) == 0);
        if (at >= 0) CHECK(entry_status(infos.get(), at + 1, n) == (second > at ? codes[1] : 0) && entry_status(infos.get(), 0, at) == 0);
        const IcpSummary s = icp_summary(icp.get(), n, conv.get(), fit.get());
        CHECK(s.status == (at < 0 ? 0 : codes[0]) && s.ran == n - bad);
        for (int j = 0; j < n; ++j) CHECK(conv[j] == (icp[j].status ? 0 : 1) && fit[j] == 0.1 * (j + 1));
        const IcpSummary bare = icp_summary(icp.get(), n, nullptr, nullptr);
        CHECK(bare.status == s.status && bare.ran == s.ran);
        // what lins_loop::choose makes of it: the smallest fitness among those that ran
        int first_ran = 0;
        while (first_ran < n && icp[first_ran].status) ++first_ran;
        CHECK(lins_loop::choose(n, conv.get(), fit.get(), 0.95f) == (first_ran < n ? first_ran : -1));
      }
  const IcpSummary none = icp_summary(nullptr, 0, nullptr, nullptr);
  CHECK(none.status == 0 && none.ran == 0);
  // the parameter ranges of the stage
  lins_loop_step_params p;
  std::memset(&p, 0, sizeof p);
  p.max_fitness = 0.3f, p.history_leaf = 0.4f, p.search_num = 25, p.min_gap_s = 30.0, p.icp.max_iterations = 100, p.icp.max_corr_dist = 100.f;
  CHECK(params_ok(&p) && !params_ok(nullptr));
  lins_loop_step_params q = p;
  q.search_num = -1;
  CHECK(!params_ok(&q));
  q = p, q.history_leaf = -0.f;
  CHECK(params_ok(&q));
  q = p, q.history_leaf = -0.1f;
  CHECK(!params_ok(&q));
  q = p, q.history_leaf = INFINITY;
  CHECK(!params_ok(&q));
  q = p, q.max_fitness = NAN;
  CHECK(!params_ok(&q));
  q = p, q.max_fitness = INFINITY, q.min_gap_s = -INFINITY, q.search_num = 0, q.icp.min_correspondences = 0;
  CHECK(params_ok(&q));
  q = p, q.min_gap_s = NAN;
  CHECK(!params_ok(&q));
  q = p, q.icp.max_iterations = 0;
  CHECK(!params_ok(&q));
  q = p, q.icp.min_correspondences = -1;
  CHECK(!params_ok(&q));
  q = p, q.icp.max_corr_dist = NAN;
  CHECK(!params_ok(&q));
  return 0;
}

static int random_tables() {
  std::mt19937 rng(20240611);
  auto below = [&](int n) { return (int)(rng() % (unsigned)n); };
  for (int round = 0; round < 400; ++round) {
    Table t;
    const int n = below(7), H = below(4) == 0 ? 0 : below(30);
    for (int e = 0; e < n; ++e) {
      t.entry(below(64));
      const int nh = below(5) == 0 ? 0 : below(LINS_RENDEZVOUS_MAX_HYP + 1), sources = 1 + below(LINS_RENDEZVOUS_MAX_WINDOW);
      for (int x = 0; x < nh; ++x) {
        const int latest = below(6) == 0 ? below(3) : below(60);
        t.hyp(100 + below(sources), below(64), below(latest + 2) - (below(20) == 0), latest - (below(30) == 0 ? latest + 1 : 0));  // (sources in any order, ids off either end)
      }
    }
    Plan p;
    CHECK(!agrees(t, H, 0.05f * below(20), &p));
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  int rc = 1;
  if (mode == "shapes") rc = shapes();
  else if (mode == "status") rc = status();
  else if (mode == "random") rc = random_tables();
  else std::fprintf(stderr, "usage: verify_plan_check shapes|status|random\n");
  if (rc == 0) std::printf("ok %s\n", mode.c_str());
  return rc;
}
