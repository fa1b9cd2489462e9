// team_pcm.h — pairwise consistency maximisation over team factors: per pair of members the largest set of factors that
// agree with each other two by two, the ONE scalar text of both libraries (lins_host_team_factors_consistent: the
// definition; team_pcm_kernels.hip calls the same functions on its LDS copy of the group, so the device holds these bits
// by construction).  The contract (include/lins_host.h, DESIGN.md §5.3 "Pairwise-consistent team factors"):
//   record      of a factor: u < v its two members, iu, iv its frames on them; Zn = Z where slot_b is u, inverse(Z)
//               otherwise (Zn measures Tu^-1 Tv); X = compose(compose(Tu, Zn), inverse(Tv)) — v's map frame to u's, as this
//               factor claims it — and p = the translation of Tv.  X is MOVED into rows 0 .. 2 of a 4 x 4 row-major matrix,
//               the layout trace_of and apart2_at of rendezvous_consensus.h read (they read nothing of row 3): 12 doubles,
//               then p: 15.
//   consistent  l != m: the same (u, v); not the same (iu, iv); trace_of(X_l, X_m) >= 1 + 2 min_cos;
//               apart2_at(X_l, X_m, p) <= t^2 at p_l AND at p_m, t = max_translation + translation_per_frame *
//               (double)(|iu_l - iu_m| + |iv_l - iv_m|).  Products commute, a difference changes only its sign when l and m
//               change places and is squared, the two positions are both asked, and |a - b| and a sum of two integers do
//               not know which came first: the relation is symmetric to the bit.
//   search      per vertex s the largest clique whose smallest member is s (subproblem): depth first over bit masks, in
//               ascending index order, with its own node counter against max_nodes and no knowledge of any other
//               subproblem; written iteratively on a caller's stack of kLevels words (a local array on the host, LDS on the
//               device).  A subproblem that runs out of nodes keeps its best so far.
//   winner      per member pair the subproblem of largest size, then smallest s; kept iff its size >= min_support
// f64, products and sums only, in the order written, no libm; the files that include this are compiled with
// -ffp-contract=off.  The masks are integers: nothing there depends on who computes it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/lins_host.h"
#include "../lins_math.h"
#include "../pose_graph_math.h"
#include "rendezvous_consensus.h"

namespace lins_pcm {

constexpr int kMaxFactors = LINS_TEAM_PCM_MAX_FACTORS;
constexpr int kLevels = 64;  // a clique of 64 opens nodes at depths 0 .. 63; a node at depth 63 has no candidate left to stack
constexpr int kXp = 15;      // rows 0 .. 2 of X | p
constexpr int kP = 12;
static_assert(kMaxFactors == 64, "one 64-bit adjacency row a factor, one lane a factor");
static_assert(sizeof(lins_team_pcm_result) == 32, "two 16-byte stores");

struct Tag {
  int32_t u, v, iu, iv;
};
// a factor as it goes to the device: 36 doubles and six integers
struct Rec {
  double Z[12], Tu[12], Tv[12];
  Tag tag;
  int32_t flip, pad;  // flip: slot_b is the LARGER member, Zn = inverse(Z)
};
static_assert(sizeof(Rec) == 312 && offsetof(Rec, tag) == 288, "a record is 39 8-byte words");
constexpr int kRecWords = (int)(sizeof(Rec) / 8);

struct Bars {
  double trace_min;        // 1 + 2 min_cos_rotation
  double max_translation;  // t at a frame distance of 0
  double per_frame;
};
LINS_HD Bars bars_of(const lins_team_pcm_params& p) {
  return Bars{lins_consensus::bars_of(p.max_translation, p.min_cos_rotation).trace_min, p.max_translation, p.translation_per_frame};
}

// xp[15] of a factor
LINS_HD void form(const double* Z, int flip, const double* Tu, const double* Tv, double* xp) {
  double Zn[12], A[12], Ti[12], X[12];
  if (flip) {
    lins_pg::inverse(Z, Zn);
  } else {
    lins_pg::pose_copy(Z, Zn);
  }
  lins_pg::compose(Tu, Zn, A);
  lins_pg::inverse(Tv, Ti);
  lins_pg::compose(A, Ti, X);
  PG_UNROLL
  for (int i = 0; i < 3; ++i) {
    xp[4 * i] = X[3 * i], xp[4 * i + 1] = X[3 * i + 1], xp[4 * i + 2] = X[3 * i + 2], xp[4 * i + 3] = X[9 + i];
    xp[kP + i] = Tv[9 + i];
  }
}

LINS_HD long long absdiff(int32_t a, int32_t b) { return a > b ? (long long)a - b : (long long)b - a; }

// a, b: the 15 doubles of two DIFFERENT factors (the caller never asks a factor about itself)
LINS_HD bool consistent(const double* a, const Tag& ta, const double* b, const Tag& tb, const Bars& bars) {
  if (ta.u != tb.u || ta.v != tb.v) return false;
  if (ta.iu == tb.iu && ta.iv == tb.iv) return false;  // one frame pair twice: no witness for each other
  if (!(lins_consensus::trace_of(a, b) >= bars.trace_min)) return false;
  const double t = bars.max_translation + bars.per_frame * (double)(absdiff(ta.iu, tb.iu) + absdiff(ta.iv, tb.iv));
  const double t2 = t * t;
  return lins_consensus::apart2_at(a, b, a + kP) <= t2 && lins_consensus::apart2_at(a, b, b + kP) <= t2;
}

LINS_HD int popcount64(uint64_t m) { return __builtin_popcountll(m); }
LINS_HD int lowest64(uint64_t m) { return __builtin_ctzll(m); }  // m != 0

// what a subproblem leaves
struct Sub {
  uint64_t best;   // its clique, s included
  int32_t size;
  uint32_t nodes;  // the counter as it stands: max_nodes + 1 where it ran out
  int32_t exhausted;
};

// Subproblem s over the rows adj[0 .. n): the best clique whose smallest member is s.  stack[d * stride] is level d of
// kLevels: the candidates still open at depth d WITH the vertex chosen there, which is their lowest bit — it leaves the
// word when the search comes back from it.
//   visit(R, |R|, P):  nodes += 1;  nodes > max_nodes: exhausted, stop;  P empty: best = R where |R| > |best|, return;
//                      while P not empty:  |R| + popcount(P) <= |best|: return;  w = lowest of P;  P -= w;
//                                          visit(R + w, |R| + 1, P & N(w))
LINS_HD Sub subproblem(int s, const uint64_t* adj, uint32_t max_nodes, uint64_t* stack, int stride) {
  const uint64_t self = (uint64_t)1 << s;
  Sub r = Sub{self, 1, 0u, 0};
  uint64_t R = self, P = adj[s] & ~(self | (self - 1));  // N(s) among the vertices behind s
  int nR = 1, depth = 0;
  bool opens = true;  // a node opens with (R, nR, P) at `depth`; otherwise the node at `depth` goes on with its candidates
  for (;;) {
    if (opens) {
      r.nodes += 1u;
      if (r.nodes > max_nodes) {
        r.exhausted = 1;
        break;
      }
      if (P == 0 && nR > r.size) r.best = R, r.size = nR;
      stack[depth * stride] = P;  // (an empty word for a leaf: it returns below)
      opens = false;
    }
    P = stack[depth * stride];
    if (P == 0 || nR + popcount64(P) <= r.size) {  // the node returns: its parent's chosen vertex leaves P and R
      if (depth == 0) break;
      depth -= 1;
      const uint64_t Pd = stack[depth * stride], wb = Pd & (~Pd + 1);
      stack[depth * stride] = Pd ^ wb;
      R ^= wb, nR -= 1;
    } else {
      const uint64_t wb = P & (~P + 1);
      R |= wb, nR += 1, depth += 1;
      P = (P ^ wb) & adj[lowest64(wb)];
      opens = true;
    }
  }
  return r;
}

// the winner of l's pair among the n subproblems: largest size, then smallest s; key[a] == key[b] iff a and b are factors
// of one member pair
LINS_HD int pair_winner(int l, int n, const int32_t* key, const int32_t* size) {
  int w = -1;
  for (int s = 0; s < n; ++s)
    if (key[s] == key[l] && (w < 0 || size[s] > size[w])) w = s;
  return w;
}
LINS_HD bool pair_head(int l, const int32_t* key) {
  for (int s = 0; s < l; ++s)
    if (key[s] == key[l]) return false;
  return true;
}

// ---- the host side: the checks and the definition itself ----
inline void default_params(lins_team_pcm_params* p) { *p = lins_team_pcm_params{1.0, 0.99619469809174555, 0.0, 3, 65536}; }

inline bool params_ok(const lins_team_pcm_params* p) {
  using lins_consensus::finite64;
  return p && finite64(p->max_translation) && p->max_translation >= 0.0 && p->min_cos_rotation == p->min_cos_rotation &&
         finite64(p->translation_per_frame) && p->translation_per_frame >= 0.0 && p->min_support >= 1 && p->max_nodes >= 1;
}

inline bool finite12(const double* T) {
  for (int i = 0; i < 12; ++i)
    if (!lins_consensus::finite64(T[i])) return false;
  return true;
}

// a factor whose slots are member indices, with the two frames' poses -> its record (the factor has passed the checks)
inline Rec record_of(const lins_team_factor& f, const double* Tb, const double* Ta) {
  Rec r;
  const bool flip = f.slot_b > f.slot_a;
  for (int i = 0; i < 12; ++i) r.Z[i] = f.Z[i], r.Tu[i] = (flip ? Ta : Tb)[i], r.Tv[i] = (flip ? Tb : Ta)[i];
  r.tag = flip ? Tag{f.slot_a, f.slot_b, f.id_a, f.id_b} : Tag{f.slot_b, f.slot_a, f.id_b, f.id_a};
  r.flip = flip ? 1 : 0, r.pad = 0;
  return r;
}

// key[l]: the first factor of l's member pair
inline void pair_keys(const Rec* rec, int n, int32_t* key) {
  for (int l = 0; l < n; ++l) {
    key[l] = l;
    for (int s = 0; s < l; ++s)
      if (rec[s].tag.u == rec[l].tag.u && rec[s].tag.v == rec[l].tag.v) {
        key[l] = s;
        break;
      }
  }
}

// LINS_OK or LINS_E_ARG for a graph handed to the search alone: rows within n, no vertex its own neighbour, symmetric, no
// edge between two pairs
inline int graph_check(int n, const uint64_t* adj, const int32_t* key) {
  for (int a = 0; a < n; ++a) {
    if ((n < 64 && (adj[a] >> n) != 0) || ((adj[a] >> a) & 1u)) return LINS_E_ARG;
    for (int b = 0; b < n; ++b)
      if ((adj[a] >> b) & 1u)
        if (!((adj[b] >> a) & 1u) || key[a] != key[b]) return LINS_E_ARG;
  }
  return LINS_OK;
}

// the searches and the winners over checked rows; stack: kLevels words
inline void evaluate_graph(int n, const uint64_t* adj, const int32_t* key, const lins_team_pcm_params& prm, uint64_t* stack,
                           lins_team_pcm_result* out) {
  uint64_t best[kMaxFactors];
  int32_t size[kMaxFactors];
  lins_team_pcm_result r = lins_team_pcm_result{n, 0, 0, 0, 1, 0u, {0u, 0u}};
  for (int s = 0; s < n; ++s) {
    const Sub sub = subproblem(s, adj, (uint32_t)prm.max_nodes, stack, 1);
    best[s] = sub.best, size[s] = sub.size;
    if (sub.exhausted) r.exact = 0;
    if (sub.nodes > r.nodes_max) r.nodes_max = sub.nodes;
  }
  for (int l = 0; l < n; ++l) {
    const int w = pair_winner(l, n, key, size);
    const bool kept = size[w] >= prm.min_support;
    if (pair_head(l, key)) r.n_pairs += 1, r.n_pairs_kept += kept ? 1 : 0;
    if (kept && ((best[w] >> l) & 1u)) r.kept[l >> 5] |= 1u << (l & 31), r.n_kept += 1;
  }
  *out = r;
}

// the definition, over checked records
inline void evaluate(const Rec* rec, int n, const lins_team_pcm_params& prm, uint64_t* stack, lins_team_pcm_result* out) {
  double xp[kMaxFactors][kXp];
  uint64_t adj[kMaxFactors];
  int32_t key[kMaxFactors];
  const Bars bars = bars_of(prm);
  for (int l = 0; l < n; ++l) form(rec[l].Z, rec[l].flip, rec[l].Tu, rec[l].Tv, xp[l]);
  for (int l = 0; l < n; ++l) {
    adj[l] = 0;
    for (int m = 0; m < n; ++m)
      if (m != l && consistent(xp[l], rec[l].tag, xp[m], rec[m].tag, bars)) adj[l] |= (uint64_t)1 << m;
  }
  pair_keys(rec, n, key);
  evaluate_graph(n, adj, key, prm, stack, out);
}

}  // namespace lins_pcm
