// rendezvous_consensus.h — which alignments of several query frames agree on one transform, the ONE scalar text of both
// libraries (lins_host_rendezvous_consensus: the definition; rendezvous_consensus_kernels.hip calls the same functions on
// its LDS copy of the table, so the device holds these bits by construction).  The contract (include/lins_host.h,
// DESIGN.md §5.3 "Rendezvous over a window"):
//   record      a hypothesis as 20 doubles — X[16] row-major, p[3], fitness — and four integers (query, rank, target_slot,
//               admissible)
//   consistent  both admissible, the same target_slot, different query; the trace of Ra^T Rb, summed row-major from the
//               left, >= 1 + 2 min_cos; |Xa p - Xb p|^2 <= max_translation^2 at p_a AND at p_b — where the robot stood, not
//               at the map origin.  Products commute and a difference changes only its sign when a and b change places, so
//               the relation is symmetric to the bit.
//   support     the population count of a 16-bit mask of the queries among a and the hypotheses consistent with a
//   order       larger support, smaller fitness, larger query, smaller rank: total, because a table names no (query, rank)
//               twice — so neither the order of the table nor the shape of a reduction shows
// f64, products and sums only, in the order written; the files that include this are compiled with -ffp-contract=off.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/lins_host.h"
#include "../lins_math.h"

namespace lins_consensus {

constexpr int kMaxHyp = LINS_RENDEZVOUS_MAX_HYP, kMaxWindow = LINS_RENDEZVOUS_MAX_WINDOW, kMaxRank = LINS_PLACE_MAX_K;
constexpr int kDoubles = 20;  // X[16] | p[3] | fitness
constexpr int kP = 16, kFitness = 19;
static_assert(kMaxHyp == 128 && kMaxWindow == 16, "a 16-bit query mask, a 128-bit member mask");
static_assert(offsetof(lins_consensus_hyp, p) == kP * 8 && offsetof(lins_consensus_hyp, fitness) == kFitness * 8 &&
                  offsetof(lins_consensus_hyp, query) == kDoubles * 8 && sizeof(lins_consensus_hyp) == (kDoubles + 2) * 8,
              "a hypothesis is 20 doubles and four integers");

struct Bars {
  double trace_min;  // 1 + 2 min_cos_rotation
  double t2_max;     // max_translation * max_translation
};
LINS_HD Bars bars_of(double max_translation, double min_cos_rotation) { return Bars{1.0 + 2.0 * min_cos_rotation, max_translation * max_translation}; }

// the integers of a hypothesis, as the kernel keeps them beside the doubles
struct Tag {
  int32_t query, rank, slot, admissible;
};

LINS_HD double trace_of(const double* Xa, const double* Xb) {
  double s = Xa[0] * Xb[0];
  s = s + Xa[1] * Xb[1], s = s + Xa[2] * Xb[2];
  s = s + Xa[4] * Xb[4], s = s + Xa[5] * Xb[5], s = s + Xa[6] * Xb[6];
  s = s + Xa[8] * Xb[8], s = s + Xa[9] * Xb[9], s = s + Xa[10] * Xb[10];
  return s;
}
LINS_HD double row_at(const double* X, int r, const double* p) { return ((X[4 * r] * p[0] + X[4 * r + 1] * p[1]) + X[4 * r + 2] * p[2]) + X[4 * r + 3]; }
LINS_HD double apart2_at(const double* Xa, const double* Xb, const double* p) {
  const double dx = row_at(Xa, 0, p) - row_at(Xb, 0, p), dy = row_at(Xa, 1, p) - row_at(Xb, 1, p), dz = row_at(Xa, 2, p) - row_at(Xb, 2, p);
  return (dx * dx + dy * dy) + dz * dz;
}

// a, b: the 20 doubles of two DIFFERENT hypotheses (the caller never asks a hypothesis about itself)
LINS_HD bool consistent(const double* a, const Tag& ta, const double* b, const Tag& tb, const Bars& bars) {
  if (!ta.admissible || !tb.admissible || ta.slot != tb.slot || ta.query == tb.query) return false;
  if (!(trace_of(a, b) >= bars.trace_min)) return false;
  return apart2_at(a, b, a + kP) <= bars.t2_max && apart2_at(a, b, b + kP) <= bars.t2_max;
}

LINS_HD int popcount16(unsigned m) {
  int n = 0;
  for (int i = 0; i < kMaxWindow; ++i) n += (int)((m >> i) & 1u);
  return n;
}

// does a come before b in the winner's order?  Both admissible, a != b.
LINS_HD bool before(int support_a, double fitness_a, const Tag& ta, int support_b, double fitness_b, const Tag& tb) {
  if (support_a != support_b) return support_a > support_b;
  if (fitness_a != fitness_b) return fitness_a < fitness_b;
  if (ta.query != tb.query) return ta.query > tb.query;
  return ta.rank < tb.rank;
}

LINS_HD bool finite64(double v) { return v - v == 0.0; }  // (no libm: false for a NaN and for an infinity)

// ---- the host side: the table's checks and the definition itself ----
inline bool bars_ok(const lins_consensus_params* p) {
  return p && finite64(p->max_translation) && p->max_translation >= 0.0 && p->min_cos_rotation == p->min_cos_rotation;
}

// LINS_OK, LINS_E_ARG or LINS_E_INPUT for one table (n_hyp is in range)
inline int table_check(const lins_consensus_hyp* h, int n_hyp) {
  unsigned char seen[kMaxWindow * kMaxRank] = {0};
  for (int i = 0; i < n_hyp; ++i) {
    if (h[i].query < 0 || h[i].query >= kMaxWindow || h[i].rank < 0 || h[i].rank >= kMaxRank || (h[i].admissible != 0 && h[i].admissible != 1))
      return LINS_E_ARG;
    unsigned char& s = seen[h[i].query * kMaxRank + h[i].rank];
    if (s) return LINS_E_ARG;
    s = 1;
  }
  for (int i = 0; i < n_hyp; ++i) {
    if (!h[i].admissible) continue;
    const double* r = (const double*)&h[i];
    for (int j = 0; j < kDoubles; ++j)
      if (!finite64(r[j])) return LINS_E_INPUT;
    if (!(h[i].fitness >= 0.0)) return LINS_E_INPUT;
  }
  return LINS_OK;
}

inline Tag tag_of(const lins_consensus_hyp& h) { return Tag{h.query, h.rank, h.target_slot, h.admissible}; }

// the definition, over a checked table
inline void evaluate(const lins_consensus_hyp* h, int n_hyp, const Bars& bars, lins_consensus_result* out) {
  int support[kMaxHyp];
  int winner = -1, n_adm = 0;
  for (int a = 0; a < n_hyp; ++a) {
    const Tag ta = tag_of(h[a]);
    unsigned mask = ta.admissible ? 1u << ta.query : 0u;
    for (int b = 0; b < n_hyp; ++b)
      if (b != a && consistent((const double*)&h[a], ta, (const double*)&h[b], tag_of(h[b]), bars)) mask |= 1u << h[b].query;
    support[a] = popcount16(mask);
    if (!ta.admissible) continue;
    ++n_adm;
    if (winner < 0 || before(support[a], h[a].fitness, ta, support[winner], h[winner].fitness, tag_of(h[winner]))) winner = a;
  }
  *out = lins_consensus_result{winner, winner < 0 ? 0 : support[winner], n_adm, 0, {0u, 0u, 0u, 0u}};
  if (winner < 0) return;
  for (int b = 0; b < n_hyp; ++b)
    if (b == winner || consistent((const double*)&h[winner], tag_of(h[winner]), (const double*)&h[b], tag_of(h[b]), bars))
      out->members[b >> 5] |= 1u << (b & 31);
}

inline void default_params(lins_consensus_params* p) {
  *p = lins_consensus_params{5, 1, 3, 0, 1.0, 0.99619469809174555};
}
// the step's own ranges (the consensus calls read the two bars only)
inline bool params_ok(const lins_consensus_params* p) {
  return bars_ok(p) && p->window >= 1 && p->window <= kMaxWindow && p->stride >= 1 && p->min_support >= 1 && p->min_support <= p->window;
}

}  // namespace lins_consensus
