// verify_plan.h — the LAYOUT of the stage every step shares (lins_loop_step, lins_loop_step_place, lins_rendezvous_step,
// lins_rendezvous_window_step; DESIGN.md §5.3 "Loop thread's step"): which submaps one lins_archive_assemble builds for the
// alignments a call wants verified, and which two of them each alignment reads.  Defined ONCE; the two stages around it are
// loop_verify.h.  Scalar host work in the style of loop_step.h.
//   hypothesis  one alignment: a frame of the entry's slot (the source) against the history window around a frame of a
//               target slot.  Within one entry, hypotheses with the same source frame share one source cloud.
//   the rule    walk the entries, then their hypotheses, in call order.  A source spec — the one frame, corner | surf,
//               LINS_SUBMAP_DROP_NEGATIVE, leaf 0 — is emitted immediately before the first hypothesis that names it; the
//               hypothesis's target spec — lins_loop::window(target_latest, target_id, search_num) of the target slot,
//               corner | surf, flags 0, leaf history_leaf — follows.  One hypothesis an entry: specs 2i, 2i + 1.  One source
//               and k targets: first, first + 1 + j.  Several sources: each in front of its first target; a frame no
//               hypothesis names gets none.
// Also what an entry makes of its specs' and its alignments' statuses, and the parameter ranges the stage reads.
#pragma once
#include <stdint.h>

#include <cmath>

#include "../../../include/lins_map.h"
#include "loop_step.h"

namespace lins_verify {

constexpr int kSource = 0, kTarget = 1;  // a spec's kind

struct Hyp {
  int32_t source_id;                              // a frame of the entry's slot
  int32_t target_slot, target_id, target_latest;  // the window's middle, and the newest frame of its slot
};

struct Sizes {
  long long specs, ids;
};

// Entry e's hypotheses are hyps[hyp0[e] .. hyp0[e + 1]), its slot is slots[e].  With specs == nullptr nothing is written:
// the return value sizes the arrays of the second call — specs and kind [specs], ids [ids], src_spec and tgt_spec
// [hyp0[n]], spec0 [n + 1] (entry e's specs are spec0[e] .. spec0[e + 1)).  A spec's ids point into `ids`.
inline Sizes layout(int n, const int32_t* slots, const int32_t* hyp0, const Hyp* hyps, int search_num, float history_leaf, lins_submap_spec* specs,
                    int32_t* kind, int32_t* ids, int32_t* src_spec, int32_t* tgt_spec, int32_t* spec0) {
  Sizes at{0, 0};
  for (int e = 0; e < n; ++e) {
    if (specs) spec0[e] = (int32_t)at.specs;
    for (int x = hyp0[e]; x < hyp0[e + 1]; ++x) {
      int named = hyp0[e];  // the first hypothesis of the entry with x's source
      while (hyps[named].source_id != hyps[x].source_id) ++named;
      if (named == x) {
        if (specs) {
          ids[at.ids] = hyps[x].source_id;
          specs[at.specs] = lins_submap_spec{ids + at.ids, 1, slots[e], LINS_SUBMAP_CORNER | LINS_SUBMAP_SURF, LINS_SUBMAP_DROP_NEGATIVE, 0.f, 0};
          kind[at.specs] = kSource, src_spec[x] = (int32_t)at.specs;
        }
        at.specs += 1, at.ids += 1;
      } else if (specs) {
        src_spec[x] = src_spec[named];
      }
      const int w = lins_loop::window_size(hyps[x].target_latest, hyps[x].target_id, search_num);
      if (specs) {
        lins_loop::window(hyps[x].target_latest, hyps[x].target_id, search_num, ids + at.ids);
        specs[at.specs] = lins_submap_spec{ids + at.ids, w, hyps[x].target_slot, LINS_SUBMAP_CORNER | LINS_SUBMAP_SURF, 0, history_leaf, 0};
        kind[at.specs] = kTarget, tgt_spec[x] = (int32_t)at.specs;
      }
      at.specs += 1, at.ids += w;
    }
  }
  if (specs) spec0[n] = (int32_t)at.specs;
  return at;
}

// an entry's status: the first non-zero status of its specs, in spec order (nothing is aligned for such an entry)
inline int entry_status(const lins_submap_info* infos, int spec_begin, int spec_end) {
  for (int s = spec_begin; s < spec_end; ++s)
    if (infos[s].status) return infos[s].status;
  return 0;
}

struct IcpSummary {
  int status;  // the first non-zero status of the k alignments (a target box beyond the gridding's limit: nothing was run)
  int ran;     // how many have none
};
// conv / fit (k each, or both null): what lins_loop::choose is handed — an alignment with a status counts as not converged
inline IcpSummary icp_summary(const lins_loop_icp_result* icp, int k, int32_t* conv, double* fit) {
  IcpSummary s{0, 0};
  for (int j = 0; j < k; ++j) {
    if (conv) conv[j] = icp[j].status ? 0 : icp[j].converged, fit[j] = icp[j].fitness;
    if (icp[j].status && !s.status) s.status = icp[j].status;
    s.ran += icp[j].status ? 0 : 1;
  }
  return s;
}

// the ranges of what the stage and the detection in front of it read of a step's parameters (lins_archive_assemble,
// lins_loop_icp_batch_from, lins_loop::accept); a caller with more parameters checks the rest
inline bool params_ok(const lins_loop_step_params* p) {
  return p && !std::isnan(p->max_fitness) && std::isfinite(p->history_leaf) && p->history_leaf >= 0.f && p->search_num >= 0 && !std::isnan(p->min_gap_s) &&
         p->icp.max_iterations >= 1 && p->icp.min_correspondences >= 0 && std::isfinite(p->icp.max_corr_dist);
}

}  // namespace lins_verify
