// loop_verify.h — the two device stages every step shares (lins_loop_step, lins_loop_step_place, lins_rendezvous_step,
// lins_rendezvous_window_step), written once: ONE lins_archive_assemble over the plan of host/verify_plan.h, then ONE
// lins_loop_icp_batch_from over the hypotheses of the entries whose assemblies have no status.  A step is
//   check -> detect -> plan (entry / hyp) -> verify_assemble -> start transforms -> verify_align -> decide.
// Two functions, not one: a step reads the assembly's statistics and serial, or takes a lap, between them.
#pragma once
#include <vector>

#include "../../include/lins_map.h"
#include "../../include/lins_place.h"
#include "host/verify_plan.h"

namespace lins {

struct Verify {
  // ---- the plan: the entries that have something to verify, and their hypotheses, in call order ----
  std::vector<int> of;                  // [entry] the caller's own index of it
  std::vector<int32_t> slots, hyp0{0};  // [entry] its slot; its hypotheses are hyp0[e] .. hyp0[e + 1]
  std::vector<lins_verify::Hyp> hyps;
  void entry(int caller_index, int32_t slot) { of.push_back(caller_index), slots.push_back(slot), hyp0.push_back(hyp0.back()); }
  // a hypothesis of the entry added last: entry() comes first
  void hyp(int32_t source_id, int32_t target_slot, int32_t target_id, int32_t target_latest) {
    hyps.push_back(lins_verify::Hyp{source_id, target_slot, target_id, target_latest});
    hyp0.back() += 1;
  }
  int n() const { return (int)of.size(); }
  // ---- verify_assemble: the assembly, as laid out ----
  std::vector<lins_submap_spec> specs;
  std::vector<int32_t> kind, ids, src_spec, tgt_spec, spec0;  // [hypothesis] src_spec, tgt_spec: its two clouds
  std::vector<lins_submap_info> infos;                        // [spec]
  std::vector<int> status;                                    // [entry] lins_verify::entry_status
  // ---- verify_align ----
  std::vector<lins_loop_icp_result> icp;  // [hypothesis]; zero where nothing ran
  int n_ran = 0;                          // entries without a status: all their hypotheses went to the ICP
};

// One lins_archive_assemble of the plan's submaps (at least one entry).  A return code: v.infos and v.status are not filled.
inline int verify_assemble(lins_ctx* ctx, Verify& v, int search_num, float history_leaf) {
  const int n = v.n();
  const lins_verify::Sizes z =
      lins_verify::layout(n, v.slots.data(), v.hyp0.data(), v.hyps.data(), search_num, history_leaf, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  v.specs.resize(z.specs), v.kind.resize(z.specs), v.infos.resize(z.specs), v.ids.resize(z.ids);
  v.src_spec.resize(v.hyps.size()), v.tgt_spec.resize(v.hyps.size()), v.spec0.resize(n + 1);
  lins_verify::layout(n, v.slots.data(), v.hyp0.data(), v.hyps.data(), search_num, history_leaf, v.specs.data(), v.kind.data(), v.ids.data(),
                      v.src_spec.data(), v.tgt_spec.data(), v.spec0.data());
  if (int rc = lins_archive_assemble(ctx, (int)z.specs, v.specs.data(), v.infos.data())) return rc;
  v.status.resize(n);
  for (int e = 0; e < n; ++e) v.status[e] = lins_verify::entry_status(v.infos.data(), v.spec0[e], v.spec0[e + 1]);
  return LINS_OK;
}

// One lins_loop_icp_batch_from over every hypothesis of the entries without a status, in plan order.  T0: 16 doubles a
// hypothesis, read for those only.  v.n_ran == 0: nothing was queued.  A return code: v.icp holds zeros.
inline int verify_align(lins_ctx* ctx, Verify& v, const double* T0, const lins_loop_icp_params* prm) {
  std::vector<int> at;  // a problem's hypothesis
  std::vector<lins_loop_icp_problem> probs;
  std::vector<double> from;
  v.icp.assign(v.hyps.size(), lins_loop_icp_result{});
  v.n_ran = 0;
  for (int e = 0; e < v.n(); ++e) {
    if (v.status[e]) continue;
    v.n_ran += 1;
    for (int x = v.hyp0[e]; x < v.hyp0[e + 1]; ++x) {
      at.push_back(x);
      probs.push_back(lins_loop_icp_problem{v.src_spec[x], v.tgt_spec[x], nullptr, nullptr, 0, 0});
      from.insert(from.end(), T0 + 16 * (size_t)x, T0 + 16 * (size_t)x + 16);
    }
  }
  if (!v.n_ran) return LINS_OK;
  std::vector<lins_loop_icp_result> res(probs.size());
  if (int rc = lins_loop_icp_batch_from(ctx, (int)probs.size(), probs.data(), from.data(), prm, res.data())) return rc;
  for (size_t p = 0; p < at.size(); ++p) v.icp[at[p]] = res[p];
  return LINS_OK;
}

}  // namespace lins
