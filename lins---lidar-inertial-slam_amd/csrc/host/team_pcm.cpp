// team_pcm.cpp — pairwise-consistent team factors on the CPU (include/lins_host.h lins_host_team_factors_consistent,
// lins_host_team_pcm_clique): the checks, then the definition of host/team_pcm.h with a local array for the stack.
#include "team_pcm.h"

#include <vector>

#include "../pose_graph_team.h"

using namespace lins_pcm;

extern "C" {

void lins_team_pcm_default_params(lins_team_pcm_params* p) {
  if (p) default_params(p);
}

int lins_host_team_factors_consistent(int n_factors, const lins_team_factor* factors, const double* Tb, const double* Ta,
                                      const lins_team_pcm_params* prm, lins_team_pcm_result* out) {
  if (!out || n_factors < 0 || (n_factors && (!factors || !Tb || !Ta)) || !params_ok(prm)) return LINS_E_ARG;
  for (int i = 0; i < n_factors; ++i) {
    const lins_team_factor& f = factors[i];
    if (f.slot_b < 0 || f.slot_a < 0 || f.slot_a == f.slot_b || f.id_b < 0 || f.id_a < 0) return LINS_E_ARG;
  }
  for (int i = 0; i < n_factors; ++i)
    if (!lins_pg::team_z_ok(factors[i].Z) || !lins_pg::team_var_ok(factors[i].var) || !finite12(Tb + 12 * (size_t)i) || !finite12(Ta + 12 * (size_t)i))
      return LINS_E_INPUT;
  if (n_factors > kMaxFactors) return LINS_E_CAPACITY;
  std::vector<Rec> rec((size_t)n_factors);
  for (int i = 0; i < n_factors; ++i) rec[i] = record_of(factors[i], Tb + 12 * (size_t)i, Ta + 12 * (size_t)i);
  uint64_t stack[kLevels];
  evaluate(rec.data(), n_factors, *prm, stack, out);
  return LINS_OK;
}

int lins_host_team_pcm_clique(int n, const uint64_t* adj, const int32_t* pair, const lins_team_pcm_params* prm, lins_team_pcm_result* out) {
  if (!out || n < 0 || n > kMaxFactors || (n && (!adj || !pair)) || !params_ok(prm)) return LINS_E_ARG;
  if (int rc = graph_check(n, adj, pair)) return rc;
  uint64_t stack[kLevels];
  evaluate_graph(n, adj, pair, *prm, stack, out);
  return LINS_OK;
}

}  // extern "C"
