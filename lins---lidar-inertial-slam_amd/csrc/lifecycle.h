// lifecycle.h — what the files behind include/lins_lifecycle.h share: every module's release is a check (nothing
// changed) and an apply (cannot refuse, short of a HIP error), so that lins_streams_retire asks every initialised module
// first and a refused call changes nothing anywhere.  The apply functions expect the context quiesced (ctx_quiesce).
#pragma once
#include "lins_ctx_priv.h"

namespace lins {

// lins_capi.hip: the context's device current, its stream behind the second launch queue, and synchronised
int ctx_quiesce(lins_ctx* ctx);

// ids[0 .. n): each in [0, limit), none twice (LINS_E_ARG otherwise)
inline int release_list_check(int n, const int32_t* ids, int limit) {
  if (n < 0 || (n && !ids)) return LINS_E_ARG;
  for (int k = 0; k < n; ++k) {
    if (ids[k] < 0 || ids[k] >= limit) return LINS_E_ARG;
    for (int i = 0; i < k; ++i)
      if (ids[i] == ids[k]) return LINS_E_ARG;
  }
  return LINS_OK;
}

int archive_slots(lins_ctx* ctx);  // lins_archive_capi.hip: n_slots of lins_archive_init (0 before it)
int archive_release_apply(lins_ctx* ctx, int n, const int32_t* slots, long long* released);
int local_map_release_apply(lins_ctx* ctx, int n, const int32_t* slots);     // lins_local_map_capi.hip
int pose_graph_release_apply(lins_ctx* ctx, int n, const int32_t* slots);    // lins_pose_graph_capi.hip
int streams_map_release_apply(lins_ctx* ctx, int n, const int32_t* streams);  // lins_streams_map_capi.hip
int streams_release_apply(lins_ctx* ctx, int n, const int32_t* streams);      // lins_lifecycle_capi.hip

}  // namespace lins
