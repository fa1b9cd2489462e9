// arena_reclaim.cpp — liblins_host.so's export of the compaction plan (host/arena_reclaim.h, include/lins_lifecycle.h).
#include "arena_reclaim.h"

#include "../../../include/lins_ieskf.h"

extern "C" long long lins_host_arena_reclaim_plan(int n_blocks, const lins_arena_block* blocks, long long chunk, lins_arena_segment* segs,
                                                  long long cap, int32_t* n_passes) {
  if (chunk < 1 || cap < 0 || (cap && !segs) || !lins_reclaim::blocks_ok(n_blocks, blocks)) return LINS_E_ARG;
  std::vector<lins_arena_segment> plan;
  const int passes = lins_reclaim::plan(n_blocks, blocks, chunk, plan);
  for (size_t i = 0; i < plan.size() && (long long)i < cap; ++i) segs[i] = plan[i];
  if (n_passes) *n_passes = passes;
  return (long long)plan.size();
}
