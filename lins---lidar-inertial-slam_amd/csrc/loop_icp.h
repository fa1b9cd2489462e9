// loop_icp.h — the device records of the loop-closure ICP (loop_icp_kernels.hip, lins_loop_icp_capi.hip); the state
// of a problem between two rounds is lins_licp::State (loop_icp_math.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lins_map.h"
#include "lins_records.h"
#include "loop_icp_math.h"

namespace lins {

constexpr int kLoopBlock = 256;
constexpr int kLoopLanes = 8;                             // lanes per query: they share the scan of its cells
constexpr int kLoopQPerBlock = kLoopBlock / kLoopLanes;   // = lins_licp::kTile: one workgroup forms one tile of the sums
constexpr int kLoopShells = 3;                            // default shell budget: the query's own cell and two shells around it
static_assert(kLoopQPerBlock == lins_licp::kTile && kLoopLanes == lins_licp::kGroup, "the sums' tree is the workgroup's shape");

struct LoopDev {  // one problem
  MapGrid g;             // the target, gridded into 1 m cells (map_grid_kernel)
  const float4* src;     // the source points where they lie (archive cloud arena or the upload arena)
  const float4* tgt;     // the target points in cloud order
  int n_src, n_tgt;
  int status, pad;       // != 0: the problem is not run
};
static_assert(sizeof(LoopDev) == 72, "LoopDev layout");

// mode 0: a round (problems that stopped return at once; cap2 < 0: no cap), 1: the fitness pass (every problem, no cap)
void launch_loop_search(hipStream_t s, int n_problems, int blocks_per_problem, int mode, int shells, float cap2, const LoopDev* probs,
                        lins_licp::State* states, const float4* pts, const int* cells, double* partials, int32_t* out_idx, float* out_d);
// one wave per problem: sums in tile order, then steps 3-6 (mode 0; still_running, may be null, counts the problems
// that go on) or the fitness score (mode 1)
void launch_loop_step(hipStream_t s, int n_problems, int blocks_per_problem, int mode, const lins_loop_icp_params& prm, const LoopDev* probs,
                      lins_licp::State* states, const double* partials, int* still_running);

// lins_loop_icp_capi.hip, for the test aids of lins_capi_debug.hip — which: 0 rounds, 1 shells, 2 group
int loop_icp_debug_set(lins_ctx* ctx, int which, int value);
int loop_icp_debug_shells_default();
unsigned loop_icp_last_far(lins_ctx* ctx);

}  // namespace lins
