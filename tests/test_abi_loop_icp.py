"""The ctypes mirrors of the loop-closure ICP's structs (include/lins_map.h lins_loop_icp_params / _problem / _result,
include/lins_host.h lins_loop_icp_round / _state) have the C structs' sizes and field offsets, compiled with the host compiler as
tests/test_abi_archive.py does, and both libraries export their entry points."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loop_icp_mirrors_match_the_c_structs(defs):
    src = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_host.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(lins_loop_icp_params), offsetof(lins_loop_icp_params, rotation_threshold),
         offsetof(lins_loop_icp_params, max_corr_dist), offsetof(lins_loop_icp_params, min_correspondences));
  printf("%zu %zu %zu %zu %zu\n", sizeof(lins_loop_icp_problem), offsetof(lins_loop_icp_problem, target_entry), offsetof(lins_loop_icp_problem, source),
         offsetof(lins_loop_icp_problem, target), offsetof(lins_loop_icp_problem, n_target));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(lins_loop_icp_result), offsetof(lins_loop_icp_result, fitness), offsetof(lins_loop_icp_result, mse),
         offsetof(lins_loop_icp_result, iterations), offsetof(lins_loop_icp_result, n_fitness), offsetof(lins_loop_icp_result, far_searches),
         offsetof(lins_loop_icp_result, status));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(lins_loop_icp_round), offsetof(lins_loop_icp_round, delta), offsetof(lins_loop_icp_round, T_out),
         offsetof(lins_loop_icp_round, mse), offsetof(lins_loop_icp_round, stop), offsetof(lins_loop_icp_round, reason));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(lins_loop_icp_state), offsetof(lins_loop_icp_state, mse_prev), offsetof(lins_loop_icp_state, fitness),
         offsetof(lins_loop_icp_state, move), offsetof(lins_loop_icp_state, iterations), offsetof(lins_loop_icp_state, n_corr),
         offsetof(lins_loop_icp_state, active));
  printf("%d %d %d %d %d %d\n", LINS_ICP_NONE, LINS_ICP_ITERATIONS, LINS_ICP_TRANSFORM, LINS_ICP_ABS_MSE, LINS_ICP_REL_MSE, LINS_ICP_NO_CORRESPONDENCES);
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    P, Q, R, T = defs.LoopIcpParamsC, defs.LoopIcpProblemC, defs.LoopIcpResultC, defs.LoopIcpRoundC
    assert got[:4] == [C.sizeof(P), P.rotation_threshold.offset, P.max_corr_dist.offset, P.min_correspondences.offset]
    assert got[4:9] == [C.sizeof(Q), Q.target_entry.offset, Q.source.offset, Q.target.offset, Q.n_target.offset]
    assert got[9:16] == [C.sizeof(R), R.fitness.offset, R.mse.offset, R.iterations.offset, R.n_fitness.offset, R.far_searches.offset, R.status.offset]
    assert got[16:22] == [C.sizeof(T), T.delta.offset, T.T_out.offset, T.mse.offset, T.stop.offset, T.reason.offset]
    S = defs.LoopIcpStateC
    assert got[22:29] == [C.sizeof(S), S.mse_prev.offset, S.fitness.offset, S.move.offset, S.iterations.offset, S.n_corr.offset, S.active.offset]
    assert got[29:] == [defs.ICP_NONE, defs.ICP_ITERATIONS, defs.ICP_TRANSFORM, defs.ICP_ABS_MSE, defs.ICP_REL_MSE, defs.ICP_NO_CORRESPONDENCES]


def test_default_parameters_are_the_mapping_nodes(host, ieskf, defs):
    for lib in (host.lib(), ieskf.lib()):
        p = defs.loop_icp_params(lib)
        assert (p.max_corr_dist, p.max_iterations, p.transformation_epsilon, p.fitness_epsilon, p.rel_mse, p.rotation_threshold,
                p.min_correspondences, p.reserved) == (100.0, 100, 1e-6, 1e-6, 1e-5, 0.99999, 3, 0)


def test_both_libraries_export_the_loop_icp(host, ieskf):
    for name in ("lins_host_loop_icp", "lins_host_loop_icp_correspondences", "lins_host_loop_icp_trace", "lins_host_loop_pose_from",
                 "lins_host_loop_icp_step", "lins_loop_icp_default_params"):
        assert hasattr(host.lib(), name), name
    want = {"lins_loop_icp_default_params", "lins_loop_icp_batch", "lins_loop_icp_correspondences", "lins_last_loop_icp_stats"}
    assert want <= set(ieskf.EXPORTS)
    for name in sorted(want) + ["lins_debug_loop_icp_rounds", "lins_debug_loop_icp_shells", "lins_debug_loop_icp_group", "lins_debug_loop_icp_last_far",
                                "lins_debug_loop_icp_step"]:
        assert hasattr(ieskf.lib(), name), name
