"""The loop thread's step (include/lins_map.h lins_loop_step, include/lins_streams_map.h lins_streams_map_loop,
include/lins_host.h lins_host_loop_*): the prototypes compile as C, the ctypes mirrors of the three structs have the C
structs' sizes and offsets — which this test pins — and both libraries export the calls."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_CALLS = ("lins_loop_step_default_params", "lins_loop_step", "lins_loop_closed_cloud", "lins_last_loop_step_stats",
             "lins_pose_graph_apply_batch", "lins_streams_map_loop")
HOST_CALLS = ("lins_host_loop_window", "lins_host_loop_candidate", "lins_host_loop_accept", "lins_host_loop_variance",
              "lins_host_loop_pose_from")

PARAMS = ("search_radius", "max_fitness", "history_leaf", "search_num", "min_gap_s", "icp", "graph")
ENTRY = ("slot", "stream", "flags", "reserved", "centre", "pad", "now")
RESULT = ("outcome", "status", "latest_id", "closest_id", "latest", "history", "icp", "pose_from", "graph")
# the layout, pinned: (sizeof, offsets in the order above)
PINNED = {"params": (120, [0, 4, 8, 12, 16, 24, 72]), "entry": (40, [0, 4, 8, 12, 16, 28, 32]),
          "result": (352, [0, 4, 8, 12, 16, 64, 112, 288, 312])}


def test_prototypes_and_layouts_match_the_c_headers(defs):
    protos = r"""
#include "lins_streams_map.h"
void (*a)(lins_loop_step_params*) = lins_loop_step_default_params;
int (*b)(lins_ctx*, int, const lins_loop_step_entry*, const lins_loop_step_params*, lins_loop_step_result*) = lins_loop_step;
int (*c)(lins_ctx*, int, lins_point*, int) = lins_loop_closed_cloud;
int (*d)(lins_ctx*, float*, float*, float*, int32_t*, int32_t*, int32_t*) = lins_last_loop_step_stats;
int (*e)(lins_ctx*, int, const int32_t*, const int32_t*) = lins_pose_graph_apply_batch;
int (*f)(lins_ctx*, int) = lins_streams_map_loop;
int (*g)(int, int, int, int32_t*, int) = lins_host_loop_window;
int (*h)(int, int, int, int) = lins_host_loop_candidate;
int (*i)(int, double, float) = lins_host_loop_accept;
int (*j)(double, double*) = lins_host_loop_variance;
"""

    def offsets(struct, fields):
        return ", ".join("offsetof(%s, %s)" % (struct, f) for f in fields)

    layout = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_map.h"
int main(void) {
  size_t v[] = {sizeof(lins_loop_step_params), %s, sizeof(lins_loop_step_entry), %s, sizeof(lins_loop_step_result), %s};
  for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%%zu ", v[i]);
  printf("%%d %%d %%d %%d %%d\n", LINS_LOOP_NONE, LINS_LOOP_REPEAT, LINS_LOOP_REJECTED, LINS_LOOP_CLOSED, LINS_LOOP_CENTRE_STREAM);
  return 0;
}
""" % (offsets("lins_loop_step_params", PARAMS), offsets("lins_loop_step_entry", ENTRY), offsets("lins_loop_step_result", RESULT))
    gcc = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    with tempfile.TemporaryDirectory() as d:
        p, c, exe = os.path.join(d, "p.c"), os.path.join(d, "c.c"), os.path.join(d, "c")
        open(p, "w").write(protos)
        open(c, "w").write(layout)
        subprocess.check_call(gcc + ["-c", p, "-o", os.path.join(d, "p.o")])  # (a changed signature is a compile error)
        subprocess.check_call(gcc + [c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]

    def mirror(T, fields):
        return [C.sizeof(T)] + [getattr(T, f).offset for f in fields]

    want = mirror(defs.LoopStepParamsC, PARAMS) + mirror(defs.LoopStepEntryC, ENTRY) + mirror(defs.LoopStepResultC, RESULT)
    assert got[:-5] == want
    assert got[-5:] == [defs.LOOP_NONE, defs.LOOP_REPEAT, defs.LOOP_REJECTED, defs.LOOP_CLOSED, defs.LOOP_CENTRE_STREAM] == [0, 1, 2, 3, 1]
    pinned = [x for k in ("params", "entry", "result") for x in [PINNED[k][0]] + PINNED[k][1]]
    assert got[:-5] == pinned


def test_both_libraries_export_the_calls(host, ieskf):
    for name in HOST_CALLS:
        assert hasattr(host.lib(), name), name
    for name in NEW_CALLS:
        assert name in ieskf.EXPORTS and hasattr(ieskf.lib(), name), name


def test_the_defaults_are_the_references(defs, ieskf):
    p = defs.loop_step_params(ieskf.lib())
    assert (p.search_radius, p.max_fitness, p.history_leaf, p.search_num, p.min_gap_s) == (5.0, C.c_float(0.3).value, C.c_float(0.4).value, 25, 30.0)
    icp, graph = defs.loop_icp_params(ieskf.lib()), defs.pose_graph_params(ieskf.lib())
    assert bytes(p.icp) == bytes(icp) and bytes(p.graph) == bytes(graph)
