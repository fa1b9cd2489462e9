"""The mapping node's step for streams (include/lins_streams_map.h, include/lins_host.h): the prototypes compile as C,
the ctypes mirrors have the C structs' sizes and offsets, both libraries export the calls."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_CALLS = ("lins_map_associate_batch", "lins_streams_map_init", "lins_streams_map_get_pose", "lins_streams_map_set_pose",
             "lins_streams_map_step", "lins_last_streams_map_ms")
HOST_CALLS = ("lins_host_map_associate", "lins_host_map_transform_update", "lins_host_map_key_rule")


def test_prototypes_and_layouts_match_the_c_headers(defs):
    protos = r"""
#include "lins_streams_map.h"
int (*a)(lins_ctx*, int, const float*, const float*, const float*, float*) = lins_map_associate_batch;
int (*b)(lins_ctx*, int, double) = lins_streams_map_init;
int (*c)(lins_ctx*, int, lins_map_pose_state*) = lins_streams_map_get_pose;
int (*d)(lins_ctx*, int, const lins_map_pose_state*) = lins_streams_map_set_pose;
int (*e)(lins_ctx*, int, const int32_t*, const lins_map_odom*, lins_map_step_result*) = lins_streams_map_step;
int (*f)(lins_ctx*, float*, float*) = lins_last_streams_map_ms;
void (*g)(const float*, const float*, const float*, float*) = lins_host_map_associate;
void (*h)(float*, int, float, float, const float*, float*, float*) = lins_host_map_transform_update;
int (*i)(float*, const float*, int) = lins_host_map_key_rule;
"""
    layout = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_streams_map.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(lins_map_pose_state), offsetof(lins_map_pose_state, n_frames),
         offsetof(lins_map_pose_state, last_time), sizeof(lins_map_odom), offsetof(lins_map_odom, time), sizeof(lins_map_step_result),
         offsetof(lins_map_step_result, status), offsetof(lins_map_step_result, archive_id), LINS_MAP_STEP_SKIPPED);
  return 0;
}
"""
    gcc = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    with tempfile.TemporaryDirectory() as d:
        p, c, exe = os.path.join(d, "p.c"), os.path.join(d, "c.c"), os.path.join(d, "c")
        open(p, "w").write(protos)
        open(c, "w").write(layout)
        subprocess.check_call(gcc + ["-c", p, "-o", os.path.join(d, "p.o")])  # (a changed signature is a compile error)
        subprocess.check_call(gcc + [c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    P, O, R = defs.MapPoseStateC, defs.MapOdomC, defs.MapStepResultC
    assert got == [C.sizeof(P), P.n_frames.offset, P.last_time.offset, C.sizeof(O), O.time.offset, C.sizeof(R), R.status.offset,
                   R.archive_id.offset, defs.MAP_STEP_SKIPPED]


def test_both_libraries_export_the_calls(host, ieskf):
    for name in HOST_CALLS:
        assert hasattr(host.lib(), name), name
    for name in NEW_CALLS:
        assert name in ieskf.EXPORTS and hasattr(ieskf.lib(), name), name
