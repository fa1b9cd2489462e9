"""Place recognition (include/lins_place.h, the lins_host_place_* part of include/lins_host.h): the prototypes compile as
C99, the ctypes mirrors have the C structs' sizes and offsets, both libraries export their calls, and
ieskf.PLACE_EXPORTS is the header's list."""
import ctypes as C
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOST_CALLS = ("lins_place_default_params", "lins_host_place_descriptor", "lins_host_place_distance", "lins_host_place_search",
              "lins_host_place_guess", "lins_host_loop_icp_from")


def test_prototypes_and_layouts_match_the_c_header(defs):
    protos = r"""
#include "lins_place.h"
void (*a)(lins_place_params*) = lins_place_default_params;
int (*b)(lins_ctx*, const lins_place_params*) = lins_place_init;
int (*c)(lins_ctx*, int, const int32_t*) = lins_place_sync;
int (*d)(lins_ctx*, int, const lins_place_query*, lins_place_result*) = lins_place_search_batch;
int (*e)(lins_ctx*, int, int, float*) = lins_place_descriptor;
int (*f)(lins_ctx*, const lins_place_query*, float*, int32_t*, int) = lins_place_distances;
int (*g)(lins_ctx*, int) = lins_place_set_chunk;
int (*h)(lins_ctx*, float*, float*, uint64_t*, int32_t*) = lins_last_place_stats;
int (*i)(lins_ctx*, int, const lins_loop_icp_problem*, const double*, const lins_loop_icp_params*, lins_loop_icp_result*) = lins_loop_icp_batch_from;
int (*j)(const lins_keyframe*, const lins_place_params*, float*) = lins_host_place_descriptor;
int (*k)(const float*, const float*, float*) = lins_host_place_distance;
int (*l)(const float*, const float*, const double*, int, int, double, double, int32_t*, int32_t*, float*, int32_t*) = lins_host_place_search;
int (*m)(const lins_key_pose*, const lins_key_pose*, int, int, double*) = lins_host_place_guess;
int (*n)(const lins_point*, int, const lins_point*, int, const double*, const lins_loop_icp_params*, int, lins_loop_icp_result*) = lins_host_loop_icp_from;
"""
    layout = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_place.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(lins_place_params), offsetof(lins_place_params, lift),
         offsetof(lins_place_params, up_axis), offsetof(lins_place_params, clouds), sizeof(lins_place_query), offsetof(lins_place_query, target_slot),
         offsetof(lins_place_query, now), offsetof(lins_place_query, min_gap_s), sizeof(lins_place_result), offsetof(lins_place_result, distance),
         offsetof(lins_place_result, candidates), offsetof(lins_place_result, status), LINS_PLACE_RINGS, LINS_PLACE_SECTORS, LINS_PLACE_CELLS);
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
    P, Q, R = defs.PlaceParamsC, defs.PlaceQueryC, defs.PlaceResultC
    assert got == [C.sizeof(P), P.lift.offset, P.up_axis.offset, P.clouds.offset, C.sizeof(Q), Q.target_slot.offset, Q.now.offset,
                   Q.min_gap_s.offset, C.sizeof(R), R.distance.offset, R.candidates.offset, R.status.offset, defs.PLACE_RINGS,
                   defs.PLACE_SECTORS, defs.PLACE_CELLS]
    assert (got[0], got[4], got[8]) == (16, 32, 24)


def test_both_libraries_export_the_calls(host, ieskf):
    text = open(os.path.join(ROOT, "include", "lins_place.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(lins_[a-z0-9_]+)\s*\(", text)))
    assert sorted(ieskf.PLACE_EXPORTS) == sorted(declared + ["lins_place_default_params"])
    for name in HOST_CALLS:
        assert hasattr(host.lib(), name), name
    for name in ieskf.PLACE_EXPORTS:
        assert hasattr(ieskf.lib(), name), name


def test_default_params_agree(host, ieskf, defs):
    a, b = defs.place_params(host.lib()), defs.place_params(ieskf.lib())
    assert (a.r_max, a.lift, a.up_axis, a.clouds) == (b.r_max, b.lift, b.up_axis, b.clouds) == (80.0, 2.0, 1, 7)
