"""The team map's calls (include/lins_map.h, lins_streams_map.h, lins_host.h): the prototypes compile as C99, the ctypes
mirror has the C struct's size and offsets, both libraries export their calls, and the calls that need no device keep the
conventions (a NULL context is LINS_E_ARG)."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("lins_keyposes_team_select_batch", "lins_last_keyposes_team_stats", "lins_local_map_build_team", "lins_local_map_build_team_streams",
         "lins_streams_map_team", "lins_streams_map_team_groups", "lins_streams_map_team_group", "lins_streams_map_team_list")
HOST_CALLS = ("lins_host_team_select", "lins_host_team_map")
E_ARG = -1


def test_prototypes_and_layouts_match_the_c_header(defs):
    protos = r"""
#include "lins_host.h"
#include "lins_map.h"
#include "lins_streams_map.h"
int (*a)(lins_ctx*, int, const lins_keyposes_team_query*, const int32_t*, int, int32_t*, int, lins_keyposes_result*) = lins_keyposes_team_select_batch;
int (*b)(lins_ctx*, float*, int32_t*, uint64_t*) = lins_last_keyposes_team_stats;
int (*c)(lins_ctx*, int, const int32_t*, const int32_t* const*, const int32_t*, const lins_local_scan*, lins_local_map_sizes*) = lins_local_map_build_team;
int (*d)(lins_ctx*, int, const int32_t*, const int32_t* const*, const int32_t*, const int32_t*, lins_local_map_sizes*) = lins_local_map_build_team_streams;
int (*e)(lins_ctx*, int, float, float) = lins_streams_map_team;
int (*f)(lins_ctx*, int, const int32_t*, const int32_t*) = lins_streams_map_team_groups;
int (*g)(lins_ctx*, int, int32_t*) = lins_streams_map_team_group;
int (*h)(lins_ctx*, int, int32_t*, int) = lins_streams_map_team_list;
int (*i)(int, const int32_t*, const lins_key_pose* const*, const int32_t*, const float*, float, float, int32_t*, int) = lins_host_team_select;
int (*j)(int, const lins_keyframe* const*, const int32_t*, const int32_t*, int, const lins_local_scan*, lins_point* const*, lins_local_map_sizes*) = lins_host_team_map;
"""
    layout = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_map.h"
#define S(t) printf("%zu ", sizeof(t))
#define O(t, f) printf("%zu ", offsetof(t, f))
int main(void) {
  S(lins_keyposes_team_query); O(lins_keyposes_team_query, radius); O(lins_keyposes_team_query, pose_leaf); O(lins_keyposes_team_query, n_targets);
  O(lins_keyposes_team_query, first_target); O(lins_keyposes_team_query, reserved);
  printf("%d\n", LINS_KEYPOSES_TEAM_CELLS);
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
    Q = defs.KeyposesTeamQueryC
    assert got == [C.sizeof(Q), Q.radius.offset, Q.pose_leaf.offset, Q.n_targets.offset, Q.first_target.offset, Q.reserved.offset,
                   defs.KEYPOSES_TEAM_CELLS]
    assert C.sizeof(Q) == 32


def test_both_libraries_export_the_calls(host, ieskf):
    assert sorted(ieskf.TEAM_MAP_EXPORTS) == sorted(CALLS)
    assert not set(CALLS) & set(ieskf.EXPORTS) and not set(CALLS) & set(ieskf.TEAM_EXPORTS)
    for name in CALLS:
        assert hasattr(ieskf.lib(), name), name
    for name in HOST_CALLS:
        assert hasattr(host.lib(), name), name


def test_conventions_without_a_device(host, ieskf):
    L = ieskf.lib()
    vp = C.c_void_p
    L.lins_keyposes_team_select_batch.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp]
    L.lins_last_keyposes_team_stats.argtypes = [vp] * 4
    L.lins_local_map_build_team.argtypes = [vp, C.c_int] + [vp] * 5
    L.lins_local_map_build_team_streams.argtypes = [vp, C.c_int] + [vp] * 5
    L.lins_streams_map_team.argtypes = [vp, C.c_int, C.c_float, C.c_float]
    L.lins_streams_map_team_groups.argtypes = [vp, C.c_int, vp, vp]
    L.lins_streams_map_team_group.argtypes = [vp, C.c_int, vp]
    L.lins_streams_map_team_list.argtypes = [vp, C.c_int, vp, C.c_int]
    for n in (0, 1):  # a NULL context is refused before n is looked at
        assert L.lins_keyposes_team_select_batch(None, n, None, None, 0, None, 0, None) == E_ARG
        assert L.lins_local_map_build_team(None, n, None, None, None, None, None) == E_ARG
        assert L.lins_local_map_build_team_streams(None, n, None, None, None, None, None) == E_ARG
        assert L.lins_streams_map_team_groups(None, n, None, None) == E_ARG
        assert L.lins_streams_map_team(None, n, 50.0, 1.0) == E_ARG
    assert L.lins_last_keyposes_team_stats(None, None, None, None) == E_ARG
    assert L.lins_streams_map_team_group(None, 0, None) == E_ARG and L.lins_streams_map_team_list(None, 0, None, 0) == E_ARG
    H = host.lib()
    H.lins_host_team_select.argtypes = [C.c_int, vp, vp, vp, vp, C.c_float, C.c_float, vp, C.c_int]
    H.lins_host_team_select.restype = C.c_int
    centre = (C.c_float * 3)(0, 0, 0)
    assert H.lins_host_team_select(0, None, None, None, centre, 1.0, 1.0, None, 0) == 0  # no targets: nothing selected
    assert H.lins_host_team_select(1, None, None, None, centre, 1.0, 1.0, None, 0) == E_ARG
    assert H.lins_host_team_select(0, None, None, None, None, 1.0, 1.0, None, 0) == E_ARG
