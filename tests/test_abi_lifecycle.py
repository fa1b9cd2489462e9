"""Stream lifecycle (include/lins_lifecycle.h): the prototypes compile as C99, the ctypes mirrors of the plan's records
have the C structs' sizes and offsets, both libraries export their calls."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_CALLS = ("lins_archive_usage", "lins_archive_release_slots", "lins_archive_set_reclaim_chunk", "lins_pose_graph_release_slot",
             "lins_local_map_release_slot", "lins_streams_release", "lins_streams_map_release", "lins_streams_retire",
             "lins_last_reclaim_stats")
HOST_CALLS = ("lins_host_arena_reclaim_plan",)


def test_prototypes_and_layouts_match_the_c_header(defs):
    protos = r"""
#include "lins_lifecycle.h"
int (*a)(lins_ctx*, long long*, long long*) = lins_archive_usage;
int (*b)(lins_ctx*, int, const int32_t*, long long*) = lins_archive_release_slots;
int (*c)(lins_ctx*, long long) = lins_archive_set_reclaim_chunk;
int (*d)(lins_ctx*, int) = lins_pose_graph_release_slot;
int (*e)(lins_ctx*, int) = lins_local_map_release_slot;
int (*f)(lins_ctx*, int, const int32_t*) = lins_streams_release;
int (*g)(lins_ctx*, int, const int32_t*) = lins_streams_map_release;
int (*h)(lins_ctx*, int, const int32_t*) = lins_streams_retire;
int (*i)(lins_ctx*, float*, uint64_t*, int32_t*, int32_t*) = lins_last_reclaim_stats;
long long (*j)(int, const lins_arena_block*, long long, lins_arena_segment*, long long, int32_t*) = lins_host_arena_reclaim_plan;
/* the header brings the streams' end-to-end calls with it */
int (*k)(lins_ctx*, int, const int32_t*, lins_fused_pose*) = lins_streams_fuse;
"""
    layout = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_lifecycle.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(lins_arena_block), offsetof(lins_arena_block, n), offsetof(lins_arena_block, keep),
         sizeof(lins_arena_segment), offsetof(lins_arena_segment, dst), offsetof(lins_arena_segment, n), offsetof(lins_arena_segment, pass),
         offsetof(lins_arena_segment, direct), sizeof(long long));
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
    B, S = defs.ArenaBlockC, defs.ArenaSegmentC
    assert got == [C.sizeof(B), B.n.offset, B.keep.offset, C.sizeof(S), S.dst.offset, S.n.offset, S.pass_.offset, S.direct.offset,
                   C.sizeof(C.c_longlong)]
    assert got[0] == 24 and got[3] == 32


def test_both_libraries_export_the_calls(host, ieskf):
    assert sorted(ieskf.LIFECYCLE_EXPORTS) == sorted(NEW_CALLS)
    for name in HOST_CALLS:
        assert hasattr(host.lib(), name), name
    for name in NEW_CALLS:
        assert name in ieskf.LIFECYCLE_EXPORTS and hasattr(ieskf.lib(), name), name
