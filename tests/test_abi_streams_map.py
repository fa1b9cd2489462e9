"""The outlier cloud's constant and the calls that hand the streams' clouds to the mapping node (include/lins_host.h,
include/lins_map.h): LINS_OUTLIER_MAX as the C header has it, the prototypes compile as C, both libraries export them."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_CALLS = ("lins_segment_batch_outliers", "lins_streams_put_outliers", "lins_streams_map_cloud", "lins_local_map_build_streams",
             "lins_last_local_map_stage_ms")


def test_constant_and_prototypes_match_the_c_headers(defs):
    protos = r"""
#include "lins_streams_map.h"
int (*a)(const lins_point*, int, lins_point*) = lins_frontend_segment_outliers;
int (*b)(lins_ctx*, int, const lins_point* const*, const int32_t*, lins_segmented_scan*, lins_point* const*) = lins_segment_batch_outliers;
int (*c)(lins_ctx*, const lins_point* const*, const int32_t*) = lins_streams_put_outliers;
int (*d)(lins_ctx*, int, int, lins_point*, int) = lins_streams_map_cloud;
int (*e)(lins_ctx*, int, const int32_t*, const int32_t*, lins_local_map_sizes*) = lins_local_map_build_streams;
int (*f)(lins_ctx*, float*) = lins_last_local_map_stage_ms;
"""
    consts = r"""
#include <stdio.h>
#include "lins_host.h"
int main(void) {
  printf("%d %d\n", LINS_OUTLIER_MAX, LINS_CLOUD_MAX);
  return 0;
}
"""
    gcc = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    with tempfile.TemporaryDirectory() as d:
        p, c, exe = os.path.join(d, "p.c"), os.path.join(d, "c.c"), os.path.join(d, "c")
        open(p, "w").write(protos)
        open(c, "w").write(consts)
        subprocess.check_call(gcc + ["-c", p, "-o", os.path.join(d, "p.o")])  # (a changed signature is a compile error)
        subprocess.check_call(gcc + [c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [defs.OUTLIER_MAX, defs.CLOUD_MAX] and defs.OUTLIER_MAX == 3600


def test_both_libraries_export_the_calls(host, ieskf):
    assert hasattr(host.lib(), "lins_frontend_segment_outliers")
    for name in NEW_CALLS:
        assert name in ieskf.EXPORTS and hasattr(ieskf.lib(), name), name
