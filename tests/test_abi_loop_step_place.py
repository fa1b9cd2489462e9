"""The top-K search and the loop thread's step by appearance (include/lins_place.h lins_place_topk_batch,
lins_loop_step_place; include/lins_host.h lins_host_place_topk, lins_host_loop_choose): the prototypes compile as C99,
the ctypes mirrors of the two new structs have the C structs' sizes and offsets, the defaults are the documented ones,
and both libraries export the calls."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("lins_place_topk_batch", "lins_last_place_select_ms", "lins_loop_place_default_params", "lins_loop_step_place")
HOST_CALLS = ("lins_host_place_topk", "lins_host_loop_choose")
PARAMS = ("mode", "k", "min_sep", "reserved", "max_distance", "pad")
RESULT = ("step", "detect", "n_candidates", "chosen", "reserved", "cand", "icp")


def test_prototypes_and_layouts_match_the_c_header(defs):
    protos = r"""
#include "lins_place.h"
int (*a)(lins_ctx*, int, const lins_place_query*, int, int, lins_place_result*, int32_t*) = lins_place_topk_batch;
int (*b)(lins_ctx*, float*) = lins_last_place_select_ms;
void (*c)(lins_loop_place_params*) = lins_loop_place_default_params;
int (*d)(lins_ctx*, int, const lins_loop_step_entry*, const lins_loop_step_params*, const lins_loop_place_params*, lins_loop_place_result*) = lins_loop_step_place;
int (*e)(const float*, const float*, const double*, int, int, double, double, int, int, int32_t*, int32_t*, float*, int32_t*) = lins_host_place_topk;
int (*f)(int, const int32_t*, const double*, float) = lins_host_loop_choose;
"""

    def offsets(struct, fields):
        return ", ".join("offsetof(%s, %s)" % (struct, f) for f in fields)

    layout = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_place.h"
int main(void) {
  size_t v[] = {sizeof(lins_loop_place_params), %s, sizeof(lins_loop_place_result), %s};
  for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%%zu ", v[i]);
  printf("%%d %%d %%d\n", LINS_PLACE_MAX_K, LINS_LOOP_DETECT_PLACE, LINS_LOOP_DETECT_POSE_THEN_PLACE);
  return 0;
}
""" % (offsets("lins_loop_place_params", PARAMS), offsets("lins_loop_place_result", RESULT))
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

    assert got[:-3] == mirror(defs.LoopPlaceParamsC, PARAMS) + mirror(defs.LoopPlaceResultC, RESULT)
    assert got[-3:] == [defs.PLACE_MAX_K, defs.LOOP_DETECT_PLACE, defs.LOOP_DETECT_POSE_THEN_PLACE] == [8, 0, 1]
    assert got[0] == 24 and got[7] == 352 + 16 + 8 * 24 + 8 * C.sizeof(defs.LoopIcpResultC)


def test_both_libraries_export_the_calls_and_the_defaults(host, ieskf, defs):
    for name in HOST_CALLS:
        assert hasattr(host.lib(), name), name
    for name in NEW_CALLS:
        assert name in ieskf.PLACE_EXPORTS and hasattr(ieskf.lib(), name), name
    p = defs.loop_place_params(ieskf.lib())
    assert (p.mode, p.k, p.min_sep, p.reserved, p.max_distance, p.pad) == (defs.LOOP_DETECT_PLACE, 4, -1, 0, 1.0, 0.0)
