"""Pairwise-consistent team factors (include/lins_team.h, the records of include/lins_host.h): the prototypes compile as C99,
the ctypes mirrors have the C structs' sizes and offsets, the defaults are the documented ones in both libraries, both
libraries export their calls, and the calls that need no device keep the conventions."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("lins_team_pcm_default_params", "lins_team_factors_consistent_batch", "lins_last_team_pcm_stats")
HOST_CALLS = ("lins_team_pcm_default_params", "lins_host_team_factors_consistent", "lins_host_team_pcm_clique")
E_ARG = -1


def test_prototypes_and_layouts_match_the_c_header(defs):
    protos = r"""
#include "lins_team.h"
int (*a)(lins_ctx*, int, const lins_team_member*, const int32_t*, const lins_team_factor*, const int32_t*, const lins_team_pcm_params*,
         lins_team_pcm_result*) = lins_team_factors_consistent_batch;
int (*b)(lins_ctx*, float*) = lins_last_team_pcm_stats;
int (*c)(lins_ctx*, int, const uint64_t*, const int32_t*, const lins_team_pcm_params*, lins_team_pcm_result*) = lins_debug_team_pcm_clique;
int (*d)(int, const lins_team_factor*, const double*, const double*, const lins_team_pcm_params*, lins_team_pcm_result*) = lins_host_team_factors_consistent;
int (*e)(int, const uint64_t*, const int32_t*, const lins_team_pcm_params*, lins_team_pcm_result*) = lins_host_team_pcm_clique;
void (*f)(lins_team_pcm_params*) = lins_team_pcm_default_params;
"""
    layout = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_team.h"
#define S(t) printf("%zu ", sizeof(t))
#define O(t, f) printf("%zu ", offsetof(t, f))
int main(void) {
  S(lins_team_pcm_params); O(lins_team_pcm_params, min_cos_rotation); O(lins_team_pcm_params, translation_per_frame);
  O(lins_team_pcm_params, min_support); O(lins_team_pcm_params, max_nodes);
  S(lins_team_pcm_result); O(lins_team_pcm_result, n_kept); O(lins_team_pcm_result, n_pairs); O(lins_team_pcm_result, n_pairs_kept);
  O(lins_team_pcm_result, exact); O(lins_team_pcm_result, nodes_max); O(lins_team_pcm_result, kept);
  printf("%d\n", LINS_TEAM_PCM_MAX_FACTORS);
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
    sz = C.sizeof
    P, R = defs.TeamPcmParamsC, defs.TeamPcmResultC
    want = [sz(P), P.min_cos_rotation.offset, P.translation_per_frame.offset, P.min_support.offset, P.max_nodes.offset,
            sz(R), R.n_kept.offset, R.n_pairs.offset, R.n_pairs_kept.offset, R.exact.offset, R.nodes_max.offset, R.kept.offset,
            defs.TEAM_PCM_MAX_FACTORS]
    assert got == want
    assert (sz(P), sz(R), R.kept.offset, defs.TEAM_PCM_MAX_FACTORS) == (32, 32, 24, 64)  # a result is two 16-byte stores


def test_both_libraries_export_the_calls_and_agree_on_the_defaults(host, ieskf, defs):
    assert sorted(ieskf.TEAM_PCM_EXPORTS) == sorted(CALLS)
    for name in CALLS + ("lins_debug_team_pcm_clique",):
        assert hasattr(ieskf.lib(), name), name
    for name in HOST_CALLS:
        assert hasattr(host.lib(), name), name
    assert not set(CALLS) & (set(ieskf.EXPORTS) | set(ieskf.TEAM_EXPORTS) | set(ieskf.TEAM_GRAPH_EXPORTS))
    for L in (host.lib(), ieskf.lib()):
        p = defs.team_pcm_params(L)
        assert (p.max_translation, p.translation_per_frame, p.min_support, p.max_nodes) == (1.0, 0.0, 3, 65536)
        assert p.min_cos_rotation == 0.99619469809174555  # cos 5 degrees, the literal of lins_consensus_params
        assert defs.team_pcm_params(L, min_support=2, translation_per_frame=0.03).min_support == 2


def test_conventions_without_a_device(ieskf, defs):
    L = ieskf.lib()
    L.lins_team_factors_consistent_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    L.lins_last_team_pcm_stats.argtypes = [C.c_void_p] * 2
    L.lins_debug_team_pcm_clique.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    L.lins_debug_team_pcm_clique.restype = C.c_int
    prm = defs.team_pcm_params(L)
    for n in (0, 1):  # a NULL context is refused before n is looked at
        assert L.lins_team_factors_consistent_batch(None, n, None, None, None, None, C.byref(prm), None) == E_ARG
        assert L.lins_debug_team_pcm_clique(None, n, None, None, C.byref(prm), None) == E_ARG
    assert L.lins_last_team_pcm_stats(None, None) == E_ARG
    L.lins_team_pcm_default_params(None)  # (a NULL is ignored, as the other default calls ignore it)
