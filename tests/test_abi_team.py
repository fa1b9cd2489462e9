"""include/lins_team.h: the prototypes compile as C99, the ctypes mirrors have the C structs' sizes and offsets, both
libraries export their calls, and the calls that need no device keep the conventions (a NULL context is LINS_E_ARG)."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("lins_place_team_default_params", "lins_place_team_topk_batch", "lins_place_team_key", "lins_place_team_set_chunk",
         "lins_last_place_team_stats", "lins_rendezvous_default_params", "lins_rendezvous_step", "lins_pose_graph_rebase_batch",
         "lins_team_rebase")
HOST_CALLS = ("lins_place_team_default_params", "lins_host_place_team_topk", "lins_host_place_ring_key", "lins_host_place_team_guess",
              "lins_host_pose_graph_rebase")
E_ARG = -1


def test_prototypes_and_layouts_match_the_c_header(defs):
    protos = r"""
#include "lins_team.h"
int (*a)(lins_ctx*, int, const lins_place_team_query*, int, const int32_t*, const lins_place_team_params*, lins_place_team_result*, int32_t*) = lins_place_team_topk_batch;
int (*b)(lins_ctx*, int, int, uint8_t*, uint32_t*, double*) = lins_place_team_key;
int (*c)(lins_ctx*, int) = lins_place_team_set_chunk;
int (*d)(lins_ctx*, float*, float*, float*, int32_t*, uint64_t*) = lins_last_place_team_stats;
int (*e)(lins_ctx*, int, const lins_rendezvous_entry*, int, const int32_t*, const lins_loop_step_params*, const lins_rendezvous_params*, lins_rendezvous_result*) = lins_rendezvous_step;
int (*f)(const float*, int, int, double, double, int, const int32_t*, const float* const*, const double* const*, const int32_t*, const lins_place_team_params*, lins_place_team_result*) = lins_host_place_team_topk;
int (*g)(const float*, uint8_t*, uint32_t*) = lins_host_place_ring_key;
int (*h)(const lins_key_pose*, const lins_key_pose*, int, int, double*) = lins_host_place_team_guess;
void (*i)(lins_place_team_params*) = lins_place_team_default_params;
void (*j)(lins_rendezvous_params*) = lins_rendezvous_default_params;
int (*k)(lins_ctx*, int, const int32_t*, const double*) = lins_pose_graph_rebase_batch;
int (*l)(lins_ctx*, int, const int32_t*, const int32_t*, const double*) = lins_team_rebase;
int (*m)(lins_host_pose_graph*, const double*) = lins_host_pose_graph_rebase;
"""
    layout = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_team.h"
#define S(t) printf("%zu ", sizeof(t))
#define O(t, f) printf("%zu ", offsetof(t, f))
int main(void) {
  S(lins_place_team_params); O(lins_place_team_params, min_sep);
  S(lins_place_team_query); O(lins_place_team_query, now); O(lins_place_team_query, min_gap_s);
  S(lins_place_team_result); O(lins_place_team_result, distance); O(lins_place_team_result, dk); O(lins_place_team_result, status);
  S(lins_rendezvous_entry); O(lins_rendezvous_entry, now);
  S(lins_rendezvous_params); O(lins_rendezvous_params, max_distance);
  S(lins_rendezvous_result); O(lins_rendezvous_result, latest); O(lins_rendezvous_result, cand); O(lins_rendezvous_result, target);
  O(lins_rendezvous_result, icp); O(lins_rendezvous_result, X);
  printf("%d %d %d %d %d\n", LINS_PLACE_MAX_SHORTLIST, LINS_PLACE_MAX_TEAM_SLOTS, LINS_RENDEZVOUS_NONE, LINS_RENDEZVOUS_REJECTED, LINS_RENDEZVOUS_FOUND);
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
    P, Q, R, E, RP, RR = (defs.PlaceTeamParamsC, defs.PlaceTeamQueryC, defs.PlaceTeamResultC, defs.RendezvousEntryC, defs.RendezvousParamsC,
                          defs.RendezvousResultC)
    want = [sz(P), P.min_sep.offset, sz(Q), Q.now.offset, Q.min_gap_s.offset, sz(R), R.distance.offset, R.dk.offset, R.status.offset,
            sz(E), E.now.offset, sz(RP), RP.max_distance.offset, sz(RR), RR.latest.offset, RR.cand.offset, RR.target.offset, RR.icp.offset,
            RR.X.offset, defs.PLACE_MAX_SHORTLIST, defs.PLACE_MAX_TEAM_SLOTS, defs.RENDEZVOUS_NONE, defs.RENDEZVOUS_REJECTED, defs.RENDEZVOUS_FOUND]
    assert got == want
    assert (sz(P), sz(Q), sz(R), sz(E)) == (16, 24, 32, 16)


def test_both_libraries_export_the_calls(host, ieskf):
    assert sorted(ieskf.TEAM_EXPORTS) == sorted(CALLS)
    assert not set(CALLS) & set(ieskf.EXPORTS) and not set(CALLS) & set(ieskf.PLACE_EXPORTS)
    for name in CALLS:
        assert hasattr(ieskf.lib(), name), name
    for name in HOST_CALLS:
        assert hasattr(host.lib(), name), name


def test_conventions_without_a_device(ieskf, defs):
    L = ieskf.lib()
    L.lins_place_team_topk_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 2 + [C.c_void_p] * 4
    L.lins_place_team_topk_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lins_rendezvous_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lins_place_team_set_chunk.argtypes = [C.c_void_p, C.c_int]
    L.lins_last_place_team_stats.argtypes = [C.c_void_p] * 6
    L.lins_place_team_key.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    for n in (0, 1):  # a NULL context is refused before n is looked at
        assert L.lins_place_team_topk_batch(None, n, None, 0, None, None, None, None) == E_ARG
        assert L.lins_rendezvous_step(None, n, None, 0, None, None, None, None) == E_ARG
    assert L.lins_place_team_set_chunk(None, 0) == E_ARG and L.lins_last_place_team_stats(None, None, None, None, None, None) == E_ARG
    assert L.lins_place_team_key(None, 0, 0, None, None, None) == E_ARG
    L.lins_pose_graph_rebase_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.lins_team_rebase.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    for n in (0, 1):
        assert L.lins_pose_graph_rebase_batch(None, n, None, None) == E_ARG and L.lins_team_rebase(None, n, None, None, None) == E_ARG
    p, r = defs.place_team_params(L), defs.rendezvous_params(L)
    assert (p.shortlist, p.k, p.min_sep) == (32, 4, 0)
    assert (r.team.shortlist, r.team.k, r.team.min_sep, r.max_distance) == (32, 4, -1, 1.0)
