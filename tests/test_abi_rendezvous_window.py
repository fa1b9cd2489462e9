"""Rendezvous over a window (include/lins_team.h, the consensus records of include/lins_host.h): the prototypes compile as
C99, the ctypes mirrors have the C structs' sizes and offsets, the defaults are the documented ones in both libraries,
both libraries export their calls, and the calls that need no device keep the conventions."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("lins_rendezvous_consensus_default_params", "lins_rendezvous_consensus_batch", "lins_last_rendezvous_consensus_stats",
         "lins_rendezvous_window_step", "lins_last_rendezvous_window_stats")
HOST_CALLS = ("lins_rendezvous_consensus_default_params", "lins_host_rendezvous_consensus")
E_ARG = -1


def test_prototypes_and_layouts_match_the_c_header(defs):
    protos = r"""
#include "lins_team.h"
int (*a)(lins_ctx*, int, const lins_consensus_hyp*, const int32_t*, const lins_consensus_params*, lins_consensus_result*) = lins_rendezvous_consensus_batch;
int (*b)(lins_ctx*, float*) = lins_last_rendezvous_consensus_stats;
int (*c)(lins_ctx*, int, const lins_rendezvous_entry*, int, const int32_t*, const lins_loop_step_params*, const lins_rendezvous_params*,
         const lins_consensus_params*, lins_rendezvous_window_result*, lins_rendezvous_hypothesis*) = lins_rendezvous_window_step;
int (*d)(lins_ctx*, float*, float*, float*, float*, float*) = lins_last_rendezvous_window_stats;
int (*e)(const lins_consensus_hyp*, int, const lins_consensus_params*, lins_consensus_result*) = lins_host_rendezvous_consensus;
void (*f)(lins_consensus_params*) = lins_rendezvous_consensus_default_params;
"""
    layout = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_team.h"
#define S(t) printf("%zu ", sizeof(t))
#define O(t, f) printf("%zu ", offsetof(t, f))
int main(void) {
  S(lins_consensus_hyp); O(lins_consensus_hyp, p); O(lins_consensus_hyp, fitness); O(lins_consensus_hyp, query); O(lins_consensus_hyp, rank);
  O(lins_consensus_hyp, target_slot); O(lins_consensus_hyp, admissible);
  S(lins_consensus_params); O(lins_consensus_params, stride); O(lins_consensus_params, min_support); O(lins_consensus_params, max_translation);
  O(lins_consensus_params, min_cos_rotation);
  S(lins_consensus_result); O(lins_consensus_result, support); O(lins_consensus_result, n_admissible); O(lins_consensus_result, members);
  S(lins_rendezvous_hypothesis); O(lins_rendezvous_hypothesis, rank); O(lins_rendezvous_hypothesis, admissible); O(lins_rendezvous_hypothesis, member);
  O(lins_rendezvous_hypothesis, cand); O(lins_rendezvous_hypothesis, target); O(lins_rendezvous_hypothesis, icp);
  S(lins_rendezvous_window_result); O(lins_rendezvous_window_result, n_queries); O(lins_rendezvous_window_result, n_hypotheses);
  O(lins_rendezvous_window_result, winner); O(lins_rendezvous_window_result, support); O(lins_rendezvous_window_result, n_admissible);
  O(lins_rendezvous_window_result, target_slot); O(lins_rendezvous_window_result, target_id); O(lins_rendezvous_window_result, members);
  O(lins_rendezvous_window_result, query_id); O(lins_rendezvous_window_result, n_ranks); O(lins_rendezvous_window_result, source);
  O(lins_rendezvous_window_result, X);
  printf("%d %d %d %d %d %d %d\n", LINS_RENDEZVOUS_MAX_WINDOW, LINS_RENDEZVOUS_MAX_HYP, LINS_RENDEZVOUS_NONE, LINS_RENDEZVOUS_REJECTED,
         LINS_RENDEZVOUS_FOUND, LINS_RENDEZVOUS_UNCONFIRMED, LINS_PLACE_MAX_K);
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
    H, P, R, RH, RW = defs.ConsensusHypC, defs.ConsensusParamsC, defs.ConsensusResultC, defs.RendezvousHypothesisC, defs.RendezvousWindowResultC
    want = [sz(H), H.p.offset, H.fitness.offset, H.query.offset, H.rank.offset, H.target_slot.offset, H.admissible.offset,
            sz(P), P.stride.offset, P.min_support.offset, P.max_translation.offset, P.min_cos_rotation.offset,
            sz(R), R.support.offset, R.n_admissible.offset, R.members.offset,
            sz(RH), RH.rank.offset, RH.admissible.offset, RH.member.offset, RH.cand.offset, RH.target.offset, RH.icp.offset,
            sz(RW), RW.n_queries.offset, RW.n_hypotheses.offset, RW.winner.offset, RW.support.offset, RW.n_admissible.offset, RW.target_slot.offset,
            RW.target_id.offset, RW.members.offset, RW.query_id.offset, RW.n_ranks.offset, RW.source.offset, RW.X.offset,
            defs.RENDEZVOUS_MAX_WINDOW, defs.RENDEZVOUS_MAX_HYP, defs.RENDEZVOUS_NONE, defs.RENDEZVOUS_REJECTED, defs.RENDEZVOUS_FOUND,
            defs.RENDEZVOUS_UNCONFIRMED, defs.PLACE_MAX_K]
    assert got == want
    # the kernel's view of a hypothesis: 20 doubles and four integers; a result is two 16-byte stores
    assert (sz(H), H.query.offset, sz(P), sz(R)) == (176, 160, 32, 32)
    assert defs.RENDEZVOUS_MAX_HYP == defs.RENDEZVOUS_MAX_WINDOW * defs.PLACE_MAX_K == 128 and defs.RENDEZVOUS_UNCONFIRMED == 3


def test_both_libraries_export_the_calls_and_agree_on_the_defaults(host, ieskf, defs):
    for name in CALLS:
        assert name in ieskf.EXPORTS and hasattr(ieskf.lib(), name), name
    for name in HOST_CALLS:
        assert hasattr(host.lib(), name), name
    assert not set(CALLS) & set(ieskf.TEAM_EXPORTS)  # (that list is lins_rendezvous_step's generation of the header, pinned by tests/test_abi_team.py)
    for L in (host.lib(), ieskf.lib()):
        p = defs.consensus_params(L)
        assert (p.window, p.stride, p.min_support, p.reserved, p.max_translation) == (5, 1, 3, 0, 1.0)
        assert p.min_cos_rotation == 0.99619469809174555  # cos 5 degrees, the literal
        assert defs.consensus_params(L, window=8, max_translation=0.5).window == 8


def test_conventions_without_a_device(ieskf, defs):
    L = ieskf.lib()
    L.lins_rendezvous_consensus_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    L.lins_rendezvous_window_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    L.lins_last_rendezvous_consensus_stats.argtypes = [C.c_void_p] * 2
    L.lins_last_rendezvous_window_stats.argtypes = [C.c_void_p] * 6
    prm = defs.consensus_params(L)
    for n in (0, 1):  # a NULL context is refused before n is looked at
        assert L.lins_rendezvous_consensus_batch(None, n, None, None, C.byref(prm), None) == E_ARG
        assert L.lins_rendezvous_window_step(None, n, None, 0, None, None, None, None, None, None) == E_ARG
    assert L.lins_last_rendezvous_consensus_stats(None, None) == E_ARG
    assert L.lins_last_rendezvous_window_stats(None, None, None, None, None, None) == E_ARG
    L.lins_rendezvous_consensus_default_params(None)  # (a NULL is ignored, as the other default calls ignore it)
