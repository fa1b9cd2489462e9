"""What the loop thread decides between its device stages (csrc/host/loop_step.h, exported as lins_host_loop_*): the
window of LM:1087-1098, the candidate rule with the project's two departures (a frame is no loop with itself; a pair equal
to the slot's most recent loop factor is a repeat), the acceptance of LM:1140-1141 with the f32 threshold promoted as the
reference's comparison promotes it, and the variance of LM:1171-1175.  lins_loop_step compiles the same text."""
import numpy as np
import pytest

DBL_MAX = np.finfo(np.float64).max
NONE, REPEAT, ALIGN = 0, 1, -1


@pytest.mark.parametrize("latest, closest, H, want", [
    (11, 4, 4, range(0, 9)),
    (11, 1, 4, range(0, 6)),
    (11, 10, 4, range(6, 12)),  # contains the latest frame, as in the reference
    (11, 4, 25, range(0, 12)),  # H = 25 with 12 frames
    (11, 4, 0, [4]),
    (0, 0, 4, [0]),             # latest = 0
    (0, 0, 0, [0]),
    (-1, -1, 4, []),            # no frames
    (11, -1, 4, []),            # no candidate
    (11, 12, 4, []),            # not a frame
    (11, 4, -1, []),
    (2 ** 31 - 1, 2 ** 31 - 2, 2 ** 31 - 1, None),  # closest + H beyond an int
])
def test_window(host, latest, closest, H, want):
    if want is None:  # the arithmetic is done wide: the count, through a buffer too small for it (LINS_E_CAPACITY)
        import ctypes as C
        L = host.lib()
        L.lins_host_loop_window.argtypes, L.lins_host_loop_window.restype = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int], C.c_int
        assert L.lins_host_loop_window(latest, closest, H, None, 0) == -3
        assert L.lins_host_loop_window(latest, closest, 1, None, 1) == -3  # 3 ids: closest - 1 .. latest
        return
    assert host.loop_window(latest, closest, H) == list(want)


def test_candidate_self_and_repeat(host, defs):
    assert (defs.LOOP_NONE, defs.LOOP_REPEAT) == (NONE, REPEAT)
    assert host.loop_candidate(11, 4) == ALIGN
    assert host.loop_candidate(11, 0) == ALIGN
    assert host.loop_candidate(11, -1) == NONE            # detectLoopClosure found nothing
    assert host.loop_candidate(-1, -1) == NONE            # no frames
    assert host.loop_candidate(11, 11) == NONE            # the latest frame itself: a departure from the reference
    assert host.loop_candidate(0, 0) == NONE
    assert host.loop_candidate(11, 4, 11, 4) == REPEAT    # the pair of the slot's most recent loop factor: a departure
    assert host.loop_candidate(12, 4, 11, 4) == ALIGN     # a new key frame arrived
    assert host.loop_candidate(11, 5, 11, 4) == ALIGN     # another candidate of the same frame
    assert host.loop_candidate(11, 4, 4, 11) == ALIGN     # (the pair is ordered)
    assert host.loop_candidate(11, 11, 11, 11) == NONE    # self before repeat


def test_accept_is_the_references_expression(host):
    edge = float(np.float32(0.3))  # (double)0.3f = 0.300000011920928955078125
    assert edge > 0.3
    assert host.loop_accept(1, edge)
    assert not host.loop_accept(1, np.nextafter(edge, 1.0))  # one ulp above
    assert host.loop_accept(1, 0.3) and host.loop_accept(1, np.nextafter(edge, 0.0)) and host.loop_accept(1, 0.0)
    assert not host.loop_accept(0, 0.0) and not host.loop_accept(0, edge)  # not converged
    assert not host.loop_accept(1, DBL_MAX)  # no source point found a target
    assert not host.loop_accept(1, np.inf)
    # max_fitness is rounded to f32 first, whatever double the caller wrote
    assert host.loop_accept(1, edge, max_fitness=0.3) and host.loop_accept(1, float(np.float32(0.5)), max_fitness=0.5)
    assert not host.loop_accept(1, 1e-300, max_fitness=0.0) and host.loop_accept(1, 0.0, max_fitness=0.0)


def decision(host, converged, fitness, max_fitness=0.3):
    """what lins_loop_step does with an alignment: accepted, and a usable variance"""
    return host.loop_accept(converged, fitness, max_fitness) and host.loop_variance(fitness)[0]


def test_variance_and_the_whole_decision(host):
    ok, v = host.loop_variance(0.25)
    assert ok and v == float(np.float32(0.25))
    ok, v = host.loop_variance(0.1)
    assert ok and v == float(np.float32(0.1)) != 0.1  # (double)(float)fitness
    assert host.loop_variance(1e-60) == (False, 0.0)  # rounds to 0 in f32: lins_pose_graph_add_loop would refuse it
    assert host.loop_variance(0.0) == (False, 0.0)
    assert not host.loop_variance(-0.1)[0]
    assert not host.loop_variance(DBL_MAX)[0] and not host.loop_variance(np.inf)[0]  # (float)DBL_MAX = inf
    ok, v = host.loop_variance(np.nan)
    assert not ok and np.isnan(v)
    tiny = float(np.finfo(np.float32).smallest_subnormal)
    assert host.loop_variance(tiny) == (True, tiny)
    # NaN passes the reference's comparison (NaN > x is false) and is stopped by the variance: rejected as a whole
    assert host.loop_accept(1, np.nan) and not decision(host, 1, np.nan)
    assert not decision(host, 0, 0.1) and not decision(host, 1, DBL_MAX) and not decision(host, 1, 1e-60)
    assert decision(host, 1, float(np.float32(0.3))) and not decision(host, 1, np.nextafter(float(np.float32(0.3)), 1.0))
