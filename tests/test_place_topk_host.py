"""lins_host_place_topk (csrc/host/place.cpp, the definition lins_place_topk_batch is held to) against the independent
numpy statement of tests/place_topk_cases.py — sort the row keys formed from host.place_distance, then one greedy pass
with the separation rule — and lins_host_loop_choose (csrc/host/loop_step.h) on its edges."""
import numpy as np
import pytest

import place_topk_cases as tk

host = tk.host
E_ARG, E_INPUT = -1, -4


def counts_for(k):
    return sorted({0, 1, 2, max(k - 1, 0), k, k + 1, 200})


@pytest.mark.parametrize("k", [1, 2, 8])
def test_topk_is_the_sorted_greedy_selection(k):
    for n in counts_for(k):
        times = np.arange(n, dtype=np.float64)
        for which in (0, 1):
            keys = tk.row_keys(which, n, times, 1e6, -1.0)
            assert len(keys) == n
            for sep in sorted({0, 1, 4, n}):
                want = tk.select(keys, k, sep)
                got, cand = host.place_topk(tk.query_desc(which), tk.descs(n), times, 1e6, -1.0, k, sep)
                assert cand == n and tk.as_keys(got) == want, (k, n, which, sep, tk.as_keys(got), want)
                if sep >= n:
                    assert len(got) == min(n, 1)
                if sep == 0:
                    assert len(got) == min(n, k)


def test_duplicates_go_by_the_lower_id_then_by_the_separation():
    """query 1 is frame 5 of the pool bit for bit, and so are frames 5 + 74 and 5 + 111: three candidates at d = 0"""
    n = 200
    times = np.arange(n, dtype=np.float64)
    got, _ = host.place_topk(tk.query_desc(1), tk.descs(n), times, 1e6, -1.0, 8, 0)
    assert [r["id"] for r in got[:3]] == [5, 79, 116] and all(r["distance"] == 0 and r["shift"] == 0 for r in got[:3])
    got, _ = host.place_topk(tk.query_desc(1), tk.descs(n), times, 1e6, -1.0, 8, 74)  # 79 lies within 74 of 5, 116 does not
    assert [r["id"] for r in got[:2]] == [5, 116]
    assert tk.as_keys(got) == tk.select(tk.row_keys(1, n, times, 1e6, -1.0), 8, 74)
    # the query itself skipped: the next duplicate leads
    got, cand = host.place_topk(tk.query_desc(1), tk.descs(n), times, 1e6, -1.0, 2, 0, skip_id=5)
    assert [r["id"] for r in got] == [79, 116] and cand == n - 1


def test_no_admissible_candidate_and_the_unfilled_ranks():
    n = 20
    times = np.arange(n, dtype=np.float64)
    got, cand = host.place_topk(tk.query_desc(0), tk.descs(n), times, 10.0, 100.0, 8, 0)
    assert got == [] and cand == 0
    raw, _ = host.place_topk(tk.query_desc(0), tk.descs(n), times, 10.0, 100.0, 8, 0, raw=True)
    assert [(r["id"], r["shift"], float(r["distance"])) for r in raw] == [(-1, 0, 1.0)] * 8
    # seven admissible (times 0 .. 3 and 17 .. 19 lie more than 6.5 from 10): the gate is find_loop's
    keys = tk.row_keys(0, n, times, 10.0, 6.5)
    assert sorted(c for _, c, _ in keys) == [0, 1, 2, 3, 17, 18, 19]
    raw, cand = host.place_topk(tk.query_desc(0), tk.descs(n), times, 10.0, 6.5, 8, 0, raw=True)
    assert cand == 7 and tk.as_keys(raw[:7]) == tk.select(keys, 8, 0) and (raw[7]["id"], raw[7]["shift"], float(raw[7]["distance"])) == (-1, 0, 1.0)
    # an empty query frame: every distance is 1, the ranks go by id
    got, _ = host.place_topk(tk.query_desc(2), tk.descs(n), times, 1e6, -1.0, 3, 1)
    assert [(r["id"], r["shift"], float(r["distance"])) for r in got] == [(0, 0, 1.0), (2, 0, 1.0), (4, 0, 1.0)]


@pytest.mark.parametrize("n", [0, 1, 2, 45])
def test_k1_is_the_search_field_for_field(n):
    times = np.arange(n, dtype=np.float64)
    for which in (0, 1, 2):
        for now, gap, skip in ((1e6, -1.0, -1), (float(n), 3.0, n - 1), (2.0, 1.0, 0)):
            s = host.place_search(tk.query_desc(which), tk.descs(n), times, now, gap, skip)
            for sep in (0, 4, 1000):
                raw, cand = host.place_topk(tk.query_desc(which), tk.descs(n), times, now, gap, 1, sep, skip_id=skip, raw=True)
                assert (raw[0]["id"], raw[0]["shift"], tk.bits(raw[0]["distance"]), cand) == (s["id"], s["shift"], tk.bits(s["distance"]), s["candidates"])
                top, _ = host.place_topk(tk.query_desc(which), tk.descs(n), times, now, gap, 8, sep, skip_id=skip, raw=True)
                assert tk.as_keys(top[:1]) == tk.as_keys(raw)  # rank 0 is the search's answer for every min_sep and k


def test_refusals():
    D, t = tk.descs(3), np.arange(3.0)
    for k, sep in ((0, 0), (9, 0), (-1, 0), (4, -1)):
        assert host.place_topk(tk.query_desc(0), D, t, 10.0, -1.0, k, sep) == E_ARG
    assert host.place_topk(tk.query_desc(0), D, t, float("inf"), -1.0, 4, 0) == E_INPUT
    assert host.place_topk(tk.query_desc(0), D, t, 10.0, float("nan"), 4, 0) == E_INPUT


def test_loop_choose():
    # the smallest accepted fitness; ties go to the lower rank
    assert host.loop_choose([1, 1, 1], [0.2, 0.05, 0.1]) == 1
    assert host.loop_choose([1, 1, 1, 1], [0.2, 0.05, 0.05, 0.1]) == 1
    assert host.loop_choose([1, 1], [0.1, 0.1]) == 0
    # all rejected: not converged, or above the bar (the bar itself passes: LM:1140 rejects fitness > bar)
    assert host.loop_choose([0, 0], [0.01, 0.02]) == -1
    assert host.loop_choose([1, 1], [0.31, 0.5]) == -1
    assert host.loop_choose([1], [float(np.float32(0.3))]) == 0
    assert host.loop_choose([1, 1], [1.7976931348623157e308, 0.4]) == -1
    # the best fit did not converge: the best of those that did
    assert host.loop_choose([0, 1, 1], [0.001, 0.25, 0.2]) == 2
    # a bar of its own
    assert host.loop_choose([1, 1], [0.4, 0.6], max_fitness=0.5) == 0
    # k = 0
    assert host.loop_choose([], []) == -1
    # every accepted rank agrees with lins_host_loop_accept
    for conv, fit in (([1, 0, 1], [0.29, 0.1, 0.31]), ([1, 1, 1], [0.5, 0.4, 0.3])):
        c = host.loop_choose(conv, fit)
        ok = [j for j in range(3) if host.loop_accept(conv[j], fit[j])]
        assert (c == -1 and not ok) or (c in ok and all(fit[c] <= fit[j] for j in ok))
