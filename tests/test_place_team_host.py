"""lins_host_place_team_topk (include/lins_host.h; the definition of include/lins_team.h's team search) against the
independent numpy statement of tests/team_cases.py: ring key from D, integer key distance, admissibility, the packed
order of the shortlist, the row keys' order and the conflict rule.  The slots are cut from the top-K tests' pool, whose
laps 0, 2 and 3 are exact duplicates: slot 0 and slot 2 hold the same frames, so ties on dk AND on d occur and the
order (dk, slot, id) decides them.  Also the scalar functions under the sanitizers, as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import place_topk_cases as tk
import team_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lins---lidar-inertial-slam_amd", "csrc")
team = tc.team
E_ARG, E_INPUT = -1, -4


def slots():
    """slot 0: pool frames 0 .. 29; slot 2: frames 74 .. 103 — lap 2, bit for bit frames 0 .. 29; slot 5: the revisits 37 ..
    56; slot 7: no frame; slot 9: frames 3 .. 5"""
    return [(0,) + tc.pool_slot(0, 30), (2,) + tc.pool_slot(74, 30), (5,) + tc.pool_slot(37, 20), (7,) + tc.pool_slot(0, 0),
            (9,) + tc.pool_slot(3, 3)]


def query(which):
    return tc.register(("query", which), tk.query_desc(which))


def check(name_q, qs, qid, now, gap, targets, M, k, sep):
    got = tc.host_got(name_q, qs, qid, now, gap, targets, M, k, sep)
    want = tc.want(name_q, qs, qid, now, gap, targets, M, k, sep)
    assert got == want, (qs, qid, now, gap, M, k, sep, got, want)
    return got


def test_ring_key_is_a_count_and_does_not_turn():
    for i in (0, 5, 37, 80):
        occ, sq = team.host_ring_key(tk.desc(i))
        want, want_sq = tc.ring_key(tk.desc(i))
        assert occ.tolist() == want.tolist() and sq == want_sq and occ.max() <= 60
        # the same place turned by 13 sectors: the columns move, the rings' counts do not
        assert team.host_ring_key(np.roll(tk.desc(i), 13, axis=1))[0].tolist() == want.tolist()
    assert team.host_ring_key(np.zeros((20, 60), np.float32)) [1] == 0
    occ, sq = team.host_ring_key(np.ones((20, 60), np.float32))
    assert occ.tolist() == [60] * 20 and sq == 72000


@pytest.mark.parametrize("M", (1, 4, 32, 64))
def test_the_restatement_is_the_contract(M):
    tg = slots()
    for which in (0, 1, 2):  # a revisit; a frame of the pool bit for bit (dk = 0, d = 0 in two slots); an empty frame
        for k, sep in ((1, 0), (4, 0), (8, 2), (8, 40)):
            for order in (tg, tg[::-1]):
                check(query(which), 11, 0, 1e6, -1.0, order, M, k, sep)
    # duplicated frames in two slots: query 1 is pool frame 5 = slot 0's frame 5 = slot 2's frame 5 = slot 9's frame 2
    got, cand = check(query(1), 11, 0, 1e6, -1.0, tg, 8, 4, 0)
    if M >= 4:
        assert [x[:2] for x in got[:3]] == [(0, 5), (2, 5), (9, 2)] and all(x[3] == 0 and x[4] == 0 for x in got[:3]) and cand == 83


def test_the_querys_own_slot_is_gated_by_time_and_other_slots_are_not():
    tg = slots()
    names0 = tg[0][1]
    # frame 20 of slot 0 asks at now = 20 with a gap of 3: ids 17 and 23 sit AT equality and are out, 16 and 24 are in;
    # slot 2's frames of the same seconds are all in — and its frame 20 is the query bit for bit
    got, cand = check(names0[20], 0, 20, 20.0, 3.0, tg, 64, 8, 0)
    assert cand == (30 - 7) + 30 + 20 + 3
    assert got[0][:2] == (2, 20) and got[0][3] == 0
    assert not any(s == 0 and 17 <= c <= 23 for s, c, *_ in got)
    # a negative gap admits every time, never the query itself
    got, cand = check(names0[20], 0, 20, 20.0, -1.0, tg, 64, 8, 0)
    assert cand == 29 + 53 and (0, 20) not in [x[:2] for x in got]
    # the same frame asked from a slot that is not in the list: its twin in slot 0 is admissible
    got, cand = check(names0[20], 11, 20, 20.0, 3.0, tg, 64, 2, 0)
    assert cand == 83 and [x[:2] for x in got] == [(0, 20), (2, 20)]


def test_short_lists_few_ranks_and_empty_slots():
    tg = slots()
    # M larger than the admissible count: slot 9 alone has three frames
    got, cand = check(query(0), 11, 0, 1e6, -1.0, [tg[4]], 64, 8, 0)
    assert cand == 3 and sum(x != tc.UNFILLED for x in got) == 3
    # k larger than the ranks that exist: a separation as wide as the slot leaves one rank a slot
    got, cand = check(query(0), 11, 0, 1e6, -1.0, tg, 64, 8, 1000)
    assert sum(x != tc.UNFILLED for x in got) == 4 and len({x[0] for x in got[:4]}) == 4
    # M = 1: one rank whatever k is
    got, cand = check(query(0), 11, 0, 1e6, -1.0, tg, 1, 8, 0)
    assert sum(x != tc.UNFILLED for x in got) == 1 and cand == 83
    # an empty target slot, alone and among others; no target at all
    for targets in ([tg[3]], []):
        got, cand = check(query(0), 11, 0, 1e6, -1.0, targets, 32, 4, 0)
        assert cand == 0 and got == [tc.UNFILLED] * 4
    assert check(query(0), 11, 0, 1e6, -1.0, [tg[3], tg[4]], 32, 4, 0) == check(query(0), 11, 0, 1e6, -1.0, [tg[4]], 32, 4, 0)


def test_refusals():
    tg = [(s, [tc._DESCS[n] for n in names], t) for s, names, t in slots()]
    q = tk.query_desc(0)
    assert isinstance(team.host_topk(q, 11, 0, 1e6, -1.0, tg), list)
    for kw in (dict(shortlist=0), dict(shortlist=65), dict(k=0), dict(k=9), dict(min_sep=-1)):
        assert team.host_topk(q, 11, 0, 1e6, -1.0, tg, **kw) == E_ARG, kw
    assert team.host_topk(q, 11, 0, 1e6, -1.0, tg + [tg[0]]) == E_ARG  # a slot twice
    assert team.host_topk(q, 65536, 0, 1e6, -1.0, tg) == E_ARG and team.host_topk(q, -1, 0, 1e6, -1.0, tg) == E_ARG
    assert team.host_topk(q, 11, 0, 1e6, -1.0, [(65536,) + tg[0][1:]]) == E_ARG
    assert team.host_topk(q, 11, 0, float("inf"), -1.0, tg) == E_INPUT and team.host_topk(q, 11, 0, 1e6, float("nan"), tg) == E_INPUT
    p = team.params()
    assert (p.shortlist, p.k, p.min_sep) == (32, 4, 0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("team") / "team_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover", "-I", CSRC, os.path.join(ROOT, "tests", "native", "team_check.cpp"),
                           os.path.join(CSRC, "host", "place.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("name", ("keys", "select", "search", "layout_b", "layout_c"))
def test_the_scalar_text_under_the_sanitizers(exe, name):
    """tests/native/team_check.cpp: ring_key / key_distance / pack_team_key on random descriptors, select_team on 200
    random key sets against a sort, lins_host_place_team_topk on random small teams, on a shortlist whose cut at position
    M decides rank 0 (622 candidates) and on frames at the ends of the key's range"""
    run = subprocess.run([exe, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()
    assert run.stdout.decode() == "ok %s\n" % name
    assert run.stderr == b""


def test_an_unknown_case_is_refused(exe):
    assert subprocess.run([exe, "nothing"], stdout=subprocess.DEVNULL).returncode == 2
