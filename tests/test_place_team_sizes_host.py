"""lins_host_place_team_topk (the definition of include/lins_team.h's team search) against the numpy statement of
tests/team_cases.py on the layouts of tests/team_sizes_cases.py — 622 candidates over slots with none, one, 64, 257 and 300
frames; the crafted shortlist whose cut at position M decides rank 0; frames at the ends of the key's range; 300 target
slots with slot numbers above 255 — for every shortlist length at the edges of the pair kernel's passes of ten.  This
anchors the reference tests/test_gpu_place_team_sizes.py holds the device to."""
import numpy as np
import pytest

import place_topk_cases as tk
import team_cases as tc
import team_sizes_cases as ts

team = tc.team
CASES = {"A": ("A", ts.A_ALL, ts.A_QUERIES), "C": ("A", list(ts.C_SLOTS), ts.C_QUERIES), "D": ("D", ts.D_ALL, ts.D_QUERIES)}


def test_the_layouts_hold_what_they_were_built_for():
    d_near, d_nearer = ts.crafted()
    assert d_nearer < d_near < tk.bits(1e-3)


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("k", ts.KS)
def test_the_definition_is_the_numpy_statement(case, k):
    layout, slots, queries = CASES[case]
    for q in queries:
        for M in ts.MS:
            for sep in ts.SEPS:
                got, want = ts.host_got(layout, q, slots, M, k, sep), ts.want(layout, q, slots, M, k, sep)
                assert got == want, (case, q, M, k, sep, got, want)
                assert sum(x != tc.UNFILLED for x in got[0]) <= min(M, k)


def test_the_target_lists_shape_does_not_matter():
    for q in ts.A_QUERIES:
        base = ts.want("A", q, ts.A_ALL, 11, 8, 2)
        for order in (ts.A_ALL[::-1], [4, 0, 6, 2, 5, 1, 3]):
            assert ts.host_got("A", q, order, 11, 8, 2) == base, (q, order)
        # empties in front, behind, and nothing but empties
        assert ts.host_got("A", q, [1, 3, 2], 11, 8, 2) == ts.want("A", q, [2], 11, 8, 2)
        assert ts.host_got("A", q, [2, 6], 11, 8, 2) == ts.want("A", q, [2], 11, 8, 2)
        assert ts.host_got("A", q, [1, 3, 6], 11, 8, 2) == ([tc.UNFILLED] * 8, 0)
    for q in ts.D_QUERIES:
        base = ts.want("D", q, ts.D_ALL, 21, 8, 0)
        for order in (ts.D_SHUFFLED, ts.D_ENDS_EMPTY):
            assert ts.host_got("D", q, order, 21, 8, 0) == base, q
        assert ts.host_got("D", q, ts.D_PAIR, 21, 8, 0) == ts.want("D", q, ts.D_PAIR, 21, 8, 0)
    # the admissible counts: the gate of the query inside slot 2 takes out ids 250 .. 262, the one inside slot 4 itself
    assert [ts.want("A", q, ts.A_ALL, 1, 1, 0)[1] for q in ts.A_QUERIES] == [622] * 5 + [622 - 13, 621]
    assert [ts.want("D", q, ts.D_ALL, 1, 1, 0)[1] for q in ts.D_QUERIES] == [450] * 3 + [448]


def test_the_whole_shortlist_shows_through_eight_ranks():
    """k = 8 and no separation return every member of a shortlist of M <= 8: sorted by (dk, slot, id) they are the first M
    tuples of the numpy sort"""
    for layout, slots, queries in CASES.values():
        for q in queries:
            order = ts.ranked(layout, q, tuple(sorted(slots)))
            for M in range(1, 9):
                got, cand = ts.host_got(layout, q, slots, M, 8, 0)
                assert ts.shortlisted(got) == order[:M] and cand == len(order), (layout, q, M)
    # the candidate whose shortlist key is 0 leads, and the rest behind it is right
    got, _ = ts.host_got("A", ts.A_QUERIES[0], ts.A_ALL, 8, 8, 0)
    assert got[0] == (0, 0, 0, 0, 0) and len(ts.shortlisted(got)) == 8


def test_the_cut_of_the_shortlist_decides_rank_0():
    d_near, d_nearer = ts.crafted()
    at64, _ = ts.host_got("A", ts.Q_B, ts.A_ALL, 64, 8, 0)
    assert at64[0] == ts.NEAR + (0, d_near, 1)
    assert all(r[:2] != ts.NEARER for r in at64) and all(r[:2] in ts.SAME for r in at64[1:])
    at63, _ = ts.host_got("A", ts.Q_B, ts.A_ALL, 63, 8, 0)
    assert all(r[:2] in ts.SAME for r in at63)  # (near is not among them)
    assert d_nearer < d_near  # nearer would lead if the shortlist admitted it


def test_keys_at_the_ends_of_their_range():
    cs = ts.layout_a()[ts.C_SLOTS[0]]
    for nm in cs:
        occ, sq = team.host_ring_key(tc._DESCS[nm])
        want, want_sq = tc.ring_key(tc._DESCS[nm])
        assert occ.tolist() == want.tolist() and sq == want_sq
    occ = {n: tc.ring_key(tc._DESCS[nm])[0].tolist() for n, nm in zip(ts.C_NAMES, cs)}
    assert occ["empty"] == [0] * 20 and occ["full"] == [60] * 20 and occ["full_less_ring"] == [60] * 13 + [0] + [60] * 6
    assert sum(occ["single"]) == 1 and occ["one_column"] == [1] * 20 and sum(occ["floor"]) == 2
    e, f, g = ts.C_NAMES.index("empty"), ts.C_NAMES.index("full"), ts.C_NAMES.index("full_less_ring")
    assert (ts.c_dk(e, f), ts.c_dk(f, f), ts.c_dk(f, g), ts.c_dk(e, g)) == (72000, 0, 3600, 68400)
    # the full frame asks: its twin in the other slot at dk 0 and d 0, the empty frame last at dk 72 000
    got, cand = ts.host_got("A", ts.C_QUERIES[f], ts.C_SLOTS, 64, 8, 0)
    assert cand == 11 and got[0] == (ts.C_SLOTS[1], 5 - f, 0, 0, 0)
    assert sorted(r[4] for r in got)[:3] == [0, 3600, 3600]
    got, _ = ts.host_got("A", ts.C_QUERIES[e], ts.C_SLOTS, 64, 8, 0)
    # the empty frame asks: every d is 1, so the ranks are the shortlist's order — (dk, slot, id)
    assert [(r[4], r[0], r[1]) for r in got] == ts.ranked("A", ts.C_QUERIES[e], ts.C_SLOTS)[:8] and all(r[2:4] == (0, tk.bits(1.0)) for r in got)
    got, _ = ts.host_got("A", ts.C_QUERIES[-1], ts.C_SLOTS, 64, 8, 0)
    assert all(r[2:4] == (0, tk.bits(1.0)) for r in got) and got[0][4] == 0
    dks = {r[0] for q in ts.C_QUERIES for r in ts.ranked("A", q, ts.C_SLOTS)}
    assert {0, 1, 3600, 68400, 72000} <= dks
