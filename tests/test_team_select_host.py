"""The team selection on the CPU (include/lins_host.h lins_host_team_select; csrc/host/team_select.h) against the
independent numpy statement of tests/team_map_np.py and against pairs read off by hand.  Every output is an integer:
exact equality throughout."""
import itertools

import numpy as np
import pytest

import team_map_np as tm

PKG = "lins---lidar-inertial-slam_amd"


@pytest.fixture(scope="module")
def team():
    import importlib

    return importlib.import_module(PKG + ".team")


def got_of(team, c, cap=None):
    r = team.host_select(c["targets"], c["centre"], c["radius"], c["leaf"], cap=cap)
    return r if isinstance(r, int) else [tuple(p) for p in r.tolist()]


@pytest.mark.parametrize("c", tm.CRAFTED, ids=[c["name"] for c in tm.CRAFTED])
def test_crafted_cases(team, c):
    want = tm.team_select(c["targets"], c["centre"], c["radius"], c["leaf"])
    assert want == c["want"]  # (the numpy statement against the pairs by hand)
    assert got_of(team, c) == want


def test_every_permutation_of_the_target_list_gives_the_same_pairs(team):
    got = [got_of(team, c) for c in tm.PERMUTED]
    assert len(got) == 6 and all(g == got[0] for g in got)
    assert got[0] == tm.team_select(tm.THREE, (0.25, -0.25, 0), 4.0, 1.0)
    assert len({s for s, _ in got[0]}) == 3  # every slot contributes


def test_stride_one_too_small(team):
    c = tm.PERMUTED[0]
    want = tm.team_select(c["targets"], c["centre"], c["radius"], c["leaf"])
    assert got_of(team, c, cap=len(want)) == want
    assert got_of(team, c, cap=len(want) - 1) == tm.E_CAPACITY


def test_random_cases_on_a_lattice(team):
    cases = tm.random_cases()
    ties = multi = 0
    for c in cases:
        want = tm.team_select(c["targets"], c["centre"], c["radius"], c["leaf"])
        assert got_of(team, c) == want, c["name"]
        multi += len({s for s, _ in want}) > 1
        ties += tm.hits_of(c["targets"], c["centre"], c["radius"]) > len(want)
    assert len(cases) == 200 and multi > 50 and ties > 100  # (teams that mix slots; cells that hold more than one hit)


def test_refusals(team):
    one = [(0, tm.poses6([(0, 0, 0)]))]
    assert team.host_select(one, (0, 0, 0), -1.0, 1.0) == tm.E_ARG
    assert team.host_select(one, (0, 0, float("nan")), 1.0, 1.0) == tm.E_ARG
    assert team.host_select(one, (0, 0, 0), 1.0, 0.0) == tm.E_ARG
    assert team.host_select([(-1, one[0][1])], (0, 0, 0), 1.0, 1.0) == tm.E_ARG
    bad = tm.poses6([(0, 0, 0), (np.inf, 0, 0)])
    assert team.host_select([(0, bad)], (0, 0, 0), 1.0, 1.0) == -4  # LINS_E_INPUT
