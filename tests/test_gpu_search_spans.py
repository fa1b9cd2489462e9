"""The searches of the batch kernel's lean core read the bounds of several windows in one trip: on clamped cells, the words
kept under the tests that used to guard the reads, two positions to a word (csrc/ieskf_lds_impl.h spans_read / spans_pack /
scan_packed; nn_lean of csrc/ieskf_lds_lean.h).  Windows are the windows they were, scanned in the order they were, so

  * tests/golden/search_spans_parent_bits.npz — what the library gave BEFORE the change on two families of scans (recipe:
    tests/golden/make_search_spans_golden.py) — is reproduced bit for bit, with the numbers of selections the certificates
    decided: plainly, with a hand-over after every iteration, and behind a 64-scan batch of other seeds in the same context;
  * hand-built pairs (tests/search_spans_cases.py) on which the span handling can go wrong — a wall across the last
    azimuth column, queries on ring 0 and ring 15, an empty neighbour ring, clouds of one to three points, an empty cloud
    of either kind, windows across the last resident record in a seed and in a widening round, a query with rho = 0, a
    deferred cold search, waves of 32 and of 33 queries — come out as the CPU oracle's (reduced form, kd-tree): flags,
    iterations and row counts equal, state and covariance within TIGHT_STATE / TIGHT_COV of tests/test_gpu_parity.py.
    The packed spans serve the cold searches of waves that hold more than 32 queries: every case is built with its
    critical queries in such a wave, and the fixture asserts that from the kernel's share arithmetic.
"""
import importlib.util
import os

import numpy as np
import pytest

import search_spans_cases as cases_mod
from test_gpu_parity import TIGHT_COV, TIGHT_STATE, _max_parts, _run_cut, _same_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "search_spans_parent_bits.npz")
RUNS = ["room_fixed", "room_stop", "open_fixed", "open_stop"]
HAND = ["wrap", "outer_rings", "gap_ring", "tiny1", "tiny2", "tiny3", "no_lines", "no_planes", "edge_seed", "edge_round", "nadir", "deferred",
        "wave32", "wave33"]


@pytest.fixture(scope="module")
def recipe():
    spec = importlib.util.spec_from_file_location("make_search_spans_golden", os.path.join(HERE, "golden", "make_search_spans_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def runs(recipe):
    """name -> (params, pairs) of the four recorded runs; built once, never modified."""
    return recipe.runs()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _assert_golden(recipe, golden, name, res, decided=True):
    got = recipe.pack(res)
    for k, v in got.items():
        if k == "decided" and not decided:
            continue
        want = golden[name + "." + k]
        if v.dtype.kind == "f":  # 64-bit pattern for 64-bit pattern
            assert np.array_equal(v.view(np.uint64), want.view(np.uint64)), (name, k)
        else:
            assert np.array_equal(v, want), (name, k, v, want)


@pytest.mark.parametrize("name", RUNS)
def test_the_bits_recorded_before_the_change(ieskf, recipe, runs, golden, name):
    prm, pairs = runs[name]
    with ieskf.IeskfContext(prm, max_batch=len(pairs), max_targets=16384, search="mr") as c:
        res = c.update_batch(pairs)
        assert c.last_search() == "mr"
    assert sum(r.reserved[1] + r.reserved[2] for r in res) > 100 * len(pairs)  # the certificates did the deciding
    _assert_golden(recipe, golden, name, res)


@pytest.mark.parametrize("name", RUNS)
def test_the_recorded_bits_with_a_hand_over_after_every_iteration(ieskf, recipe, runs, golden, monkeypatch, name):
    """Every iteration a part of its own.  (The counts of decided selections are per part and not compared.)"""
    prm, pairs = runs[name]
    whole, cut0 = _run_cut(ieskf, monkeypatch, prm, pairs, 0)
    assert cut0 == (1, 0)
    parts, cut = _run_cut(ieskf, monkeypatch, prm, pairs, 1, LINS_RELAY_CUTS=14, LINS_QUEUE_GRID=len(pairs) // 2)
    assert cut == (_max_parts(prm.num_iter, 1, 14), 0) and cut[0] >= 10, cut
    for a, b in zip(whole, parts):
        _same_bits(a, b)
    _assert_golden(recipe, golden, name, parts, decided=False)


def test_the_recorded_bits_in_a_context_that_ran_a_larger_other_batch(ieskf, host, recipe, runs, golden):
    """64 room scans of other seeds first, in the same context."""
    other = host.synth_batch(64, start=38000)
    for fixed, stop in (("open_fixed", "room_fixed"), ("open_stop", "room_stop")):
        prm = runs[fixed][0]
        with ieskf.IeskfContext(prm, max_batch=64, max_targets=16384, search="mr") as c:
            c.update_batch(other)
            for name in (fixed, stop):  # the smaller clouds first
                res = c.update_batch(runs[name][1])
                assert c.last_search() == "mr"
                _assert_golden(recipe, golden, name, res)


# ---- hand-built pairs, the oracle as judge ------------------------------------------------------------------------------------
def build_hand(pkg, host, oracle, prm):
    """name -> (pair, critical queries, check): every case with its critical queries in a wave of more than 32."""
    return {"wrap": cases_mod.wrap_pair(pkg), "outer_rings": cases_mod.outer_rings_pair(pkg), "gap_ring": cases_mod.gap_ring_pair(pkg),
            "tiny1": cases_mod.tiny_pair(pkg, 1), "tiny2": cases_mod.tiny_pair(pkg, 2), "tiny3": cases_mod.tiny_pair(pkg, 3),
            "no_lines": cases_mod.no_lines_pair(pkg), "no_planes": cases_mod.no_planes_pair(pkg),
            "edge_seed": cases_mod.resident_edge_pair(pkg, host, oracle, prm, (0.0, 0.3, 0.6)),
            "edge_round": cases_mod.resident_edge_pair(pkg, host, oracle, prm, (0.0, 3.2, 4.2)),
            "nadir": cases_mod.nadir_pair(pkg), "deferred": cases_mod.deferred_pair(pkg),
            "wave32": cases_mod.wave_fill_pair(pkg, 107), "wave33": cases_mod.wave_fill_pair(pkg, 110)}


@pytest.fixture(scope="module")
def hand(pkg, host, oracle):
    """(params, pairs, the oracle's results).  Every input is checked on the oracle's trace to be what it was built as and to
    give the oracle at least one row; and, from the share arithmetic of the batch shape, to have its critical queries in a
    wave that searches with ONE lane per query in the cold iteration — where the packed spans are (wave32: the contrary)."""
    prm = pkg.default_params(num_iter=6, fixed_iters=1)
    built = build_hand(pkg, host, oracle, prm)
    assert list(built) == HAND
    pairs, want = [], []
    for name, (pair, critical, check) in built.items():
        lanes1 = cases_mod.one_lane(len(pair.surf_flat), len(pair.corner_sharp))
        assert critical, name
        for kind, q in critical:
            assert (q in lanes1[kind]) == (name != "wave32"), (name, kind, q)
        w, tr = oracle.ieskf(prm, pair, oracle.FORM_REDUCED, oracle.NN_KDTREE, trace=True)
        assert (w.iters, w.converged, w.diverged) == (6, 0, 0), name
        check(w, tr)
        assert w.m_surf + w.m_corner > 0, (name, w.m_surf, w.m_corner)
        pairs.append(pair), want.append(w)
    return prm, pairs, want


def _assert_tight(got, want, what):
    assert (got.iters, got.converged, got.diverged) == (want.iters, want.converged, want.diverged), (what, got, want)
    assert (got.m_surf, got.m_corner) == (want.m_surf, want.m_corner), (what, got, want)
    gc, wc = np.asarray(got.cov).ravel(), np.asarray(want.cov).ravel()
    assert not np.isnan(got.state).any() and not np.isnan(gc).any(), what
    ds = np.abs(got.state - want.state).max()
    dc = np.abs(gc - wc).max() / np.abs(wc).max()
    print(f"{what}: state {ds:.2e}, covariance {dc:.2e} (rel)")
    assert ds <= TIGHT_STATE and dc <= TIGHT_COV, what


@pytest.fixture(scope="module")
def hand_results(ieskf, hand):
    """The hand-built pairs as ONE batch of the batch shape."""
    prm, pairs, _ = hand
    with ieskf.IeskfContext(prm, max_batch=len(pairs), max_targets=16384, search="mr") as c:
        out = c.update_batch(pairs)
        assert c.last_search() == "mr"
    return out


@pytest.mark.parametrize("name", HAND)
def test_hand_built_pairs_come_out_as_the_oracles(hand, hand_results, name):
    _, _, want = hand
    k = HAND.index(name)
    _assert_tight(hand_results[k], want[k], name)


@pytest.mark.parametrize("name", HAND)
def test_a_hand_built_pair_alone_in_its_context(ieskf, hand, hand_results, name):
    """One scan per context gives the bits the scan has inside the batch."""
    prm, pairs, want = hand
    k = HAND.index(name)
    with ieskf.IeskfContext(prm, max_batch=1, max_targets=16384, search="mr") as c:
        got = c.update_batch([pairs[k]])[0]
        assert c.last_search() == "mr"
    _same_bits(got, hand_results[k])
    _assert_tight(got, want[k], f"{name} alone")
