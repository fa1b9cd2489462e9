"""The certificates of the batch kernel's lean correspondence phase fetch their tracked candidates' records in one trip, on
clamped grid positions (csrc/ieskf_lds_impl.h pt_rec, csrc/ieskf_lds_lean_body.inc, walk_lean of csrc/ieskf_lds_lean.h).
No operation of the arithmetic moved, so

  * tests/golden/cert_fetch_parent_bits.npz — what the library gave BEFORE the change on two families of scans (recipe:
    tests/golden/make_cert_fetch_golden.py) — is reproduced bit for bit, with the numbers of selections the certificates
    decided: plainly, with a hand-over after every iteration, and in a context whose carry records and walk cache a
    larger batch of other scans has filled with positions of larger clouds;
  * hand-built pairs (tests/cert_fetch_cases.py), on which a fetch that is no longer guarded can go wrong — clouds of one
    to three points, a query that finds its first neighbour late, a kind of query whose cloud is empty, candidates on the
    last resident and the first global record — come out as the CPU oracle's: flags, iterations and row counts equal,
    state and covariance within TIGHT_STATE / TIGHT_COV of tests/test_gpu_parity.py; and with every certificate checked
    against a real search on the device (LINS_DEBUG_SKIP=8) none disagrees.
"""
import importlib.util
import os

import numpy as np
import pytest

import cert_fetch_cases as cases_mod
from test_gpu_parity import TIGHT_COV, TIGHT_STATE, _max_parts, _run_cut, _same_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "cert_fetch_parent_bits.npz")
RUNS = ["room_fixed", "room_stop", "open_fixed", "open_stop"]
HAND = ["tiny1", "tiny2", "tiny3", "late", "late+lines", "poles", "poles+planes", "edge"]


@pytest.fixture(scope="module")
def recipe():
    spec = importlib.util.spec_from_file_location("make_cert_fetch_golden", os.path.join(HERE, "golden", "make_cert_fetch_golden.py"))
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
    """Every iteration a part of its own: each warm iteration reads the carry records another workgroup wrote.  (The counts
    of decided selections are per part and not compared.)"""
    prm, pairs = runs[name]
    whole, cut0 = _run_cut(ieskf, monkeypatch, prm, pairs, 0)
    assert cut0 == (1, 0)
    parts, cut = _run_cut(ieskf, monkeypatch, prm, pairs, 1, LINS_RELAY_CUTS=14, LINS_QUEUE_GRID=len(pairs) // 2)
    assert cut == (_max_parts(prm.num_iter, 1, 14), 0) and cut[0] >= 10, cut
    for a, b in zip(whole, parts):
        _same_bits(a, b)
    _assert_golden(recipe, golden, name, parts, decided=False)


def test_the_recorded_bits_in_a_context_that_ran_a_larger_other_batch(ieskf, host, recipe, runs, golden):
    """64 room scans of other seeds first: their carry records (and walk-cache entries) stay in the context, with positions
    of clouds larger than the ones that follow.  Planes 2-3 of a query that has no neighbour are not its own — they are
    fetched now (and discarded): on clamped positions."""
    other = host.synth_batch(64, start=33000)
    prm = runs["room_fixed"][0]
    with ieskf.IeskfContext(prm, max_batch=64, max_targets=16384, search="mr") as c:
        c.update_batch(other)
        for name in ("open_fixed", "room_fixed"):  # the smaller clouds first
            res = c.update_batch(runs[name][1])
            assert c.last_search() == "mr"
            _assert_golden(recipe, golden, name, res)
    prm = runs["room_stop"][0]
    with ieskf.IeskfContext(prm, max_batch=64, max_targets=16384, search="mr") as c:
        c.update_batch(other)
        for name in ("open_stop", "room_stop"):
            res = c.update_batch(runs[name][1])
            _assert_golden(recipe, golden, name, res)


# ---- hand-built pairs, the oracle as judge ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand(pkg, host, oracle):
    """(params, names, pairs, the oracle's results); every input is checked on the oracle's trace to be what it was built as."""
    prm = pkg.default_params(num_iter=6, fixed_iters=1)
    built = {"tiny1": cases_mod.tiny_plane_pair(pkg, 1), "tiny2": cases_mod.tiny_plane_pair(pkg, 2), "tiny3": cases_mod.tiny_plane_pair(pkg, 3),
             "late": cases_mod.late_neighbour_pair(pkg), "late+lines": cases_mod.late_neighbour_pair(pkg, corner_queries=3),
             "poles": cases_mod.poles_pair(pkg), "poles+planes": cases_mod.poles_pair(pkg, surf_queries=3),
             "edge": cases_mod.resident_edge_pair(pkg, host, oracle, prm)}
    assert list(built) == HAND
    pairs, want = [], []
    for name, (pair, check) in built.items():
        w, tr = oracle.ieskf(prm, pair, oracle.FORM_DENSE, oracle.NN_KDTREE, trace=True)
        assert (w.iters, w.converged, w.diverged) == (6, 0, 0), name
        check(w, tr)
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
    """The hand-built pairs as ONE batch of the batch shape, plainly and with LINS_DEBUG_SKIP=8 (every certificate is followed
    by the search it would have saved, disagreements counted on the device)."""
    prm, pairs, _ = hand
    out = {}
    mp = pytest.MonkeyPatch()
    try:
        for mode in ("plain", "verify"):
            if mode == "verify":
                mp.setenv("LINS_ENABLE_DEBUG_KNOBS", "1")
                mp.setenv("LINS_DEBUG_SKIP", "8")
            with ieskf.IeskfContext(prm, max_batch=len(pairs), max_targets=16384, search="mr") as c:
                out[mode] = c.update_batch(pairs)
                assert c.last_search() == "mr"
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("mode", ["plain", "verify"])
@pytest.mark.parametrize("name", HAND)
def test_hand_built_pairs_come_out_as_the_oracles(hand, hand_results, name, mode):
    _, _, want = hand
    k = HAND.index(name)
    got = hand_results[mode][k]
    if mode == "verify":
        assert got.reserved[0] == 0, f"{got.reserved[0]} certificate disagreements"
    _assert_tight(got, want[k], f"{name} {mode}")


@pytest.mark.parametrize("name", HAND)
def test_a_hand_built_pair_alone_in_its_context(ieskf, hand, hand_results, name):
    """One scan per context — for the small ones a context whose buffers hold nothing but this scan's few points — gives the
    bits the scan has inside the batch."""
    prm, pairs, want = hand
    k = HAND.index(name)
    with ieskf.IeskfContext(prm, max_batch=1, max_targets=16384, search="mr") as c:
        got = c.update_batch([pairs[k]])[0]
        assert c.last_search() == "mr"
    _same_bits(got, hand_results["plain"][k])
    _assert_tight(got, want[k], f"{name} alone")
