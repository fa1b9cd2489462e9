"""lins_host_rendezvous_consensus (include/lins_host.h; the scalar text csrc/host/rendezvous_consensus.h) against the
independent numpy statement of tests/rendezvous_window_np.py: every decision equal on 200 seeded tables of two or three
clusters of X with noise on both sides of the bars, and on the contract's corners.

The restatement rounds differently, so the seeded tables must hold no pair on a bar: the number of comparable pairs within
a relative 1e-9 of a bar is asserted to be 0 — a condition on the inputs, not a tolerance."""
import ctypes as C

import numpy as np
import pytest

import rendezvous_window_np as rw

E_ARG, E_INPUT = -1, -4


def test_the_seeded_tables_hold_no_pair_on_a_bar_and_both_sides_of_each():
    near = inside = outside = turned = 0
    for hyps in rw.tables():
        near += rw.near_bars(hyps)
        for i, a in enumerate(hyps):
            for b in hyps[i + 1:]:
                if rw.comparable(a, b):
                    tr, far = rw.measures(a, b)
                    ok_r = tr >= 1.0 + 2.0 * rw.MIN_COS
                    inside += ok_r and far <= rw.MAX_T
                    outside += ok_r and far > rw.MAX_T and far < 3.0 * rw.MAX_T  # (the same cluster, beyond the bar)
                    turned += (not ok_r) and far <= rw.MAX_T
    print("comparable pairs: %d consistent, %d just beyond the translation bar, %d beyond the rotation bar alone; %d near a bar" % (inside, outside, turned, near))
    assert near == 0
    assert inside > 1000 and outside > 1000 and turned > 100


def test_every_decision_is_the_numpy_statements(host):
    sizes, supports = set(), set()
    for s, hyps in enumerate(rw.tables()):
        got, want = host.rendezvous_consensus(hyps), rw.consensus(hyps)
        assert got == want, s
        sizes.add(len(hyps)), supports.add(got["support"])
    print("table sizes:", sorted(sizes), "supports seen:", sorted(supports))
    assert 128 in sizes and max(supports) >= 5 and 1 in supports


@pytest.mark.parametrize("name", sorted(rw.corners()))
def test_corner(host, name):
    hyps, kw, want = rw.corners()[name]
    got = host.rendezvous_consensus(hyps, **kw)
    assert isinstance(got, dict), got
    for k, v in (want or {}).items():
        assert got[k] == v, (k, got)
    assert got == rw.consensus(hyps, kw.get("max_translation", rw.MAX_T), kw.get("min_cos_rotation", rw.MIN_COS))


def test_the_relation_is_symmetric_and_a_permutation_moves_only_the_indices(host):
    for s in (0, 7, 31, 120, 199):
        hyps = rw.tables()[s]
        base = host.rendezvous_consensus(hyps)
        for seed in (1, 2):
            other, perm = rw.permuted(hyps, seed)
            got = host.rendezvous_consensus(other)
            assert (perm[got["winner"]] if got["winner"] >= 0 else -1, got["support"], got["n_admissible"]) == (base["winner"], base["support"], base["n_admissible"])
            assert sorted(perm[i] for i in got["members"]) == base["members"]
        # symmetry: a table of two has support 2 iff the two are consistent, whichever comes first
        rng = np.random.default_rng(s)
        for _ in range(100):
            a, b = (hyps[int(i)] for i in rng.choice(len(hyps), 2, replace=False))
            if rw.comparable(a, b):
                ab, ba = host.rendezvous_consensus([a, b]), host.rendezvous_consensus([b, a])
                assert ab["support"] == ba["support"] == (2 if rw.consistent(a, b) else 1), (s, a, b)


def test_refusals(host, defs):
    good = [rw.shift((0, 0, 0), query=0), rw.shift((0, 0, 0), query=1)]
    assert isinstance(host.rendezvous_consensus(good), dict)
    assert host.rendezvous_consensus(good, n_hyp=-1) == E_ARG
    big = defs.consensus_table([rw.shift((0, 0, 0), query=i // 8 % 16, rank=i % 8) for i in range(129)])
    assert host.rendezvous_consensus(big, n_hyp=129) == E_ARG and isinstance(host.rendezvous_consensus(big, n_hyp=128), dict)
    for kw in (dict(max_translation=-1.0), dict(max_translation=float("inf")), dict(max_translation=float("nan")), dict(min_cos_rotation=float("nan"))):
        assert host.rendezvous_consensus(good, **kw) == E_ARG, kw
    # the two bars are all the rule reads of its parameters
    assert host.rendezvous_consensus(good, window=0, stride=0, min_support=99) == host.rendezvous_consensus(good)
    for bad in (dict(query=-1), dict(query=16), dict(rank=-1), dict(rank=8), dict(admissible=2), dict(admissible=-1), dict(query=0, rank=0)):
        assert host.rendezvous_consensus([good[0], dict(good[1], **bad)]) == E_ARG, bad
    nan, inf = float("nan"), float("inf")
    for field, at, v in (("X", (0, 0), nan), ("X", (2, 3), inf), ("X", (3, 3), -inf), ("p", (1,), nan), ("p", (2,), inf)):
        h = dict(good[1], **{field: np.array(good[1][field], np.float64)})
        h[field][at] = v
        assert host.rendezvous_consensus([good[0], h]) == E_INPUT, (field, at, v)
        assert isinstance(host.rendezvous_consensus([good[0], dict(h, admissible=0)]), dict)  # (an inadmissible one is not read)
    for f in (nan, inf, -1e-300):
        assert host.rendezvous_consensus([good[0], dict(good[1], fitness=f)]) == E_INPUT, f
    assert isinstance(host.rendezvous_consensus([good[0], dict(good[1], fitness=0.0)]), dict)
    # an argument error comes before an input error; null pointers
    assert host.rendezvous_consensus([dict(good[0], fitness=nan), dict(good[1], query=16)]) == E_ARG
    L = host.lib()
    prm, out = defs.consensus_params(L), defs.ConsensusResultC()
    L.lins_host_rendezvous_consensus.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.lins_host_rendezvous_consensus.restype = C.c_int
    tab = defs.consensus_table(good)
    assert L.lins_host_rendezvous_consensus(None, 2, C.byref(prm), C.byref(out)) == E_ARG
    assert L.lins_host_rendezvous_consensus(tab, 2, None, C.byref(out)) == E_ARG
    assert L.lins_host_rendezvous_consensus(tab, 2, C.byref(prm), None) == E_ARG
    assert L.lins_host_rendezvous_consensus(None, 0, C.byref(prm), C.byref(out)) == 0 and out.winner == -1
    # a refused call writes nothing
    out.winner, out.support = 77, 78
    tab[1].query = 16
    assert L.lins_host_rendezvous_consensus(tab, 2, C.byref(prm), C.byref(out)) == E_ARG and (out.winner, out.support) == (77, 78)
