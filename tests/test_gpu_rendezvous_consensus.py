"""lins_rendezvous_consensus_batch (include/lins_team.h; csrc/rendezvous_consensus_kernels.hip) against its definition,
lins_host_rendezvous_consensus: record for record, bit for bit — the kernel calls the host's scalar text on its LDS copy
of the table — on the 200 seeded tables and the corners of tests/rendezvous_window_np.py, at the wave and workgroup
edges (H = 0, 1, 2, 63, 64, 65, 127, 128), alone, in a batch and in reversed order, after an unrelated call on the same
context, and for n = 0.  The call needs a context only: no archive, no place store."""
import numpy as np
import pytest

import rendezvous_window_np as rw

pytestmark = pytest.mark.gpu
E_ARG, E_INPUT = -1, -4
EDGES = (0, 1, 2, 63, 64, 65, 127, 128)


@pytest.fixture(scope="module")
def team(pkg):
    import importlib

    return importlib.import_module(pkg.__name__ + ".team")


@pytest.fixture(scope="module")
def ctx(pkg, ieskf):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=16384)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want(host):
    """the definition's answer per seeded table, computed once"""
    return [host.rendezvous_consensus(t) for t in rw.tables()]


def test_the_seeded_tables_in_one_launch(ctx, team, want):
    got = team.consensus_batch(ctx, rw.tables())
    assert isinstance(got, list) and len(got) == rw.N_TABLES
    for s in range(rw.N_TABLES):
        assert got[s] == want[s], s
    print("consensus launch over %d tables (%d hypotheses): %.3f ms" % (rw.N_TABLES, sum(len(t) for t in rw.tables()), team.consensus_stats(ctx)))


@pytest.mark.parametrize("name", sorted(rw.corners()))
def test_corner(ctx, team, host, name):
    hyps, kw, pinned = rw.corners()[name]
    got = team.consensus_batch(ctx, [hyps], **kw)
    assert got == [host.rendezvous_consensus(hyps, **kw)]
    for k, v in (pinned or {}).items():
        assert got[0][k] == v, (k, got)


def test_wave_and_workgroup_edges_alone_in_a_batch_and_reversed(ctx, team, host):
    tabs = [rw.sized(H) for H in EDGES]
    ref = [host.rendezvous_consensus(t) for t in tabs]
    assert [len(t) for t in tabs] == list(EDGES) and ref[0]["winner"] == -1 and all(r["winner"] >= 0 for r in ref[1:])
    assert team.consensus_batch(ctx, tabs) == ref
    assert team.consensus_batch(ctx, tabs[::-1]) == ref[::-1]
    for t, r in zip(tabs, ref):
        assert team.consensus_batch(ctx, [t]) == [r]
        assert team.consensus_batch(ctx, [tabs[4], t, tabs[7]]) == [ref[4], r, ref[7]]  # an entry in a batch of 3
    # a permutation of a table moves only the indices
    for t, r in zip(tabs[2:], ref[2:]):
        other, perm = rw.permuted(t, 3)
        g = team.consensus_batch(ctx, [other])[0]
        assert (perm[g["winner"]], g["support"], g["n_admissible"], sorted(perm[i] for i in g["members"])) == (r["winner"], r["support"], r["n_admissible"], r["members"])


def test_after_an_unrelated_call_and_with_nothing_to_do(ctx, team, want, pkg, host):
    some = [0, 17, 199]
    first = team.consensus_batch(ctx, [rw.tables()[s] for s in some])
    assert first == [want[s] for s in some]
    ctx.update(host.synth_pair(0))  # an IESKF update on the same context and stream
    big = team.consensus_batch(ctx, rw.tables()[:50])  # ... and a larger batch: the staging buffers grow
    assert big == want[:50]
    assert team.consensus_batch(ctx, [rw.tables()[s] for s in some]) == first
    assert team.consensus_batch(ctx, []) == []


def test_refusals_come_before_anything_is_queued(ctx, team, host):
    good = [rw.shift((0, 0, 0), query=0), rw.shift((0, 0, 0), query=1)]
    ref = team.consensus_batch(ctx, [good, good])
    assert ref == [host.rendezvous_consensus(good)] * 2
    nan = float("nan")
    for kw in (dict(max_translation=-1.0), dict(max_translation=float("inf")), dict(min_cos_rotation=nan)):
        assert team.consensus_batch(ctx, [good], **kw) == E_ARG, kw
        assert team.consensus_batch(ctx, [], **kw) == E_ARG  # (the parameters are asked first, as the context is)
    for off in ([1, 2, 4], [0, 3, 2], [0, 2, 131]):
        assert team.consensus_batch(ctx, [good, good], offsets=off) == E_ARG, off
    full = [rw.shift((0, 0, 0), query=i // 8, rank=i % 8) for i in range(128)]
    assert team.consensus_batch(ctx, [full + [rw.shift((0, 0, 0))]], offsets=[0, 129]) == E_ARG
    for bad in (dict(query=16), dict(rank=8), dict(admissible=2), dict(query=0, rank=0)):
        assert team.consensus_batch(ctx, [good, [good[0], dict(good[1], **bad)]]) == E_ARG, bad
    bad_x = dict(good[1], X=np.full((4, 4), nan))
    assert team.consensus_batch(ctx, [good, [good[0], bad_x]]) == E_INPUT
    assert team.consensus_batch(ctx, [[good[0], dict(good[1], fitness=-1.0)], good]) == E_INPUT
    # an argument error in a later table comes before an input error in an earlier one; an inadmissible NaN is not read
    assert team.consensus_batch(ctx, [[good[0], bad_x], [good[0], dict(good[1], rank=8)]]) == E_ARG
    assert team.consensus_batch(ctx, [[good[0], dict(bad_x, admissible=0)]]) == [host.rendezvous_consensus([good[0], dict(bad_x, admissible=0)])]
    assert team.consensus_batch(ctx, [good, good]) == ref
