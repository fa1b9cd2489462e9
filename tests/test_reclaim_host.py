"""The compaction plan of the key-frame archive's arena (csrc/host/arena_reclaim.h, exported by liblins_host.so as
lins_host_arena_reclaim_plan; include/lins_lifecycle.h): executed on a numpy array it is a stable compaction whatever the
chunk, every pass holds at most `chunk` points, a pass marked direct has disjoint ranges, and after every pass the
surviving points not yet moved lie at or beyond the end of what the pass wrote."""
import numpy as np
import pytest

N_TABLES = 200
PATTERNS = ("front", "back", "adjacent", "everywhere", "nowhere", "random")


def _table(seed):
    """(offset, points, keep) of a dense arena of 1-40 blocks; sizes 0 and 1 are frequent"""
    rng = np.random.default_rng(1000 + seed)
    nb = int(rng.integers(1, 41))
    sizes = rng.choice([0, 1, 2, 3, 7, 16, 33, 64], size=nb, p=[0.15, 0.15, 0.1, 0.1, 0.15, 0.15, 0.1, 0.1])
    pattern = PATTERNS[(seed // 8) % len(PATTERNS)]  # (every group of the test below sees every pattern)
    keep = np.ones(nb, bool)
    if pattern == "front":
        keep[: int(rng.integers(1, nb + 1))] = False
    elif pattern == "back":
        keep[nb - int(rng.integers(1, nb + 1)):] = False
    elif pattern == "adjacent":
        a = int(rng.integers(0, nb))
        keep[a: a + int(rng.integers(2, 5))] = False
    elif pattern == "everywhere":
        keep[:] = False
    elif pattern == "random":
        keep = rng.random(nb) < 0.6
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return [(int(o), int(n), bool(k)) for o, n, k in zip(off, sizes, keep)], pattern


def _chunks(blocks):
    total = sum(n for _, n, _ in blocks)
    one = max([n for _, n, _ in blocks if n] + [1])  # the size of one block
    return sorted({1, 7, one, total + 5})


def _run(host, blocks, chunk):
    """execute the plan on an array of distinct values, checking every pass; returns the arena afterwards"""
    total = sum(n for _, n, _ in blocks)
    arena = np.arange(1, total + 1, dtype=np.int64)
    passes = host.arena_reclaim_plan(blocks, chunk)
    segs = [(s, d, n, p) for p, ps in enumerate(passes) for (s, d, n) in ps["segments"]]
    # order kept, dst <= src, destinations handed out consecutively, no empty segment
    for (s, d, n, _), nxt in zip(segs, segs[1:] + [None]):
        assert n >= 1 and 0 <= d <= s and s + n <= total
        if nxt is not None:
            assert nxt[0] >= s + n and nxt[1] == d + n
    for p, ps in enumerate(passes):
        sg = ps["segments"]
        m = sum(n for _, _, n in sg)
        assert 1 <= m <= chunk, (p, m, chunk)
        D = sg[0][1]
        if ps["direct"]:  # one forward copy: the ranges written and the ranges read are disjoint
            assert D + m <= sg[0][0]
            wr = np.zeros(total, bool)
            for s, d, n in sg:
                wr[d: d + n] = True
            for s, d, n in sg:
                assert not wr[s: s + n].any()
            for s, d, n in sg:
                arena[d: d + n] = arena[s: s + n]
        else:  # copy out, then in
            stage = np.concatenate([arena[s: s + n] for s, _, n in sg])
            assert len(stage) <= chunk
            at = 0
            for s, d, n in sg:
                arena[d: d + n] = stage[at: at + n]
                at += n
        # the invariant: what has not moved yet lies at or beyond the end of what this pass wrote
        later = [s for (s, _, _, q) in segs if q > p]
        assert all(s >= D + m for s in later), (p, D, m, min(later))
    return arena, passes


@pytest.mark.parametrize("group", range(8))
def test_plan_is_a_stable_compaction_for_every_chunk(host, group):
    seen = set()
    for seed in range(group, N_TABLES, 8):
        blocks, pattern = _table(seed)
        seen.add(pattern)
        total = sum(n for _, n, _ in blocks)
        want = np.concatenate([np.arange(o + 1, o + n + 1, dtype=np.int64) for o, n, k in blocks if k] + [np.zeros(0, np.int64)])
        for chunk in _chunks(blocks):
            arena, passes = _run(host, blocks, chunk)
            assert np.array_equal(arena[: len(want)], want), (seed, chunk)
            # only blocks behind the first dropped one appear
            drops = [o for o, _, k in blocks if not k]
            moved = sum(n for ps in passes for _, _, n in ps["segments"])
            if not drops:
                assert passes == []
            else:
                assert all(s >= drops[0] for ps in passes for s, _, _ in ps["segments"])
                gone_before = [sum(m for oo, m, kk in blocks if not kk and oo < o) for o, n, k in blocks]
                assert moved == sum(n for (o, n, k), g in zip(blocks, gone_before) if k and g > 0)
            assert total >= len(want)
    assert len(seen) == len(PATTERNS)


def test_both_kinds_of_pass_occur_and_chunk_one_is_all_direct(host):
    blocks = [(0, 3, False), (3, 500, True), (503, 40, False), (543, 20, True)]
    big = host.arena_reclaim_plan(blocks, 10 ** 6)
    assert [p["direct"] for p in big] == [False] and sum(n for _, _, n in big[0]["segments"]) == 520
    kinds = {p["direct"] for p in host.arena_reclaim_plan(blocks, 64)}
    assert kinds == {False, True}  # (the gap grows past 64 behind the second dropped block)
    assert all(p["direct"] for p in host.arena_reclaim_plan(blocks, 1))
    _run(host, blocks, 64)


def test_gaps_between_blocks_and_refusals(host):
    blocks = [(2, 3, True), (10, 4, False), (20, 5, True), (30, 0, False), (31, 2, True)]
    passes = host.arena_reclaim_plan(blocks, 3)
    flat = [g for p in passes for g in p["segments"]]
    assert flat[0][:2] == (20, 10) and sum(n for _, _, n in flat) == 7 and flat[-1][1] + flat[-1][2] == 17
    for bad in ([(5, 3, True), (4, 2, False)], [(0, -1, True)]):  # out of order, a negative count
        with pytest.raises(RuntimeError):
            host.arena_reclaim_plan(bad, 4)
    with pytest.raises(RuntimeError):
        host.arena_reclaim_plan(blocks, 0)
