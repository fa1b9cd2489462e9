"""lins_place_topk_batch (include/lins_place.h; place_select_kernel behind the search) against its definition on the CPU,
lins_host_place_topk, bit for bit, and against the numpy selection of tests/place_topk_cases.py over the device's own
row (lins_place_distances): for every frame count at the edges of the search's chunk (20) and of the select workgroup's
stride (256), every K and separation; whatever the chunk, the batch, its order and the context's history; rank 0 equal to
lins_place_search_batch; and the refusals."""
import numpy as np
import pytest

import place_topk_cases as tk

pytestmark = pytest.mark.gpu
host = tk.host
F = np.float32
POSE = (0.5, -1.0, 0.2, 0.01, -0.02, 0.4)
COUNTS = (0, 1, 2, 19, 20, 21, 255, 256, 257, 600)
QS = len(COUNTS)  # the slot of the three query frames
KS, SEPS = (1, 2, 8), (0, 1, 4)
E_ARG, E_INPUT, E_STATE = -1, -4, -6
UNFILLED = (tk.bits(1.0), -1, 0)


def context(pkg, ieskf, n_slots, max_frames, cap):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=max(n_slots, 1), max_targets=1024)
    c.streams_init(n_slots)
    c.archive_init(n_slots, max_frames, cap)
    assert c.place_init() == 0
    return c


def push(c, slot, ids, t0=0.0):
    for i, f in enumerate(ids):
        c.archive_push(slot, *tk.frame(f), POSE, time=t0 + i)


@pytest.fixture(scope="module")
def filled(pkg, ieskf):
    """slot s holds the first COUNTS[s] frames of the pool at times 0, 1, ..; the last slot holds the three queries"""
    c = context(pkg, ieskf, QS + 1, max(COUNTS), (sum(COUNTS) + 3) * 150)
    for s, n in enumerate(COUNTS):
        push(c, s, range(n))
    for q in range(3):
        c.archive_push(QS, *tk.query_frame(q), POSE, time=1e6)
    yield c
    c.close()


def entries_of(s):
    """slot s: the three queries from the query slot (every frame admissible), and the slot's own last frame (itself
    skipped, the time gate cutting at equality)"""
    n = COUNTS[s]
    ent = [(QS, q, s, 1e6, -1.0) for q in range(3)]
    return ent + ([(s, n - 1, s, float(n - 1), 3.0)] if n else [])


def host_want(e, k, sep):
    """lins_host_place_topk for entry e -> ([k keys, the unfilled ones included], candidates)"""
    qs, qid, s, now, gap = e
    n = COUNTS[s]
    qd = tk.query_desc(qid) if qs == QS else tk.desc(qid)
    raw, cand = host.place_topk(qd, tk.descs(n), np.arange(n, dtype=np.float64), now, gap, k, sep, skip_id=qid if qs == s else -1, raw=True)
    return tk.as_keys(raw), cand


def device_got(c, ent, k, sep):
    res = c.place_topk(ent, k, sep)
    assert isinstance(res, list) and len(res) == len(ent)
    out = []
    for e, filled_ranks, raw, cand in zip(ent, res, c.place_topk_raw, c.place_topk_candidates):
        keys = tk.as_keys(raw)
        assert keys[:len(filled_ranks)] == tk.as_keys(filled_ranks) and all(x == UNFILLED for x in keys[len(filled_ranks):])
        assert all(r["status"] == 0 and r["candidates"] == cand for r in raw)
        out.append((keys, cand))
    return out


def numpy_over_the_devices_row(c, e, k, sep):
    d, sh = c.place_distances(e)
    keys = [(tk.bits(d[i]), i, int(sh[i])) for i in range(len(d)) if sh[i] >= 0]
    sel = tk.select(keys, k, sep)
    return sel + [UNFILLED] * (k - len(sel)), len(keys)


def numpy_want(e, k, sep):
    """the sorted greedy selection over the row keys formed from host.place_distance (tests/test_place_topk_host.py holds
    lins_host_place_topk to the same statement on the CPU)"""
    qs, qid, s, now, gap = e
    n = COUNTS[s]
    keys = tk.row_keys(qid if qs == QS else ("frame", qid), n, np.arange(n, dtype=np.float64), now, gap, skip=qid if qs == s else -1)
    sel = tk.select(keys, k, sep)
    return sel + [UNFILLED] * (k - len(sel)), len(keys)


@pytest.mark.parametrize("k", KS)
def test_the_device_is_the_hosts_bits(filled, k):
    every = [e for s in range(len(COUNTS)) for e in entries_of(s)]
    for sep in SEPS:
        got = device_got(filled, every, k, sep)
        want = [numpy_want(e, k, sep) for e in every]
        assert got == want, (k, sep, [(e, g, w) for e, g, w in zip(every, got, want) if g != w][:2])
        assert filled.place_select_ms() > 0 and filled.place_stats()["pairs"] == sum(COUNTS[e[2]] for e in every)
        # lins_host_place_topk itself: every entry of the small slots; of the large ones the revisit and the slot's own frame
        for e, g in zip(every, got):
            if COUNTS[e[2]] <= 21 or (sep == 4 and e[1] in (0, COUNTS[e[2]] - 1)):
                assert g == host_want(e, k, sep), (e, k, sep)
    for s, n in enumerate(COUNTS):  # min_sep = the count: one rank at most
        ent = entries_of(s)
        got = device_got(filled, ent, k, n)
        assert got == [numpy_want(e, k, n) for e in ent], (k, s)
        assert got[0] == host_want(ent[0], k, n)
        assert all(sum(x != UNFILLED for x in keys) == min(cand, 1) for keys, cand in got)
    # the numpy selection over the device's own row
    for s in (3, 5, 8, 9):
        for e in entries_of(s):
            for sep in SEPS:
                assert device_got(filled, [e], k, sep)[0] == numpy_over_the_devices_row(filled, e, k, sep), (e, k, sep)


def test_chunks_batches_and_order_give_the_same_bits(filled):
    every = [e for s in range(len(COUNTS)) for e in entries_of(s)]
    base = device_got(filled, every, 8, 4)
    for chunk in (1, 7, 0):
        assert filled.place_set_chunk(chunk) == 0
        assert device_got(filled, every, 8, 4) == base, chunk
    rng = np.random.default_rng(5)
    perm = [int(i) for i in rng.permutation(len(every))]
    got = device_got(filled, [every[i] for i in perm], 8, 4)
    assert got == [base[i] for i in perm]
    for i in (2, len(every) - 1, len(every) - 6, 13):
        assert device_got(filled, [every[i]], 8, 4)[0] == base[i]
    assert filled.place_topk([], 4, 4) == []


def test_rank_0_is_the_search_and_another_slots_frames_are_searched(filled):
    every = [e for s in range(len(COUNTS)) for e in entries_of(s)]
    searched = filled.place_search(every)
    for k, sep in ((1, 0), (8, 0), (8, 4), (2, 600)):
        got = device_got(filled, every, k, sep)
        for e, (keys, cand), s in zip(every, got, searched):
            assert (keys[0], cand) == ((tk.bits(s["distance"]), s["id"], s["shift"]), s["candidates"]), (e, k, sep)
    # query 1 is frame 5 of the pool: in the slot of 257 frames its duplicates lead, by id, in ANOTHER slot than the query's
    (keys, cand), = device_got(filled, [(QS, 1, 8, 1e6, -1.0)], 4, 0)
    assert [x[1] for x in keys[:3]] == [5, 79, 116] and all(x[0] == 0 and x[2] == 0 for x in keys[:3]) and cand == 257
    (keys, cand), = device_got(filled, [(QS, 1, 8, 1e6, -1.0)], 4, 74)
    assert [x[1] for x in keys[:2]] == [5, 116]


def test_history_and_a_released_slot_leave_the_bits(pkg, ieskf, filled):
    ent = entries_of(5) + entries_of(2)  # the slots of 21 and of 2 frames
    want = device_got(filled, ent, 8, 1)
    c = context(pkg, ieskf, 4, 64, 1 << 16)
    push(c, 0, range(30, 60))  # lies in front of the others in the arena
    push(c, 1, range(21)), push(c, 2, range(2))
    for q in range(3):
        c.archive_push(3, *tk.query_frame(q), POSE, time=1e6)
    remap = {5: 1, 2: 2, QS: 3}
    mine = [(remap[a], b, remap[s], now, gap) for a, b, s, now, gap in ent]
    assert device_got(c, mine, 8, 1) == want
    # unrelated searches, larger and smaller, then the same again
    assert isinstance(c.place_search([(3, 0, 0, 1e6, -1.0)] * 5), list)
    device_got(c, [(3, 2, 0, 1e6, -1.0), (0, 7, 0, 7.0, 1.0)], 8, 0), device_got(c, [(3, 0, 2, 1e6, -1.0)], 1, 9)
    assert device_got(c, mine, 8, 1) == want
    # releasing slot 0 moves the other slots' blocks in the arena
    used = c.archive_usage()[0]
    c.archive_release_slots([0])
    assert c.archive_usage()[0] < used
    assert device_got(c, mine, 8, 1) == want
    c.close()


def test_refusals_change_nothing(pkg, ieskf):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=2, max_targets=1024)
    c.archive_init(2, 32, 1 << 14)
    good = [(1, 0, 0, 50.0, -1.0)]
    assert c.place_topk(good, 4, 4) == E_STATE  # before lins_place_init
    assert c.place_init() == 0
    push(c, 0, range(25)), push(c, 1, [40], t0=50.0)
    want = device_got(c, good, 4, 2)
    assert c.place_stats()["frames_built"] == 26
    for k, sep in ((0, 0), (9, 0), (-1, 0), (4, -1)):
        assert c.place_topk(good, k, sep) == E_ARG, (k, sep)
    for bad, rc in (((2, 0, 0, 50.0, -1.0), E_ARG), ((1, 0, -1, 50.0, -1.0), E_ARG), ((1, 1, 0, 50.0, -1.0), E_ARG),
                    ((1, 0, 0, float("inf"), -1.0), E_INPUT), ((1, 0, 0, 50.0, float("nan")), E_INPUT)):
        assert c.place_topk(good + [bad], 4, 2) == rc, bad  # (the good entry in front of it is not run either)
    assert device_got(c, good, 4, 2) == want and c.place_stats()["frames_built"] == 0
    s = c.place_search(good)[0]
    assert want[0][0][0] == (tk.bits(s["distance"]), s["id"], s["shift"])
    assert c.place_select_ms() == 0  # (the search ran no select)
    c.close()
