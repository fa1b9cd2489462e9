"""lins_place_team_topk_batch (include/lins_team.h; team_kernels.hip) against its definition on the CPU,
lins_host_place_team_topk, bit for bit — and through it against the numpy statement of tests/team_cases.py, which
tests/test_place_team_host.py holds the definition to.  Fixture: the room frames of tests/place_loop_cases.py in three
slots of twelve frames (slot 2 repeats slot 0's frames five ids on, so every query ties on dk and on d between two
slots), and a fourth slot with one frame so that target lists of 36 and of 37 candidates exist: the shortlist's chunk is
put at chunk - 1, chunk, chunk + 1 and 2 chunk + 1 candidates."""
import numpy as np
import pytest

import place_topk_cases as tk
import team_cases as tc

pytestmark = pytest.mark.gpu
team, host = tc.team, tc.host
N = tc.N_FRAMES
ALL3, ALL4 = [0, 1, 2], [0, 1, 2, tc.EXTRA]
MS, KS = (1, 4, 11, 36), (1, 4, 8)
E_ARG, E_CAPACITY, E_INPUT, E_STATE = -1, -3, -4, -6
# each slot's latest frame as a rendezvous asks (its own slot gated by time, AT equality for ids 8 and 14), a frame from
# the middle with every time admitted, and the one frame of the extra slot — a twin of slot 1's frame 4
QUERIES = [(0, N - 1, float(N - 1), 3.0), (1, N - 1, float(N - 1), 3.0), (2, N - 1, float(N - 1), 3.0), (1, 4, 4.0, -1.0), (tc.EXTRA, 0, 0.0, 0.0),
           (0, 5, 8.0, 3.0)]


def context(pkg, ieskf, n_slots=4, max_frames=16, cap=1 << 17):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=n_slots, max_targets=1024)
    c.streams_init(n_slots)
    c.archive_init(n_slots, max_frames, cap)
    assert c.place_init(up_axis=tc.UP) == 0
    return c


def push(c, slot, frames, t0=0.0):
    for i, f in enumerate(frames):
        c.archive_push(slot, *f[:3], tuple(float(v) for v in f[3]), time=t0 + i)


def fill(c, slots=(0, 1, 2, tc.EXTRA)):
    for s in slots:
        push(c, s, tc.room_slots()[s])


@pytest.fixture(scope="module")
def filled(pkg, ieskf):
    c = context(pkg, ieskf)
    fill(c)
    yield c
    c.close()


def device_got(c, queries, targets, M, k, sep):
    res = team.topk(c, queries, targets, raw=True, shortlist=M, k=k, min_sep=sep)
    assert isinstance(res, list) and len(res) == len(queries), res
    out = []
    for raw, n_filled in res:
        got = tc.as_tuples(raw)
        assert all(x == tc.UNFILLED for x in got[n_filled:]) and all(x != tc.UNFILLED for x in got[:n_filled])
        assert all(r["status"] == 0 and r["candidates"] == raw[0]["candidates"] for r in raw)
        out.append((got, raw[0]["candidates"]))
    return out


def host_want(q, targets, M, k, sep, counts=None):
    qs, qid, now, gap = q
    return tc.host_got(tc.room_descs()[qs][qid], qs, qid, now, gap, tc.room_targets(targets, counts), M, k, sep)


def numpy_want(q, targets, M, k, sep):
    qs, qid, now, gap = q
    return tc.want(tc.room_descs()[qs][qid], qs, qid, now, gap, tc.room_targets(targets), M, k, sep)


@pytest.mark.parametrize("k", KS)
def test_the_device_is_the_hosts_bits(filled, k):
    for M in MS:
        for sep in (0, 4):
            got = device_got(filled, QUERIES, ALL3, M, k, sep)
            want = [host_want(q, ALL3, M, k, sep) for q in QUERIES]
            assert got == want, (M, k, sep, [(q, g, w) for q, g, w in zip(QUERIES, got, want) if g != w][:2])
            assert want == [numpy_want(q, ALL3, M, k, sep) for q in QUERIES]
            st = team.stats(filled)
            assert st["scanned"] == len(QUERIES) * 36 and st["shortlist_ms"] > 0 and st["pair_ms"] > 0
    # the admissible counts: slot 0's latest frame loses itself and ids 8 .. 10 of its own slot; another slot loses nothing
    (got0, cand0), (_, _), (_, _), (_, cand3), (got4, cand4), _ = device_got(filled, QUERIES, ALL3, 36, k, 0)
    assert (cand0, cand3, cand4) == (36 - 4, 35, 36)
    # the twin of the extra slot's frame leads at d = 0, dk = 0; slot 0's frames tie with slot 2's and the lower slot leads
    assert got4[0] == (1, 4, 0, 0, 0)
    if k >= 4:
        pairs = [(a, b) for a, b in zip(got0, got0[1:]) if a[3] == b[3] and a != tc.UNFILLED]
        assert pairs and all(a[0] == 0 and b[0] == 2 and (a[1] - b[1]) % N == 5 and a[4] == b[4] for a, b in pairs)


def test_the_device_key_is_the_hosts(filled):
    for s, i in ((0, 0), (1, 7), (2, 11), (tc.EXTRA, 0)):
        occ, sq, t = team.key(filled, s, i)
        want, want_sq = team.host_ring_key(tc._DESCS[tc.room_descs()[s][i]])
        assert occ.tolist() == want.tolist() and sq == want_sq and t == float(i)
        assert occ.tolist() == tc.ring_key(filled.place_descriptor(s, i))[0].tolist()


def test_chunks_orders_batches_and_history_give_the_same_bits(filled):
    base3, base4 = device_got(filled, QUERIES, ALL3, 11, 8, 1), device_got(filled, QUERIES, ALL4, 11, 8, 1)
    assert base4 == [host_want(q, ALL4, 11, 8, 1) for q in QUERIES]
    every3, every4 = device_got(filled, QUERIES, ALL3, 36, 8, 1), device_got(filled, QUERIES, ALL4, 64, 8, 1)
    # 36 candidates at chunk - 1, chunk, chunk + 1; 37 at the same three and at 2 chunk + 1; one candidate a workgroup
    for chunk in (37, 36, 35, 38, 18, 5, 1, 0):
        assert team.set_chunk(filled, chunk) == 0
        assert device_got(filled, QUERIES, ALL3, 11, 8, 1) == base3, chunk
        assert device_got(filled, QUERIES, ALL4, 11, 8, 1) == base4, chunk
        assert device_got(filled, QUERIES, ALL3, 36, 8, 1) == every3 and device_got(filled, QUERIES, ALL4, 64, 8, 1) == every4, chunk
    # the target list in other orders
    for order in ([2, 1, 0], [1, 0, 2]):
        assert device_got(filled, QUERIES, order, 11, 8, 1) == base3, order
    assert device_got(filled, QUERIES, [tc.EXTRA, 2, 1, 0], 11, 8, 1) == base4
    # the batch reversed, each entry alone
    assert device_got(filled, QUERIES[::-1], ALL3, 11, 8, 1) == base3[::-1]
    for i, q in enumerate(QUERIES):
        assert device_got(filled, [q], ALL3, 11, 8, 1) == [base3[i]]
    # after other place calls on the same context, larger and smaller
    assert isinstance(filled.place_search([(0, 3, 1, 3.0, -1.0)] * 7), list)
    assert isinstance(filled.place_topk([(1, 2, 2, 2.0, 1.0)], 4, 2), list)
    device_got(filled, QUERIES[:2], [1], 3, 2, 0)
    assert device_got(filled, QUERIES, ALL3, 11, 8, 1) == base3
    # a subset of the slots, an empty list, no query
    assert device_got(filled, QUERIES, [1], 11, 8, 1) == [host_want(q, [1], 11, 8, 1) for q in QUERIES]
    assert device_got(filled, QUERIES[:2], [], 11, 2, 0) == [([tc.UNFILLED] * 2, 0)] * 2
    assert team.topk(filled, [], ALL3) == []


def test_everything_shortlisted_rank_0_is_the_exhaustive_search(filled):
    """M = every candidate: rank 0 is what lins_place_search_batch returns per target slot, minimised over the slots by
    (d, slot, id, shift) — the shortlist changes which candidates are compared, never how"""
    got = device_got(filled, QUERIES, ALL3, 36, 1, 0)
    for q, (ranks, cand) in zip(QUERIES, got):
        qs, qid, now, gap = q
        per_slot = filled.place_search([(qs, qid, s, now, gap if s == qs else -1.0) for s in ALL3])
        best = min((tk.bits(r["distance"]), s, r["id"], r["shift"]) for s, r in zip(ALL3, per_slot) if r["id"] >= 0)
        assert (ranks[0][3], ranks[0][0], ranks[0][1], ranks[0][2]) == best, q
        assert cand == sum(r["candidates"] for r in per_slot)


def test_keys_are_rebuilt_after_a_release_and_after_a_restore(pkg, ieskf, filled):
    want = device_got(filled, QUERIES, ALL4, 11, 8, 1)
    c = context(pkg, ieskf)
    fill(c, (0, tc.EXTRA))
    push(c, 1, tc.room_slots()[0][:7])  # other frames where slot 1's will lie
    push(c, 2, tc.room_slots()[2])
    device_got(c, QUERIES[:1] + QUERIES[2:3], ALL4, 11, 8, 1)  # (keys of the wrong frames are built)
    assert team.stats(c)["frames_keyed"] == 12 + 7 + 12 + 1
    c.archive_release_slots([1])
    push(c, 1, tc.room_slots()[1])
    assert device_got(c, QUERIES, ALL4, 11, 8, 1) == want
    assert team.stats(c)["frames_keyed"] == 12  # slot 1's only: the others kept theirs
    # snapshot slot 1, put other frames there, search, retire, restore: the keys follow the restored frames
    (blob,) = c.streams_snapshot([1])
    c.streams_retire([1])
    push(c, 1, tc.room_slots()[2][:5])
    device_got(c, QUERIES[:1], ALL4, 11, 8, 1)
    c.streams_retire([1])
    c.streams_restore([1], [blob])
    assert device_got(c, QUERIES, ALL4, 11, 8, 1) == want
    assert team.stats(c)["frames_keyed"] == 12
    # lins_place_init drops descriptors and keys alike
    assert c.place_init(up_axis=tc.UP) == 0
    assert device_got(c, QUERIES, ALL4, 11, 8, 1) == want and team.stats(c)["frames_keyed"] == 37
    c.close()


def test_refusals_change_nothing(pkg, ieskf):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=4, max_targets=1024)
    c.streams_init(4)
    c.archive_init(4, 16, 1 << 17)
    good = QUERIES[:2]
    assert team.topk(c, good, ALL3) == E_STATE  # before lins_place_init
    assert c.place_init(up_axis=tc.UP) == 0
    fill(c)
    want = device_got(c, good, ALL3, 11, 4, 1)
    assert team.stats(c)["frames_keyed"] == 36
    for kw in (dict(shortlist=0), dict(shortlist=65), dict(k=0), dict(k=9), dict(min_sep=-1)):
        assert team.topk(c, good, ALL3, **kw) == E_ARG, kw
    for targets in ([0, 4], [-1], [0, 1, 0]):
        assert team.topk(c, good, targets) == E_ARG, targets
    for bad, rc in (((4, 0, 1.0, 1.0), E_ARG), ((0, N, 1.0, 1.0), E_ARG), ((0, -1, 1.0, 1.0), E_ARG), ((0, 1, float("inf"), 1.0), E_INPUT),
                    ((0, 1, 1.0, float("nan")), E_INPUT)):
        assert team.topk(c, good + [bad], ALL3) == rc, bad
    assert device_got(c, good, ALL3, 11, 4, 1) == want and team.stats(c)["frames_keyed"] == 0
    c.close()
