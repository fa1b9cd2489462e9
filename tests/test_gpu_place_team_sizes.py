"""lins_place_team_topk_batch (include/lins_team.h; team_kernels.hip: key, shortlist, merge, pair) past one workgroup of
candidates and at the ends of its keys' range, on the layouts of tests/team_sizes_cases.py: the device against its
definition on the CPU, lins_host_place_team_topk, against the numpy statement of tests/team_cases.py
(tests/test_place_team_sizes_host.py holds the two to each other without a GPU).  Everything compared is an integer or
the bits of an f32.

What the room fixture of tests/test_gpu_place_team.py (at most 37 candidates) cannot show and these do: a lane of the
shortlist kernel that forms three keys and walks over an empty and a one-frame slot between them; live keys in every wave,
so that the cross-wave step of the workgroup's minimum decides; chunk edges on, before and behind every target boundary
and the block size; empty slots at the front, in the middle and at the end of the target list, and 300 targets; the
candidate whose shortlist key is 0; descriptors with no cell and with every cell; slot numbers above 255; and the cut of
the shortlist at position M, which ranks of M <= 8 show whole and layout B shows at M = 63 / 64."""
import pytest

import place_topk_cases as tk
import team_cases as tc
import team_sizes_cases as ts

pytestmark = pytest.mark.gpu
team = tc.team
# a chunk edge on, before and behind the block size, each target boundary (places 1, 301, 558) and the total (622)
CHUNKS = (1, 255, 256, 257, 300, 301, 302, 557, 558, 621, 622, 623)
ONE = tk.bits(1.0)


def context(pkg, ieskf, layout, n_slots, max_frames):
    L = layout()
    frames = [(s, i, ts.frame_of(nm)) for s, names in L.items() for i, nm in enumerate(names)]
    cap = sum(len(x) for _, _, f in frames for x in f) + 256 * len(frames)
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    c.archive_init(n_slots, max_frames, cap)
    assert c.place_init() == 0
    for s, i, f in frames:
        c.archive_push(s, *f, ts.POSE, time=float(i))
    return c


@pytest.fixture(scope="module")
def arch_a(pkg, ieskf):
    """layouts A, B and C"""
    c = context(pkg, ieskf, ts.layout_a, ts.A_SLOTS, ts.A_MAX_FRAMES)
    yield c
    c.close()


@pytest.fixture(scope="module")
def arch_d(pkg, ieskf):
    c = context(pkg, ieskf, ts.layout_d, ts.D_SLOTS, ts.D_MAX_FRAMES)
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


def host_want(layout, queries, targets, M, k, sep):
    """the definition's answer with the target list as given, held to the numpy statement"""
    want = [ts.host_got(layout, q, targets, M, k, sep) for q in queries]
    assert want == [ts.want(layout, q, targets, M, k, sep) for q in queries]
    return want


def check(c, layout, queries, targets, M, k, sep):
    got, want = device_got(c, queries, targets, M, k, sep), host_want(layout, queries, targets, M, k, sep)
    assert got == want, (layout, targets[:8], M, k, sep, [(q, g, w) for q, g, w in zip(queries, got, want) if g != w][:2])
    return got


def filled(ranks):
    return sum(r != tc.UNFILLED for r in ranks)


@pytest.mark.parametrize("k", ts.KS)
def test_every_size_at_every_chunk(arch_a, k):
    """622 candidates: at the default chunk a lane strides three times, over slot 1 (empty) and slot 0 (one frame)"""
    base = {}
    for M in ts.MS:
        for sep in ts.SEPS:
            base[M, sep] = check(arch_a, "A", ts.A_QUERIES, ts.A_ALL, M, k, sep)
            st = team.stats(arch_a)
            assert st["scanned"] == len(ts.A_QUERIES) * ts.A_TOTAL and st["shortlist_ms"] > 0 and st["pair_ms"] > 0
    try:
        for chunk in CHUNKS:
            assert team.set_chunk(arch_a, chunk) == 0
            for M in ts.MS:
                assert device_got(arch_a, ts.A_QUERIES, ts.A_ALL, M, k, 2) == base[M, 2], (chunk, M)
            assert team.stats(arch_a)["scanned"] == len(ts.A_QUERIES) * ts.A_TOTAL
    finally:
        assert team.set_chunk(arch_a, 0) == 0
    assert device_got(arch_a, ts.A_QUERIES, ts.A_ALL, 64, k, 2) == base[64, 2]
    # the admissible counts: the gate of the query inside slot 2 takes out ids 250 .. 262, the one inside slot 4 itself
    assert [cand for _, cand in base[64, 0]] == [622] * 5 + [622 - 13, 621]


def test_the_target_lists_shape(arch_a):
    base = check(arch_a, "A", ts.A_QUERIES, ts.A_ALL, 11, 8, 2)
    for order in (ts.A_ALL[::-1], [4, 0, 6, 2, 5, 1, 3]):
        assert check(arch_a, "A", ts.A_QUERIES, order, 11, 8, 2) == base, order
    # empty slots in front, behind, and nothing but empty slots
    only2 = check(arch_a, "A", ts.A_QUERIES, [2], 11, 8, 2)
    assert check(arch_a, "A", ts.A_QUERIES, [1, 3, 2], 11, 8, 2) == only2
    assert check(arch_a, "A", ts.A_QUERIES, [2, 6], 11, 8, 2) == only2
    assert check(arch_a, "A", ts.A_QUERIES, [1, 3, 6], 11, 8, 2) == [([tc.UNFILLED] * 8, 0)] * len(ts.A_QUERIES)
    assert team.stats(arch_a)["scanned"] == 0
    for chunk in (1, 299, 300):
        try:
            assert team.set_chunk(arch_a, chunk) == 0
            assert device_got(arch_a, ts.A_QUERIES, [1, 3, 2], 11, 8, 2) == only2 and device_got(arch_a, ts.A_QUERIES, [2, 6], 11, 8, 2) == only2
            assert device_got(arch_a, ts.A_QUERIES, [4, 0, 6, 2, 5, 1, 3], 11, 8, 2) == base
        finally:
            assert team.set_chunk(arch_a, 0) == 0
    # the queries inside slots 2 and 4 never return their own frame nor a gated one
    for (ranks, _), q in zip(base[5:], ts.A_QUERIES[5:]):
        assert filled(ranks) == 8 and all(not (r[0] == q[0] and not abs(r[1] - q[2]) > q[3]) for r in ranks)


def test_the_whole_shortlist_shows_and_its_cut_decides(arch_a):
    d_near, d_nearer = ts.crafted()
    near = ts.NEAR + (0, d_near, 1)
    try:
        for chunk in (0, 256, 1):
            assert team.set_chunk(arch_a, chunk) == 0
            # k = 8 ranks without separation are the whole shortlist of M <= 8: the first M tuples of the numpy sort
            for M in range(1, 9):
                got = check(arch_a, "A", ts.A_QUERIES, ts.A_ALL, M, 8, 0)
                for q, (ranks, cand) in zip(ts.A_QUERIES, got):
                    order = ts.ranked("A", q, tuple(ts.A_ALL))
                    assert ts.shortlisted(ranks) == order[:M] and cand == len(order), (chunk, M, q)
            # the candidate whose shortlist key is 0 — dk 0, slot 0, id 0 — leads, and the seven behind it are right
            got = device_got(arch_a, ts.A_QUERIES[:1], ts.A_ALL, 8, 8, 0)[0][0]
            assert got[0] == (0, 0, 0, 0, 0) and ts.shortlisted(got) == ts.ranked("A", ts.A_QUERIES[0], tuple(ts.A_ALL))[:8]
            # layout B: near is position 63 of the shortlist and the best of it; nearer, position 64, would beat it
            (at64, _), = check(arch_a, "A", [ts.Q_B], ts.A_ALL, 64, 8, 0)
            assert at64[0] == near and all(r[:2] != ts.NEARER for r in at64) and all(r[:2] in ts.SAME and r[4] == 0 for r in at64[1:])
            (at63, _), = check(arch_a, "A", [ts.Q_B], ts.A_ALL, 63, 8, 0)
            assert near not in at63 and all(r[:2] in ts.SAME and r[4] == 0 for r in at63) and at63[:7] == at64[1:]
            assert d_nearer < d_near
    finally:
        assert team.set_chunk(arch_a, 0) == 0


def test_keys_at_the_ends_of_their_range(arch_a):
    L = ts.layout_a()
    for s in ts.C_SLOTS:
        for i, nm in enumerate(L[s]):
            occ, sq, t = team.key(arch_a, s, i)
            want, want_sq = team.host_ring_key(tc._DESCS[nm])
            assert occ.tolist() == want.tolist() and sq == want_sq and t == float(i), nm
            assert occ.tolist() == tc.ring_key(arch_a.place_descriptor(s, i))[0].tolist() == tc.ring_key(tc._DESCS[nm])[0].tolist()
    e, f = ts.C_NAMES.index("empty"), ts.C_NAMES.index("full")
    assert team.key(arch_a, ts.C_SLOTS[0], e)[1] == 0 and team.key(arch_a, ts.C_SLOTS[0], f)[1] == 72000
    for M, k in ((64, 8), (11, 8), (2, 1)):
        got = check(arch_a, "A", ts.C_QUERIES, ts.C_SLOTS, M, k, 0)
    got = check(arch_a, "A", ts.C_QUERIES, ts.C_SLOTS, 64, 8, 0)
    assert [cand for _, cand in got] == [11] * 6 + [12]
    # the full frame asks: its twin in the other slot at dk 0 and d 0; the frame less a ring at 3 600 in both slots
    assert got[f][0][0] == (ts.C_SLOTS[1], 5 - f, 0, 0, 0) and sorted(r[4] for r in got[f][0])[:3] == [0, 3600, 3600]
    # the empty frame asks: every d is 1, the ranks are the shortlist's order, which ends at dk 72 000
    for ranks, q in ((got[e][0], ts.C_QUERIES[e]), (got[-1][0], ts.C_QUERIES[-1])):
        assert all(r[2:4] == (0, ONE) for r in ranks) and [(r[4], r[0], r[1]) for r in ranks] == ts.ranked("A", q, ts.C_SLOTS)[:8]
    assert got[e][0][0][4] == 0 and ts.ranked("A", ts.C_QUERIES[e], ts.C_SLOTS)[-1][0] == 72000
    # one slot of the pair alone: six candidates, so eight ranks return every one — each dk between 0 and 72 000 shows
    alone = check(arch_a, "A", ts.C_QUERIES[:6], ts.C_SLOTS[1:], 64, 8, 0)
    for i, (ranks, cand) in enumerate(alone):
        assert cand == 6 and sorted((r[4], r[1]) for r in ranks[:6]) == sorted((ts.c_dk(i, 5 - c), c) for c in range(6)), i
    assert alone[e][0][5][2:] == (0, ONE, 72000) and alone[f][0][5] == (ts.C_SLOTS[1], 5 - e, 0, ONE, 72000)
    # the empty frame of slot 7 against layout A: d = 1 for each of the 622
    (ranks, cand), = check(arch_a, "A", ts.A_QUERIES[4:5], ts.A_ALL, 64, 8, 0)
    assert cand == 622 and all(r[2:4] == (0, ONE) for r in ranks)


def test_the_pair_kernels_passes(arch_a):
    """a workgroup of the pair kernel takes ten shortlist positions: M at the passes' edges, every position filled; and
    fewer candidates than M, so that a middle pass holds empty positions and later passes nothing else"""
    for M in (9, 10, 11, 20, 21, 63):
        assert all(filled(ranks) == 8 for ranks, _ in check(arch_a, "A", ts.A_QUERIES, ts.A_ALL, M, 8, 0))
    inside5 = (5, 40, 40.0, 3.0)  # its gate takes out ids 37 .. 43
    got = check(arch_a, "A", ts.A_QUERIES[:5] + [inside5], [0, 5], 64, 8, 0)
    assert [cand for _, cand in got] == [65] * 5 + [65 - 7] and all(filled(ranks) == 8 for ranks, _ in got)
    got = check(arch_a, "A", ts.A_QUERIES[:5] + [inside5], [0], 21, 8, 0)
    assert all(cand == 1 and filled(ranks) == 1 and ranks[0][:2] == (0, 0) for ranks, cand in got)
    got = check(arch_a, "A", [inside5], [5], 64, 8, 50)  # 57 candidates of one slot of 64 frames, ranks at least 51 ids apart
    assert got[0][1] == 57 and 1 <= filled(got[0][0]) <= 2


def test_300_targets_and_slots_above_255(arch_d):
    for targets in (ts.D_ALL, ts.D_SHUFFLED, ts.D_ENDS_EMPTY):
        for M, sep in ((8, 0), (21, 2), (64, 0)):
            got = check(arch_d, "D", ts.D_QUERIES, targets, M, 8, sep)
            assert [cand for _, cand in got] == [450] * 3 + [448]
            assert team.stats(arch_d)["scanned"] == len(ts.D_QUERIES) * ts.D_TOTAL
    base = check(arch_d, "D", ts.D_QUERIES, ts.D_ALL, 21, 8, 2)
    assert check(arch_d, "D", ts.D_QUERIES, ts.D_SHUFFLED, 21, 8, 2) == base == check(arch_d, "D", ts.D_QUERIES, ts.D_ENDS_EMPTY, 21, 8, 2)
    assert any(r[0] > 255 for ranks, _ in base for r in ranks)
    # two slots with an empty one between them, in every order
    for targets in (ts.D_PAIR, ts.D_PAIR[::-1], [260, 263, 257]):
        got = check(arch_d, "D", ts.D_QUERIES, targets, 21, 8, 0)
        assert all(cand == 4 and filled(ranks) == 4 for ranks, cand in got)
    for M in range(1, 9):
        for q, (ranks, _) in zip(ts.D_QUERIES, check(arch_d, "D", ts.D_QUERIES, ts.D_ALL, M, 8, 0)):
            assert ts.shortlisted(ranks) == ts.ranked("D", q, tuple(ts.D_ALL))[:M], (M, q)
    try:
        for chunk in (1, 256, 449, 450):
            assert team.set_chunk(arch_d, chunk) == 0
            assert device_got(arch_d, ts.D_QUERIES, ts.D_SHUFFLED, 21, 8, 2) == base, chunk
    finally:
        assert team.set_chunk(arch_d, 0) == 0


def test_batches_and_history_give_the_same_bits(arch_a):
    Q = ts.A_QUERIES
    base = check(arch_a, "A", Q, ts.A_ALL, 21, 8, 2)
    assert device_got(arch_a, Q[::-1], ts.A_ALL, 21, 8, 2) == base[::-1]
    for i, q in enumerate(Q):
        assert device_got(arch_a, [q], ts.A_ALL, 21, 8, 2) == [base[i]], q
    # after a call on layout C's slots (other targets, fewer candidates, another M), and after a call with one candidate
    check(arch_a, "A", ts.C_QUERIES, ts.C_SLOTS, 64, 8, 0)
    assert device_got(arch_a, Q, ts.A_ALL, 21, 8, 2) == base
    device_got(arch_a, Q[:2], [0], 1, 1, 0)
    assert device_got(arch_a, Q, ts.A_ALL, 21, 8, 2) == base
