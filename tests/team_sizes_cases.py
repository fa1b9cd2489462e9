"""Shared by the team search's size tests (tests/test_place_team_sizes_host.py on the CPU, tests/test_gpu_place_team_sizes.py
on the device; not a test): archives large enough that a lane of the shortlist kernel strides more than once, that keys
live in every wave, that target lists have empty slots at the front, in the middle and at the end, and frames at the ends
of the key's range.  Every descriptor is registered in team_cases._DESCS, so team_cases.want (the numpy statement) and
team_cases.host_got serve unchanged; both are memoised here, a reference is computed once.

Layout A  one archive, max_frames 300: slot 0 one frame | 1 none | 2 300 | 3 none | 4 257 | 5 64 | 6 none | 7 the queries.
          Target list [0 .. 6]: 622 candidates, target boundaries at places 1, 301 and 558.  Frames of 20 .. 400 points cut
          to 150; 45 frames are bit-for-bit repeats in another slot; slot 0's frame is the twin of query 0, the candidate
          whose shortlist key is 0.
Layout B  inside layout A's slots 2, 4 and 5: for the query Q (slot 7, id 3) 63 frames with exactly Q's cells and other
          heights (dk 0, d large; places >= 256 and >= 512 of the concatenation), `near` (Q less one point of a column
          that keeps others: dk 1, d tiny) and `nearer` (Q less two points that were alone in their columns, in two rings:
          dk 2, the columns left compare equal).  So near is the 64th of the shortlist and nearer the 65th: the cut at
          position M is visible in rank 0.  crafted() asserts all of it from the numpy statement.
Layout C  slots 8 and 9 of the same archive (so that a call on it is history for layout A's): the empty frame, one point,
          one column, the floor's edge, a point in every cell, and that less one ring; slot 9 the same in reverse.
Layout D  a second archive: 302 slots, max_frames 4, slot s < 300 holds (7 s) % 4 frames of the top-K pool (its laps
          repeat: dk ties that the slot decides), 450 candidates; slot 300 is empty, the queries lie in slot 301.
          ((7 s) % 4 is 0 for every fourth slot, slot 0 among them; slot 299 holds one frame, so the ascending list ends
          in a one-frame slot, and ENDS_EMPTY is the list that ends in an empty one.)"""
import functools

import numpy as np

import place_cases as pc
import place_topk_cases as tk
import team_cases as tc

host = tc.host
F = np.float32
MS, KS, SEPS = (1, 2, 7, 8, 9, 10, 11, 20, 21, 63, 64), (1, 8), (0, 2)
POSE = (0.5, -1.0, 0.2, 0.01, -0.02, 0.4)

# ---- layouts A, B, C: one archive ----
A_SLOTS, A_MAX_FRAMES = 10, 300
A_COUNTS = {0: 1, 1: 0, 2: 300, 3: 0, 4: 257, 5: 64, 6: 0}
A_ALL = [0, 1, 2, 3, 4, 5, 6]
A_TOTAL = 622
A_FIRST = {0: 0, 2: 1, 4: 301, 5: 558}  # a slot's first place in the default list's concatenation
A_QS = 7
C_SLOTS = (8, 9)
NEAR, NEARER = (4, 250), (2, 5)  # (slot, id)
SAME = [(2, 262 + i) for i in range(21)] + [(4, 215 + i) for i in range(21)] + [(5, 20 + i) for i in range(21)]
Q_B = (A_QS, 3, 1e6, -1.0)
# (slot, id, now, gap): query 0 the twin of slot 0's frame; 1 a revisit of slot 2's frame 40; 2 slot 2's frame 110 = slot
# 4's frame 10 bit for bit; 3 layout B's Q; 4 the empty frame; a frame inside slot 2 whose gate takes out ids 250 .. 262,
# places on both sides of a lane's first stride; a frame inside slot 4 (its twin is slot 5's frame 0)
A_QUERIES = [(A_QS, 0, 1e6, -1.0), (A_QS, 1, 1e6, -1.0), (A_QS, 2, 1e6, -1.0), Q_B, (A_QS, 4, 1e6, -1.0), (2, 256, 256.0, 6.0), (4, 100, 100.0, -1.0)]
C_NAMES = ("empty", "single", "one_column", "floor", "full", "full_less_ring")
C_QUERIES = [(C_SLOTS[0], i, float(i), -1.0) for i in range(len(C_NAMES))] + [(A_QS, 4, 1e6, -1.0)]

_SEED_B, _N_B = 4242, 140


@functools.lru_cache(maxsize=None)
def _q_cells():
    """Q's cells: 140 distinct ones -> (ring, sector)"""
    cells = np.random.default_rng(_SEED_B).choice(pc.NR * pc.NS, _N_B, replace=False)
    return cells // pc.NS, cells % pc.NS


def _q_cloud(height_seed, drop=()):
    """a point at the centre of each of Q's cells, heights drawn from height_seed, the points `drop` left out"""
    ring, sec = _q_cells()
    h = np.random.default_rng(height_seed).uniform(0.5, 6.0, _N_B)
    keep = np.ones(_N_B, bool)
    keep[list(drop)] = False
    return pc.polar_cloud((ring[keep] + 0.5) * pc.DR, -np.pi + (sec[keep] + 0.5) * pc.DS, h[keep])


@functools.lru_cache(maxsize=None)
def _removals():
    """(near's point, nearer's two points): one of a column that holds others; two alone in their columns, in two rings"""
    ring, sec = _q_cells()
    per_col = np.bincount(sec, minlength=pc.NS)
    shared = [i for i in range(_N_B) if per_col[sec[i]] >= 3]
    alone = [i for i in range(_N_B) if per_col[sec[i]] == 1]
    b = alone[0]
    c = next(i for i in alone[1:] if ring[i] != ring[b])
    return shared[0], (b, c)


def _full(less_ring=None):
    ring, sec = np.divmod(np.arange(pc.NR * pc.NS), pc.NS)
    keep = ring != less_ring
    h = 0.5 + 5.0 * ((ring * 7 + sec * 3) % 11) / 11.0
    return pc.polar_cloud((ring[keep] + 0.5) * pc.DR, -np.pi + (sec[keep] + 0.5) * pc.DS, h[keep])


@functools.lru_cache(maxsize=None)
def frame_of(name):
    """the (corner, surf, outlier) a name stands for"""
    kind = name[0]
    if kind == "v":  # the varied pool: 20 .. 400 points, cut to 150
        return pc.frame(pc.place(7000 + name[1], n=20 + (name[1] * 37) % 381)[:150])
    if kind == "rev":  # the same place seen again
        return pc.frame(pc.place(7000 + name[1], n=20 + (name[1] * 37) % 381, jitter=0.02, drop=0.05)[:150])
    if kind == "Q":
        return pc.frame(_q_cloud(_SEED_B))
    if kind == "same":
        return pc.frame(_q_cloud(_SEED_B + 1 + name[1]))
    if kind == "near":
        return pc.frame(_q_cloud(_SEED_B, drop=(_removals()[0],)))
    if kind == "nearer":
        return pc.frame(_q_cloud(_SEED_B, drop=_removals()[1]))
    if kind == "edge":
        return pc.edge_frames()[name[1]]
    if kind == "full":
        return pc.frame(_full())
    if kind == "full_less_ring":
        return pc.frame(_full(less_ring=13))
    if kind == "pool":
        return tk.frame(name[1])
    if kind == "query":
        return tk.query_frame(name[1])
    raise KeyError(name)


def named(name):
    """registers the name's descriptor (the CPU restatement's) and returns the name"""
    if name not in tc._DESCS:
        tc.register(name, host.place_descriptor(*frame_of(name)))
    return name


def _c_name(n):
    return (n,) if n.startswith("full") else ("edge", n)


@functools.lru_cache(maxsize=None)
def layout_a():
    """slot -> [names] of the archive of layouts A, B and C"""
    s2 = [("v", i) for i in range(300)]
    s4 = [("v", 300 + i) for i in range(257)]
    s5 = [("v", 600 + i) for i in range(64)]
    for i in range(30):
        s4[i] = s2[100 + i]
    for i in range(15):
        s5[i] = s4[100 + i]
    by_slot = {2: s2, 4: s4, 5: s5}
    for i, (s, c) in enumerate(SAME):
        by_slot[s][c] = ("same", i)
    s4[NEAR[1]], s2[NEARER[1]] = ("near",), ("nearer",)
    cs = [_c_name(n) for n in C_NAMES]
    slots = {0: [("v", 900)], 1: [], 2: s2, 3: [], 4: s4, 5: s5, 6: [], A_QS: [("v", 900), ("rev", 40), s2[110], ("Q",), ("edge", "empty")],
             C_SLOTS[0]: cs, C_SLOTS[1]: cs[::-1]}
    assert all(len(slots[s]) == n for s, n in A_COUNTS.items()) and sum(A_COUNTS.values()) == A_TOTAL
    return {s: [named(n) for n in names] for s, names in slots.items()}


# ---- layout D ----
D_SLOTS, D_MAX_FRAMES, D_TARGETS, D_QS = 302, 4, 300, 301
D_ALL = list(range(D_TARGETS))
D_SHUFFLED = [int(s) for s in np.random.default_rng(11).permutation(D_TARGETS)]
D_ENDS_EMPTY = list(range(1, D_TARGETS)) + [0]
D_PAIR = [257, 260, 263]  # three frames | none | one frame
D_TOTAL = 450
# the top-K tests' revisit of place 3, their pool frame 5 bit for bit (in several slots), pool frame 40; a frame inside slot
# 297 gated by time (its id 0 is inside the gap and out, id 2 is in)
D_QUERIES = [(D_QS, 0, 1e6, -1.0), (D_QS, 1, 1e6, -1.0), (D_QS, 2, 1e6, -1.0), (297, 1, 0.0, 0.5)]


@functools.lru_cache(maxsize=None)
def layout_d():
    slots = {s: [("pool", (4 * s + i) % 148) for i in range((7 * s) % 4)] for s in range(D_SLOTS - 1)}
    slots[D_QS] = [("query", 0), ("query", 1), ("pool", 40)]
    assert sum(len(slots[s]) for s in D_ALL) == D_TOTAL and not slots[0] and not slots[300] and len(slots[299]) == 1 and len(slots[297]) == 3
    return {s: [named(n) for n in names] for s, names in slots.items()}


LAYOUTS = {"A": layout_a, "D": layout_d}


def targets_of(layout, slots):
    """[(slot, names, times)]: a frame's time is its id"""
    L = LAYOUTS[layout]()
    return [(s, L[s], np.arange(len(L[s]), dtype=np.float64)) for s in slots]


@functools.lru_cache(maxsize=None)
def _want(layout, q, slots, M, k, sep):
    qs, qid, now, gap = q
    return tc.want(LAYOUTS[layout]()[qs][qid], qs, qid, now, gap, targets_of(layout, slots), M, k, sep)


@functools.lru_cache(maxsize=None)
def _host(layout, q, slots, M, k, sep):
    qs, qid, now, gap = q
    return tc.host_got(LAYOUTS[layout]()[qs][qid], qs, qid, now, gap, targets_of(layout, slots), M, k, sep)


def want(layout, q, slots, M, k, sep):
    """the numpy statement -> ([k tuples (slot, id, shift, bits(d), dk)], admissible candidates).  It sorts: the order of
    the target list cannot matter to it"""
    return _want(layout, q, tuple(sorted(slots)), M, k, sep)


def host_got(layout, q, slots, M, k, sep):
    """lins_host_place_team_topk with the target list in the order given"""
    return _host(layout, q, tuple(slots), M, k, sep)


@functools.lru_cache(maxsize=None)
def ranked(layout, q, slots):
    """the admissible candidates' (dk, slot, id), sorted: the numpy statement's shortlist order"""
    qs, qid, now, gap = q
    name_q = LAYOUTS[layout]()[qs][qid]
    return sorted((tc.key_distance(tc._DESCS[name_q], tc._DESCS[nm]), s, c) for s, names, times in targets_of(layout, slots)
                  for c, nm in enumerate(names) if tc.admissible(s, c, times[c], qs, qid, now, gap))


def shortlisted(ranks):
    """the filled ranks of a result as (dk, slot, id), sorted"""
    return sorted((r[4], r[0], r[1]) for r in ranks if r != tc.UNFILLED)


@functools.lru_cache(maxsize=None)
def crafted():
    """asserts what layouts A and B were built for, from the numpy statement alone -> (bits of near's d, of nearer's d)"""
    L = layout_a()
    # A: the repeats, and the candidate with shortlist key 0
    where = {}
    for s in A_ALL:
        for c, nm in enumerate(L[s]):
            where.setdefault(nm, []).append((s, c))
    assert sum(len({s for s, _ in at}) > 1 for at in where.values()) >= 40
    assert ranked("A", A_QUERIES[0], tuple(A_ALL))[0] == (0, 0, 0)
    dks = [r[0] for r in ranked("A", A_QUERIES[1], tuple(A_ALL))]
    assert len(set(dks)) >= 100 and dks[-1] >= 20 * max(dks[0], 1)  # (dk spreads widely)
    # B: the 63 frames of Q's cells lead at dk 0, near is position 63, nearer position 64
    order = ranked("A", Q_B, tuple(A_ALL))
    assert len(order) == A_TOTAL
    assert sorted(order[:63]) == sorted((0,) + sc for sc in SAME)
    assert order[63] == (1,) + NEAR and order[64] == (2,) + NEARER and order[65][0] > 2
    assert all(A_FIRST[s] + c >= 256 for s, c in SAME) and sum(A_FIRST[s] + c >= 512 for s, c in SAME) == 42 and A_FIRST[NEAR[0]] + NEAR[1] >= 512
    d_near, d_nearer = tc._pair(L[A_QS][3], L[NEAR[0]][NEAR[1]])[0], tc._pair(L[A_QS][3], L[NEARER[0]][NEARER[1]])[0]
    d_same = min(tc._pair(L[A_QS][3], L[s][c])[0] for s, c in SAME)
    assert d_nearer < d_near < d_same  # (bits of non-negative floats order as the floats do)
    assert want("A", Q_B, A_ALL, 64, 1, 0)[0][0][:2] == NEAR and want("A", Q_B, A_ALL, 64, 1, 0)[0][0][4] == 1
    return d_near, d_nearer


def c_dk(i, j):
    """the key distance of layout C's frames i and j, from their occupancies"""
    cs = layout_a()[C_SLOTS[0]]
    return tc.key_distance(tc._DESCS[cs[i]], tc._DESCS[cs[j]])
