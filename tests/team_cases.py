"""Shared by the team-search tests (tests/test_place_team_host.py on the CPU, tests/test_gpu_place_team.py on the
device; not a test): an independent numpy statement of include/lins_team.h's contract, and the device fixture.

The statement is written from the contract, not from the library's text: the ring key is a count over a boolean array,
the key distance a sum of squared differences, the shortlist and the ranks come from SORTING tuples where the libraries
take minima of packed words.  Only the f32 distance of a pair is taken from the library (host.place_distance — pinned by
tests/test_place_host.py against its own numpy statement)."""
import functools
import importlib

import numpy as np

import place_loop_cases as plc
import place_topk_cases as tk

PKG = "lins---lidar-inertial-slam_amd"
host = importlib.import_module(PKG + ".host")
team = importlib.import_module(PKG + ".team")
F = np.float32
UNFILLED = (-1, -1, 0, tk.bits(1.0), -1)


def ring_key(D):
    occ = (np.asarray(D, F).reshape(20, 60) > 0).sum(axis=1)
    return occ, int((occ * occ).sum())


def key_distance(D_q, D_c):
    return int(((ring_key(D_q)[0] - ring_key(D_c)[0]) ** 2).sum())


def admissible(slot, c, time_c, query_slot, query_id, now, gap):
    return slot != query_slot or (c != query_id and abs(time_c - now) > gap)


@functools.lru_cache(maxsize=None)
def _pair(key_q, key_c):
    """(bits of the smallest d, the smallest shift that gives it) of a pair of descriptors named by hashable keys"""
    d = host.place_distance(_DESCS[key_q], _DESCS[key_c])
    s = int(np.argmin(d))
    return tk.bits(d[s]), s


_DESCS = {}


def want(name_q, query_slot, query_id, now, gap, targets, M, k, min_sep):
    """targets: [(slot, [descriptor names], times)] with the descriptors registered in _DESCS.  -> ([k tuples (slot, id,
    shift, bits(d), dk), the unfilled ones included], admissible candidates)"""
    cands = []
    for slot, names, times in targets:
        for c, name in enumerate(names):
            if admissible(slot, c, times[c], query_slot, query_id, now, gap):
                cands.append((key_distance(_DESCS[name_q], _DESCS[name]), slot, c, name))
    short = sorted(cands)[:M]
    rows = []
    for m, (dk, slot, c, name) in enumerate(short):
        b, shift = _pair(name_q, name)
        rows.append((b, m, shift, dk, slot, c))
    rows.sort()  # (bits of d, shortlist position, shift)
    ranks = []
    for b, m, shift, dk, slot, c in rows:
        if len(ranks) == k:
            break
        if all(not (slot == r[0] and abs(c - r[1]) <= min_sep) for r in ranks):
            ranks.append((slot, c, shift, b, dk))
    return ranks + [UNFILLED] * (k - len(ranks)), len(cands)


def as_tuples(raw):
    """team.topk / team.host_topk raw records -> [(slot, id, shift, bits(d), dk)]"""
    return [(r["slot"], r["id"], r["shift"], tk.bits(r["distance"]), r["dk"]) for r in raw]


# ---- the CPU cases: slots of the top-K tests' pool (exact duplicates between its laps) ----
def pool_slot(first, n):
    """n frames of the pool from frame `first` on: (descriptor names, times 0, 1, ..)"""
    names = [("pool", first + i) for i in range(n)]
    for nm in names:
        _DESCS.setdefault(nm, tk.desc(nm[1]))
    return names, np.arange(n, dtype=np.float64)


def register(name, D):
    _DESCS.setdefault(name, np.asarray(D, F).reshape(20, 60))
    return name


def host_got(name_q, query_slot, query_id, now, gap, targets, M, k, min_sep):
    tg = [(slot, [_DESCS[nm] for nm in names], times) for slot, names, times in targets]
    raw, filled = team.host_topk(_DESCS[name_q], query_slot, query_id, now, gap, tg, raw=True, shortlist=M, k=k, min_sep=min_sep)
    got = as_tuples(raw)
    assert all(x == UNFILLED for x in got[filled:]) and all(x != UNFILLED for x in got[:filled])
    assert len({r["candidates"] for r in raw}) == 1
    return got, raw[0]["candidates"]


# ---- the device fixture: the room frames of tests/place_loop_cases.py in three slots, twelve frames each ----
N_FRAMES, UP = plc.N, plc.UP
SLOTS = (0, 1, 2)
EXTRA = 3  # a fourth slot with ONE frame, so that target lists of 36 and of 37 candidates exist


@functools.lru_cache(maxsize=None)
def room_slots():
    """slot -> [(corner, surf, outlier, pose)]: slot 0 the case's own frames; slot 1 another robot's drive through the same
    room (its own trajectory and scans); slot 2 slot 0's frames five ids on, bit for bit — every query ties on dk and on d
    between slots 0 and 2; the extra slot: slot 1's frame 4 again"""
    import local_map_synth as lms

    a = [f for f in plc.case()[0]]
    poses = lms.trajectory(N_FRAMES, seed=plc.SEED + 1)
    b = [plc.scan(8000 + i, poses[i]) + (poses[i],) for i in range(N_FRAMES)]
    c = [a[(i + 5) % N_FRAMES] for i in range(N_FRAMES)]
    return {0: a, 1: b, 2: c, EXTRA: [b[4]]}


@functools.lru_cache(maxsize=None)
def room_descs():
    """slot -> descriptor names, registered: the CPU restatement's descriptors of the fixture's frames"""
    prm = host.place_params(up_axis=UP)
    return {s: [register(("room", s, i), host.place_descriptor(*f[:3], params=prm)) for i, f in enumerate(fr)] for s, fr in room_slots().items()}


def room_targets(slots, counts=None):
    names = room_descs()
    return [(s, names[s][:(counts or {}).get(s, len(names[s]))], np.arange(len(names[s]), dtype=np.float64)) for s in slots]
