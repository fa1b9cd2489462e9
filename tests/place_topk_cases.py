"""Shared by the top-K place tests (tests/test_place_topk_host.py on the CPU, tests/test_gpu_place_topk.py on the device;
not a test): a pool of small frames with exact duplicates, and an independent numpy statement of the selection — SORT
the candidates' row keys, then one greedy pass with the separation rule — where the libraries take K separated minima."""
import functools
import importlib

import numpy as np

import place_cases as pc

PKG = "lins---lidar-inertial-slam_amd"
host = importlib.import_module(PKG + ".host")
F = np.float32
PLACES = 37


@functools.lru_cache(maxsize=None)
def _frame(place, variant):
    """variant 0: the place as first seen (every frame of it bit for bit the same); v > 0: a revisit, turned and jittered"""
    if variant == 0:
        return pc.frame(pc.place(500 + place, n=150, turn=(5 * place) % 60))
    return pc.frame(pc.place(500 + place, n=150, turn=(5 * place + 7 * variant) % 60, jitter=0.03, drop=0.05))


def frame(i):
    """frame i of the pool: place i % 37; the laps 0, 2 and 3 are exact duplicates of one another, the others revisits"""
    lap = i // PLACES
    return _frame(i % PLACES, 0 if lap in (0, 2, 3) else lap)


@functools.lru_cache(maxsize=None)
def desc(i):
    return host.place_descriptor(*frame(i))


def descs(n):
    return [desc(i) for i in range(n)]


@functools.lru_cache(maxsize=None)
def query_frame(which=0):
    """0: a revisit of place 3; 1: frame 5 of the pool bit for bit; 2: an empty frame"""
    if which == 2:
        return pc.E, pc.E, pc.E
    return pc.frame(pc.place(503, n=150, turn=11, jitter=0.02, drop=0.05)) if which == 0 else frame(5)


@functools.lru_cache(maxsize=None)
def query_desc(which=0):
    return host.place_descriptor(*query_frame(which))


def bits(x):
    return int(np.asarray(x, F).reshape(1).view(np.uint32)[0])


@functools.lru_cache(maxsize=None)
def _pair(which, i):
    """which: a query of query_frame, or ("frame", id): frame id of the pool asks"""
    d = host.place_distance(desc(which[1]) if isinstance(which, tuple) else query_desc(which), desc(i))
    s = int(np.argmin(d))  # (the first of equal minima: the smaller shift)
    return bits(d[s]), s


def row_keys(which, n, times, now, gap, skip=-1):
    """[(bits(d), id, shift)] of the admissible candidates among the first n pool frames, query `which`"""
    keys = []
    for c in range(n):
        if c == skip or not abs(times[c] - now) > gap:
            continue
        b, s = _pair(which, c)
        keys.append((b, c, s))
    return keys


def select(keys, k, min_sep):
    """sort, then one greedy pass: a key is taken when its id lies more than min_sep from every id taken"""
    out = []
    for key in sorted(keys):
        if len(out) == k:
            break
        if all(abs(key[1] - o[1]) > min_sep for o in out):
            out.append(key)
    return out


def as_keys(ranks):
    """result dicts (id, shift, distance) -> [(bits(d), id, shift)]"""
    return [(bits(r["distance"]), r["id"], r["shift"]) for r in ranks]
