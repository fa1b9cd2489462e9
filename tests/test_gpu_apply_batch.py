"""lins_pose_graph_apply_batch — the write-back of n loop closures in one call, the streams' records by one kernel
(map_pose_correct_kernel: one lane per entry, workgroups of one wave) — against n single lins_pose_graph_apply calls on a
second context: the streams' map pose records, the archive's assemblies and the rings' builds, bit for bit, for n = 1, 3
and 65 (one full wave plus one lane).  Shapes: the three tiny frames of tests/test_gpu_pose_graph.py per slot, a ring
window of 2."""
import importlib

import numpy as np
import pytest

import loop_icp_cases as licp
import pose_graph_cases as cases
from test_gpu_pose_graph import six_of_key, tiny_frames

pytestmark = pytest.mark.gpu
sm = importlib.import_module("lins---lidar-inertial-slam_amd.streams_map")
F = np.float32


def stream_of(slot, n):
    """the stream slot `slot` is written to: a permutation of the streams (7 is coprime to 1, 3 and 65), -1 for slot 1 of
    a batch of at least three"""
    return -1 if (n >= 3 and slot == 1) else (7 * slot + 3) % n


def start_pose(stream):
    """a record with every field set, different per stream"""
    v = lambda k: (np.arange(6, dtype=F) * F(0.01) + F(0.1 * k + stream)).astype(F)
    return dict(bef=v(1), aft=v(2), tobe=v(3), last=v(4), prev=v(5)[:3], n_frames=3 + stream, last_time=0.5 * stream)


def fill(c, n, ring_short=None):
    """n slots of three frames in the archive, the ring (window 2) and the graph, one loop each, solved; n streams"""
    frames = tiny_frames(3)
    c.archive_init(n, 4, n * sum(len(f[0]) + len(f[1]) + len(f[2]) for f in frames))
    c.local_map_init(n, 2, 1024)
    c.streams_init(n)
    sm.init(c, n)
    c.pose_graph_init(n, 4, 1)
    for s in range(n):
        for i, f in enumerate(frames):
            assert c.archive_push(s, *f, time=float(i)) == c.pose_graph_push(s, six_of_key(frames[i - 1][3]) if i else None, six_of_key(f[3])) == i
            if s != ring_short or i == 0:
                c.local_map_push(s, *f)
        c.pose_graph_add_loop(s, 2, 0, cases.corrected(six_of_key(frames[2][3]), 0.2 + 0.002 * s, 1.0 + 0.02 * s, 5 + s), 1e-6)
        sm.set_pose(c, s, start_pose(s))
    assert all(r["iterations"] > 0 for r in c.pose_graph_solve(list(range(n))))


def snapshot(c, n):
    scan = licp.room_scan(950, tiny_frames(3)[2][3], n_corner=40, n_surf=300, n_outlier=30)
    poses = [sm.get_pose(c, s) for s in range(n)]
    recs = [tuple(np.asarray(p[k], F).tobytes() for k in ("bef", "aft", "tobe", "last", "prev")) + (p["n_frames"], p["last_time"]) for p in poses]
    info = c.archive_assemble([dict(slot=s, ids=[0, 1, 2], clouds=7, leaf=0.4, flags=0) for s in range(n)])
    archive = [(info[s]["n"], c.archive_download(s).tobytes()) for s in range(n)]
    sizes = c.local_map_build(list(range(n)), [scan] * n)
    rings = [(tuple(sizes[s]["n"]), [c.local_map_download(s, w).tobytes() for w in (0, 1)]) for s in range(n)]
    return recs, archive, rings


@pytest.fixture(scope="module")
def pair(pkg, ieskf):
    a = ieskf.IeskfContext(pkg.default_params(), max_batch=65, max_targets=1024)
    b = ieskf.IeskfContext(pkg.default_params(), max_batch=65, max_targets=1024)
    yield a, b
    a.close()
    b.close()


@pytest.mark.parametrize("n", [1, 3, 65])
def test_batch_equals_single_applies(pair, n):
    a, b = pair
    slots = list(range(n))[::-1] if n == 3 else list(range(n))  # (any order)
    streams = [stream_of(s, n) for s in slots]
    assert len({t for t in streams if t >= 0}) == sum(t >= 0 for t in streams)  # a stream at most once
    fill(a, n)
    fill(b, n)
    before = snapshot(a, n)
    a.pose_graph_apply_batch(slots, streams)
    for s, t in zip(slots, streams):
        b.pose_graph_apply(s, t)
    got, want = snapshot(a, n), snapshot(b, n)
    assert got == want
    frames = tiny_frames(3)
    for s, t in zip(slots, streams):
        newest = six_of_key(a.pose_graph_poses(s)[2]).tobytes()
        assert np.abs(a.pose_graph_poses(s)[2] - frames[2][3]).max() > 0.01  # the solve moved the newest frame
        assert got[1][s] != before[1][s] and got[2][s] != before[2][s]  # ... and archive and ring moved with it
        if t >= 0:  # aft = last = tobe = the newest pose; bef, prev, n_frames (and the host's last_time) untouched
            assert got[0][t][1] == got[0][t][2] == got[0][t][3] == newest
            assert (got[0][t][0],) + got[0][t][4:] == (before[0][t][0],) + before[0][t][4:]
    written = {t for t in streams if t >= 0}
    for t in range(n):
        if t not in written:  # the stream of the slot given with -1: its record is untouched
            assert got[0][t] == before[0][t]
    assert n < 3 or len(written) == n - 1


def test_a_refused_batch_changes_nothing(pair, ieskf):
    a, _ = pair
    fill(a, 3, ring_short=2)  # the ring of slot 2 holds one frame: behind its graph of three
    before = snapshot(a, 3)
    with pytest.raises(ieskf.LinsError, match="error -1"):
        a.pose_graph_apply_batch([0, 1, 2], [0, 1, 2])
    for slots, streams in (([0, 0], [0, 1]), ([0, 1], [1, 1]), ([0, 3], [0, 1]), ([0, 1], [0, 3]), ([0, 1], [0, -2])):
        with pytest.raises(ieskf.LinsError, match="error -1"):  # a slot or a stream twice, out of range
            a.pose_graph_apply_batch(slots, streams)
    assert snapshot(a, 3) == before
    a.pose_graph_apply_batch([1, 0], [-1, 2])  # the slots whose rings are in step go through
    after = snapshot(a, 3)
    assert after[1][2] == before[1][2] and after[1][0] != before[1][0] and after[0][2] != before[0][2] and after[0][:2] == before[0][:2]
    a.pose_graph_apply_batch([], [])
