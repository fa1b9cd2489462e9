"""The key-frame archive's CPU restatement (host/keyframe_archive.cpp, host/keyframe_select.h: lins_host_select_radius /
_find_loop / _submap) against the independent numpy statement tests/archive_np.py, bit for bit."""
import numpy as np
import pytest

import archive_np as anp
from local_map_synth import room_scan, trajectory

SMALL = dict(n_corner=60, n_surf=500, n_outlier=40)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def pose(x, y, z):
    return (x, y, z, 0.0, 0.0, 0.0)


def assert_same_submap(host, frames, spec):
    want, wi = anp.submap(frames, spec["ids"], spec["clouds"], spec["leaf"], spec["flags"])
    got, gi = host.submap(frames, spec["ids"], spec["clouds"], spec["leaf"], spec["flags"])
    assert gi == wi, (gi, wi)
    assert np.array_equal(bits(got), bits(want))
    return got, gi


@pytest.fixture(scope="module")
def frames60():
    poses = trajectory(60, seed=3)
    fr = [room_scan(100 + i, poses[i], **SMALL) + (poses[i],) for i in range(60)]
    e = np.zeros((0, 4), np.float32)
    fr[5] = (e, fr[5][1], fr[5][2], poses[5])  # empty clouds inside frames
    fr[6] = (fr[6][0], e, e, poses[6])
    fr[58] = (e, e, fr[58][2], poses[58])
    fr[59][1][:5, 3] = [-1.5, -1.0, -0.5, 0.0, 7.25]
    return fr, poses


def test_radius_selection_on_a_looping_trajectory(host):
    poses = np.concatenate([trajectory(150, seed=1), trajectory(150, seed=2)])  # two laps: every place is visited twice
    for centre, radius, leaf in ((poses[10, :3], 6.0, 1.0), (poses[200, :3], 500.0, 1.0), ((0.0, 0.0, 0.0), 7.5, 0.05), ((50.0, 0, 0), 3.0, 1.0)):
        want = anp.select_radius(poses, centre, radius, leaf)
        got = host.select_radius(poses, centre, radius, leaf)
        assert np.array_equal(got, want), (centre, radius, leaf)
    assert len(anp.select_radius(poses, poses[200, :3], 500.0, 1.0)) > 30 and len(anp.select_radius(poses, (50.0, 0, 0), 3.0, 1.0)) == 0


def test_selection_names_the_truncated_mean_id_even_when_that_frame_is_elsewhere(host):
    poses = [pose(0.2, 0.2, 0.2), pose(5.5, 5.5, 0.5), pose(0.6, 0.6, 0.2), pose(0.7, 0.1, 0.3)]
    got = host.select_radius(poses, (0, 0, 0), 100.0, 1.0)
    assert np.array_equal(got, anp.select_radius(poses, (0, 0, 0), 100.0, 1.0))
    # voxel (0, 0, 0) holds frames 0, 2, 3: mean 5 / 3 -> 1, a frame that lies in another voxel (LM:1007)
    assert got.tolist() == [1, 1]


def test_distance_ties_are_broken_by_id_and_a_pose_at_the_radius_is_a_hit(host):
    poses = [pose(0, 1, 0), pose(-1, 0, 0), pose(1, 0, 0), pose(3, 4, 0), pose(3, 4, 0.01)]
    times = [0.0, 0.0, 0.0, 0.0, 0.0]
    for recent, want in (([], 0), ([0], 1), ([0, 1], 2), ([0, 1, 2], 3)):
        t = list(times)
        for r in recent:
            t[r] = 100.0
        assert host.find_loop(poses, t, (0, 0, 0), 5.0, 100.0, 30.0) == want == anp.find_loop(poses, t, (0, 0, 0), 5.0, 100.0, 30.0)
    # 3*3 + 4*4 = 25 <= 5*5 exactly in f32: frame 3 is in, frame 4 (a centimetre further) is out
    t = [100.0, 100.0, 100.0, 100.0, 0.0]
    assert host.find_loop(poses, t, (0, 0, 0), 5.0, 100.0, 30.0) == -1
    assert sorted(host.select_radius(poses, (0, 0, 0), 5.0, 0.5).tolist()) == sorted(anp.select_radius(poses, (0, 0, 0), 5.0, 0.5).tolist())
    assert 3 in host.select_radius(poses, (0, 0, 0), 5.0, 0.5) and 4 not in host.select_radius(poses, (0, 0, 0), 5.0, 0.5)


def test_find_loop_none_skipped_and_first_of_several(host):
    poses = np.concatenate([trajectory(150, seed=1), trajectory(150, seed=2)])
    poses[150:, :2] += np.float32(0.25)  # lap two runs beside lap one: the nearest poses are the recent ones
    times = np.arange(300) * 0.5  # lap two starts at 75 s
    c, now = poses[299, :3], 149.5
    cases = [(5.0, 30.0), (5.0, 1e9), (0.05, 30.0), (2.0, 0.0), (5.0, 70.0)]
    got = [host.find_loop(poses, times, c, r, now, gap) for r, gap in cases]
    assert got == [anp.find_loop(poses, times, c, r, now, gap) for r, gap in cases]
    assert got[1] == -1  # nothing is old enough
    assert got[0] >= 0 and abs(times[got[0]] - now) > 30.0  # the recent neighbours of lap two were skipped
    hits = anp.radius_search(poses, c, 5.0)
    assert hits[0] == 299 and got[0] != hits[0] and sum(abs(times[i] - now) > 30.0 for i in hits) > 1  # the first of several
    assert host.find_loop(poses[:0], times[:0], c, 5.0, now, 30.0) == -1


def test_the_three_compositions(host, frames60):
    fr, poses = frames60
    g = anp.global_map_spec(poses, poses[59, :3])
    assert np.array_equal(host.select_radius(poses, poses[59, :3], 500.0, 1.0), g["ids"]) and len(g["ids"]) > 10
    cloud, info = assert_same_submap(host, fr, g)
    assert info["n"] > 1000 and info["box_dim"][0] > 20
    for closest in (3, 57, 30):  # windows clipped at the start, at the end, and whole
        h = anp.history_spec(60, closest)
        assert (h["ids"][0], h["ids"][-1]) == (max(0, closest - 25), min(59, closest + 25))
        assert_same_submap(host, fr, h)
    cloud, info = assert_same_submap(host, fr, anp.latest_spec(60))
    n_in = len(fr[59][0]) + len(fr[59][1])
    assert info["points_in"] == n_in and info["n"] == n_in - 2  # -1.5 and -1.0 are dropped, -0.5 is kept
    assert np.array_equal(bits(cloud[len(fr[59][0]):len(fr[59][0]) + 3, 3]), bits([-0.5, 0.0, 7.25]))


def test_submap_edge_cases(host, frames60):
    fr, _ = frames60
    cloud, info = assert_same_submap(host, fr, dict(ids=[], clouds=anp.ALL, leaf=0.4, flags=0))
    assert info["n"] == 0 and info["status"] == 0 and info["box_dim"] == [1, 1, 1]
    assert_same_submap(host, fr, dict(ids=[], clouds=anp.SURF, leaf=0.0, flags=anp.DROP_NEGATIVE))
    cloud, info = assert_same_submap(host, fr, dict(ids=[7, 7, 8, 7], clouds=anp.ALL, leaf=0.0, flags=0))  # a repeated id
    n7 = sum(len(c) for c in fr[7][:3])
    assert np.array_equal(bits(cloud[:n7]), bits(cloud[n7:2 * n7])) and info["n"] == 3 * n7 + sum(len(c) for c in fr[8][:3])
    assert_same_submap(host, fr, dict(ids=[7, 7, 8, 7], clouds=anp.ALL, leaf=0.4, flags=0))
    for clouds in (anp.CORNER, anp.SURF, anp.OUTLIER, anp.CORNER | anp.OUTLIER, anp.SURF | anp.OUTLIER):
        assert_same_submap(host, fr, dict(ids=[4, 5, 6, 58], clouds=clouds, leaf=0.2, flags=0))
        assert_same_submap(host, fr, dict(ids=[4, 5, 6, 58], clouds=clouds, leaf=0.0, flags=anp.DROP_NEGATIVE))
    assert_same_submap(host, fr, dict(ids=[5], clouds=anp.CORNER, leaf=0.4, flags=0))  # only an empty cloud


def test_submap_statuses_and_refused_arguments(host, frames60):
    fr, _ = frames60
    far = list(fr[:3])
    far[1] = fr[1][:3] + ((999990.0, 0.0, 0.0, 0.0, 0.0, 0.0),)  # the pose throws its points beyond 1e6
    for leaf, flags in ((0.4, 0), (0.0, 0), (0.0, anp.DROP_NEGATIVE)):
        _, info = assert_same_submap(host, far, dict(ids=[0, 1], clouds=anp.ALL, leaf=leaf, flags=flags))
        assert info["status"] == -4 and info["n"] == 0
    wide = list(fr[:3])
    wide[2] = fr[2][:3] + ((9.0e5, 9.0e5, 0.0, 0.0, 0.0, 0.0),)  # a 0.4 m box of far more than 2^31 cells
    _, info = assert_same_submap(host, wide, dict(ids=[0, 2], clouds=anp.SURF, leaf=0.4, flags=0))
    assert info["status"] == -3 and info["n"] == 0
    for bad in (dict(ids=[60], clouds=anp.ALL, leaf=0.4, flags=0), dict(ids=[-1], clouds=anp.ALL, leaf=0.4, flags=0),
                dict(ids=[1], clouds=0, leaf=0.4, flags=0), dict(ids=[1], clouds=8, leaf=0.4, flags=0),
                dict(ids=[1], clouds=anp.ALL, leaf=0.4, flags=anp.DROP_NEGATIVE), dict(ids=[1], clouds=anp.ALL, leaf=-1.0, flags=0)):
        with pytest.raises(RuntimeError, match="-1"):
            host.submap(fr, bad["ids"], bad["clouds"], bad["leaf"], bad["flags"])
