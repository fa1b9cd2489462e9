"""The team map's CPU restatement (include/lins_host.h lins_host_team_map): a composition of the existing restatements
over a frame list gathered from several slots, so it is held against lins_host_surround_map — pairs all from one slot
against the surround map of their ids, pairs from two slots against the surround map over one frame array that holds the
same frames in list order.  Clouds, sizes, boxes and status bit for bit."""
import importlib

import numpy as np

from local_map_synth import room_scan, trajectory

PKG = "lins---lidar-inertial-slam_amd"
team = importlib.import_module(PKG + ".team")
SMALL = dict(n_corner=60, n_surf=500, n_outlier=30)
E_ARG = -1


def make_frames(n, seed):
    poses = trajectory(n, seed=seed)
    return [room_scan(100 * seed + i, poses[i], **SMALL) + (poses[i],) for i in range(n)], poses


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_pairs_of_one_slot_are_the_surround_map_of_their_ids(host):
    fr, poses = make_frames(6, 1)
    other, _ = make_frames(3, 2)
    fr[2] = (fr[2][0], fr[2][1], fr[2][2][:0], fr[2][3])  # a frame without outliers
    fr[4] = (fr[4][0][:1], fr[4][1][:0], fr[4][2][:0], fr[4][3])  # a one-point frame
    scan = room_scan(900, poses[3], **SMALL)
    for ids in ([], [3], [5, 0, 3, 2], [4], [4, 2, 4]):
        want, ws = host.surround_map(fr, ids, scan)
        got, gs = team.host_map([other, fr], [(1, i) for i in ids], scan)
        assert gs == ws and same(got, want), ids
        assert gs["frames"] == len(ids) and gs["status"] == 0


def test_pairs_of_two_slots_are_the_surround_map_of_the_frames_in_list_order(host):
    a, poses = make_frames(6, 3)
    b, _ = make_frames(4, 4)
    scan = room_scan(901, poses[2], **SMALL)
    for pairs in ([(0, 5), (1, 2), (0, 0), (1, 3)], [(1, 0)], [(1, 1), (0, 1), (1, 1)], [(0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (0, 4)]):
        listed = [(a, b)[s][i] for s, i in pairs]
        want, ws = host.surround_map(listed, list(range(len(pairs))), scan)
        got, gs = team.host_map([a, b], pairs, scan)
        assert gs == ws and same(got, want), pairs
        assert gs["n"][0] > 0 and gs["n"][1] > 0
    # the order of the list shows in the bits (sequential f32 sums), so "in list order" is a claim
    one, _ = team.host_map([a, b], [(0, 5), (1, 2), (0, 0)], scan)
    two, _ = team.host_map([a, b], [(1, 2), (0, 0), (0, 5)], scan)
    assert one[1].shape == two[1].shape and not same(one[:2], two[:2])


def test_a_pair_that_names_nothing_is_refused(host):
    a, poses = make_frames(2, 5)
    scan = room_scan(902, poses[0], **SMALL)
    for bad in ([(0, 2)], [(0, 0), (1, 0)], [(-1, 0)], [(0, -1)], [(2, 0)]):
        assert team.host_map([a, []], bad, scan) == E_ARG
