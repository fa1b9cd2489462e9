"""The team map on the device (include/lins_map.h lins_local_map_build_team): the local map built from a list of
(slot, id) pairs of the key-frame archive.  All six clouds, sizes, boxes and status bit for bit against
lins_local_map_build_surround for pairs of one slot, against a second context whose single slot was pushed the frames of
both slots in list order with their poses for pairs across two slots, and against the CPU restatement
(lins_host_team_map); the scans of large map jobs split at every chunk size; batch positions; and the calls that share
the build (lins_local_map_build, lins_archive_assemble) before and after a team build.  Ring window 3, frames of 300 to
1 500 points."""
import importlib

import numpy as np
import pytest

import map_step_chain as ch
from local_map_synth import room_scan, trajectory
from map_step_chain import defs, host

pytestmark = pytest.mark.gpu
PKG = "lins---lidar-inertial-slam_amd"
team = importlib.import_module(PKG + ".team")

F = np.float32
WINDOW = 3
SMALL = dict(n_corner=60, n_surf=500, n_outlier=30)
CORNER, SURF_OUTLIER = defs.SUBMAP_CORNER, defs.SUBMAP_SURF | defs.SUBMAP_OUTLIER
INT_MAX = 2 ** 31 - 1
bits = ch.bits


def make_frames(n, seed, **kw):
    poses = trajectory(n, seed=seed)
    return [room_scan(100 * seed + i, poses[i], **kw) + (poses[i],) for i in range(n)], poses


def fill(c, slot, frames):
    for i, (co, su, ou, p) in enumerate(frames):
        assert c.archive_push(slot, co, su, ou, p, time=float(i)) == i


def clouds_of(c, k):
    return [c.local_map_download(k, w) for w in range(6)]


def same_clouds(a, b):
    return all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def frames():
    a, poses = make_frames(8, 1, **SMALL)
    a[2] = (a[2][0], a[2][1], a[2][2][:0], a[2][3])  # a frame without outliers
    a[4] = (a[4][0][:1], a[4][1][:0], a[4][2][:0], a[4][3])  # a one-point frame
    b, _ = make_frames(5, 3, **SMALL)
    return a, b, poses


@pytest.fixture
def ctx(pkg, ieskf):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    yield c
    c.close()


@pytest.fixture
def two(ctx, frames):
    """slot 0: a, slot 1: b, a ring of two frames of its own in slot 0"""
    a, b, _ = frames
    ctx.local_map_init(2, WINDOW, 4096)
    ctx.archive_init(2, 16, 1 << 16)
    fill(ctx, 0, a)
    fill(ctx, 1, b)
    for i in range(2):
        ctx.local_map_push(0, *a[i])
    return ctx


LISTS = [[], [3], [0, 1, 2, 3, 4, 5, 6], [5, 0, 3], [2], [4], [4, 2]]
ACROSS = [[(0, 5), (1, 2), (0, 0), (1, 4)], [(1, 0)], [(1, 1), (0, 4), (1, 1)], [(0, 2), (1, 3), (0, 4), (0, 7), (1, 0), (0, 1), (1, 2)], []]


def test_pairs_of_one_slot_are_the_surround_build(two, frames):
    a, b, poses = frames
    scans = [room_scan(900 + k, poses[k % 8], **SMALL) for k in range(len(LISTS))]
    scans[1] = (scans[1][0][:0], scans[1][1], scans[1][2][:0])
    slots = [0] * len(LISTS)
    want_sizes = two.local_map_build_surround(slots, LISTS, scans)
    want = [clouds_of(two, k) for k in range(len(LISTS))]
    sizes = two.local_map_build_team(slots, [[(0, i) for i in lst] for lst in LISTS], scans)
    for k, lst in enumerate(LISTS):
        got = clouds_of(two, k)
        assert sizes[k] == want_sizes[k] and same_clouds(got, want[k]), k
        hw, hs = team.host_map([a, b], [(0, i) for i in lst], scans[k])
        assert sizes[k] == hs and same_clouds(got, hw), k
        assert sizes[k]["frames"] == len(lst) and sizes[k]["status"] == 0
    assert sizes[0]["n"][:2] == [0, 0] and sizes[5]["n"][:2] == [1, 0]
    # the entry's own slot decides nothing about the map side: slot 1 lists frames of slot 0 alone
    other = two.local_map_build_team([1] * len(LISTS), [[(0, i) for i in lst] for lst in LISTS], scans)
    assert other == want_sizes and all(same_clouds(clouds_of(two, k), want[k]) for k in range(len(LISTS)))


def test_pairs_across_two_slots_are_one_slot_holding_the_frames_in_list_order(two, frames, pkg, ieskf):
    a, b, poses = frames
    scans = [room_scan(920 + k, poses[k], **SMALL) for k in range(len(ACROSS))]
    sizes = two.local_map_build_team([k % 2 for k in range(len(ACROSS))], ACROSS, scans)
    got = [clouds_of(two, k) for k in range(len(ACROSS))]
    single = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    single.local_map_init(1, WINDOW, 4096)
    for k, pairs in enumerate(ACROSS):
        listed = [(a, b)[s][i] for s, i in pairs]
        single.archive_init(1, 16, 1 << 16)  # (a second call drops every frame)
        fill(single, 0, listed)
        ws = single.local_map_build_surround([0], [list(range(len(pairs)))], [scans[k]])
        assert sizes[k] == ws[0] and same_clouds(got[k], clouds_of(single, 0)), k
        hw, hs = team.host_map([a, b], pairs, scans[k])
        assert sizes[k] == hs and same_clouds(got[k], hw), k
        assert sizes[k]["frames"] == len(pairs) and sizes[k]["status"] == 0
    single.close()
    assert sizes[0]["n"][0] > 0 and sizes[0]["n"][1] > 0 and sizes[4]["n"][:2] == [0, 0] and sizes[4]["n"][2] > 0


def test_split_scans_give_the_same_bits_at_every_chunk(ctx):
    a, poses = make_frames(7, 2, n_corner=200, n_surf=1200, n_outlier=100)
    b, _ = make_frames(3, 5, n_corner=200, n_surf=1200, n_outlier=100)
    ctx.local_map_init(2, WINDOW, 4096)
    ctx.archive_init(2, 8, 1 << 16)
    fill(ctx, 0, a)
    fill(ctx, 1, b)
    lists = [[(0, 0), (1, 0), (0, 1), (0, 2), (1, 2), (0, 3), (0, 4), (0, 5), (0, 6), (1, 1)], [(1, 1), (0, 0)]]
    scans = [room_scan(960 + k, poses[k], **SMALL) for k in range(2)]
    want = [team.host_map([a, b], lists[k], scans[k]) for k in range(2)]
    assert sum(len((a, b)[s][i][1]) + len((a, b)[s][i][2]) for s, i in lists[0]) > 16 * 512  # (more tiles than the default chunk)
    for chunk in (1, 2, 0, INT_MAX):  # every map job split; the large ones; the default; none
        ctx.archive_set_scan_chunk(chunk)
        sizes = ctx.local_map_build_team([0, 1], lists, scans)
        for k in range(2):
            assert sizes[k] == want[k][1], (chunk, k, sizes[k], want[k][1])
            assert same_clouds(clouds_of(ctx, k), want[k][0]), (chunk, k)
    assert want[0][1]["n"][1] > 1024


def test_batch_positions(two, frames):
    a, b, poses = frames
    x = (0, ACROSS[0], room_scan(970, poses[2], **SMALL))
    y = (1, ACROSS[3], room_scan(971, poses[5], **SMALL))
    e = (1, [], room_scan(972, poses[0], **SMALL))

    def build(entries):
        sizes = two.local_map_build_team([t[0] for t in entries], [t[1] for t in entries], [t[2] for t in entries])
        return [(sizes[k], clouds_of(two, k)) for k in range(len(entries))]

    alone = build([x])[0]
    first, last = build([x, e, y]), build([y, e, x])
    for got in (first[0], last[2]):
        assert got[0] == alone[0] and same_clouds(got[1], alone[1])
    assert first[2][0] == last[0][0] and same_clouds(first[2][1], last[0][1])
    assert first[1][0]["n"][:2] == [0, 0] and first[1][0]["frames"] == 0


def test_the_calls_that_share_the_build_keep_their_bits(two, frames):
    a, b, poses = frames
    scan = room_scan(980, poses[3], **SMALL)
    specs = [(0, [5, 0, 3], CORNER, 0.2, 0), (1, [4, 1], SURF_OUTLIER, 0.4, 0), (1, [2], CORNER | SURF_OUTLIER, 0.0, 0)]

    def others():
        ring = two.local_map_build([0, 1], [scan, scan])
        rc = [clouds_of(two, k) for k in range(2)]
        sur = two.local_map_build_surround([0, 1], [[5, 0, 3], [4, 1]], [scan, scan])
        sc = [clouds_of(two, k) for k in range(2)]
        info = two.archive_assemble(specs)
        return ring, rc, sur, sc, info, [two.archive_download(k) for k in range(len(specs))]

    before = others()
    sizes = two.local_map_build_team([1, 0], [ACROSS[3], ACROSS[0]], [scan, scan])
    assert all(z["status"] == 0 and z["n"][0] > 0 for z in sizes)
    after = others()
    assert before[0] == after[0] and before[2] == after[2] and before[4] == after[4]
    for k in range(2):
        assert same_clouds(before[1][k], after[1][k]) and same_clouds(before[3][k], after[3][k])
    assert same_clouds(before[5], after[5])
    assert before[0][0]["frames"] == 2 and before[0][1]["frames"] == 0  # (the rings: slot 0 holds two frames, slot 1 none)


def test_refusals_change_nothing(two, frames, pkg, ieskf):
    a, b, poses = frames
    scan = room_scan(990, poses[1], **SMALL)
    sizes = two.local_map_build_team([0], [ACROSS[0]], [scan])
    kept = clouds_of(two, 0)
    for slots, lists in (([0], [[(0, 8)]]), ([0], [[(1, 5)]]), ([0], [[(2, 0)]]), ([0], [[(-1, 0)]]), ([0], [[(0, -1)]]), ([2], [[(0, 0)]]),
                         ([0, 0], [ACROSS[0], [(0, 0), (1, 9)]])):
        with pytest.raises(ieskf.LinsError, match="error -1"):
            two.local_map_build_team(slots, lists, [scan] * len(slots))
        two._local_sizes = sizes  # (the wrapper forgets them when a call fails; the context does not)
        assert same_clouds(clouds_of(two, 0), kept)
    bare = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    with pytest.raises(ieskf.LinsError, match="error -6"):
        bare.local_map_build_team([0], [[]], [scan])
    bare.local_map_init(1, WINDOW, 4096)
    with pytest.raises(ieskf.LinsError, match="error -6"):  # (no archive)
        bare.local_map_build_team([0], [[]], [scan])
    bare.close()
