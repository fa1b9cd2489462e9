"""Key-pose selection on the device (include/lins_map.h lins_keyposes_*): the batched radius search, pose grid, loop
candidate and surround list rule against the host text — lins_host_select_radius / _find_loop / _surround_update on the
same poses, and lins_archive_select_radius / _find_loop on a second context — id for id (every output is an integer: exact
equality throughout); the archive's pose mirror behind every call that writes poses; and the two callers, the surround
step and the loop step, in LINS_KEYPOSES_DEVICE against LINS_KEYPOSES_HOST on a second context.  Frames of one point."""
import numpy as np
import pytest

import loop_step_cases as lsc
import map_step_chain as ch
from map_step_chain import defs, host, sm

pytestmark = pytest.mark.gpu

F = np.float32
PT = np.array([[0.1, 0.2, 0.3, 0.0]], F)
NONE = np.zeros((0, 4), F)
E_ARG, E_CAPACITY, E_INPUT, E_STATE = -1, -3, -4, -6
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025]
HOST, DEVICE = defs.KEYPOSES_HOST, defs.KEYPOSES_DEVICE


def make(pkg, ieskf):
    return ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)


def poses6(xyz):
    p = np.zeros((len(xyz), 6), F)
    p[:, :3] = np.asarray(xyz, F).reshape(-1, 3)
    return p


def fill(c, slot, poses, times=None):
    for i, p in enumerate(poses):
        assert c.archive_push(slot, PT, NONE, NONE, p, time=float(i) if times is None else float(times[i])) == i


def host_select(poses, centre, radius, leaf):
    """the ids, or None where the host refuses the box"""
    try:
        return host.select_radius(poses, centre, radius, leaf).tolist()
    except RuntimeError as e:
        assert "-3" in str(e)
        return None


def ids_of(got):
    return [None if g is None else g.tolist() for g in got]


def lattice(n, seed):
    """n poses on a 0.5 m lattice in [-8, 8]^2 x [-1, 1]: equal distances, coincident poses, negative coordinates"""
    rng = np.random.default_rng(seed)
    return poses6(np.stack([0.5 * rng.integers(-16, 17, n), 0.5 * rng.integers(-16, 17, n), 0.5 * rng.integers(-2, 3, n)], 1))


# ---- 1. sizes: one slot per size, one batch over all of them ----------------------------------------------------------
@pytest.fixture(scope="module")
def sized(pkg, ieskf):
    a, b = make(pkg, ieskf), make(pkg, ieskf)
    all_poses = [lattice(n, 40 + k) for k, n in enumerate(SIZES)]
    for c in (a, b):
        c.archive_init(len(SIZES), max(SIZES), 2 * sum(SIZES) + 1)
        for s, p in enumerate(all_poses):
            fill(c, s, p)
    yield a, b, all_poses
    a.close()
    b.close()


@pytest.mark.parametrize("centre,radius,leaf", [((0.0, 0.0, 0.0), 6.0, 1.0), ((0.25, -0.25, 0.0), 3.0, 0.4), ((-3.0, 2.0, 0.5), 100.0, 2.5),
                                                ((0.5, 0.5, 0.0), 0.75, 1.0), ((0.0, 0.0, 0.0), 2.5, 0.02)])
def test_select_at_every_size(sized, centre, radius, leaf):
    a, b, all_poses = sized
    got, res = a.keyposes_select_batch([(s, centre, radius, leaf) for s in range(len(SIZES))])
    hits = 0
    for s, p in enumerate(all_poses):
        want = host_select(p, centre, radius, leaf)
        assert want is not None and ids_of(got)[s] == want, (SIZES[s], got[s], want)
        assert want == b.archive_select_radius(s, centre, radius, leaf).tolist()
        d = ((p[:, 0] - F(centre[0])) ** 2 + (p[:, 1] - F(centre[1])) ** 2) + (p[:, 2] - F(centre[2])) ** 2
        assert res[s] == dict(n=len(want), hits=int((d <= F(radius) * F(radius)).sum()), status=0, host=0)
        hits += res[s]["hits"]
    st = a.keyposes_stats()
    assert st["hits"] == hits and st["host_entries"] == 0 and st["device_ms"] > 0


def test_find_loop_at_every_size(sized):
    a, b, all_poses = sized
    for centre, radius, now, gap in (((0.0, 0.0, 0.0), 6.0, 100.0, 30.0), ((0.5, 0.5, 0.0), 2.0, 40.0, 10.0), ((0.0, 0.0, 0.0), 1.0, 2000.0, 1.0)):
        got = a.keyposes_find_loop_batch([(s, centre, radius, now, gap) for s in range(len(SIZES))])
        want = [host.find_loop(p, np.arange(len(p), dtype=np.float64), centre, radius, now, gap) for p in all_poses]
        assert got == want == [b.archive_find_loop(s, centre, radius, now, gap) for s in range(len(SIZES))]
        assert got[0] == -1 and any(g >= 0 for g in got)


def test_surround_at_every_size(sized):
    a, _, all_poses = sized
    rng = np.random.default_rng(3)
    lists = [rng.permutation(n)[: n // 2].tolist() + ([0, 0] if n else []) for n in SIZES]  # (the tail: an id held twice)
    for centre, radius, leaf in (((0.0, 0.0, 0.0), 4.0, 1.0), ((2.0, -1.0, 0.0), 7.0, 0.02)):
        got, res = a.keyposes_surround_batch([(s, centre, radius, leaf) for s in range(len(SIZES))], lists)
        for s, p in enumerate(all_poses):
            ds = host_select(p, centre, radius, leaf)
            assert got[s] == host.surround_update(lists[s], ds), SIZES[s]
            assert res[s] == dict(n=len(ds), hits=res[s]["hits"], status=0, host=0)
        lists = got  # the second query erases and appends on what the first left


# ---- 2. geometry ------------------------------------------------------------------------------------------------------
GEOMETRY = {
    # name: (poses, centre, radius, leaf, the ids by hand)
    "radius 0 with a pose on the centre": ([(1, 2, 3), (1, 2, 3.5), (1, 2, 3)], (1, 2, 3), 0.0, 0.1, [1]),  # ids 0 and 2 in one cell: (0 + 2) / 2
    "a hit exactly on the boundary": ([(3, 4, 0), (3, 4, 0.01), (0, 0, 9)], (0, 0, 0), 5.0, 0.001, [0]),
    "coincident poses": ([(0.5, 0.5, 0.5)] * 5 + [(7, 7, 7)], (0, 0, 0), 2.0, 1.0, [2]),
    # the floor: x = -0.5, -1.0, -0.25 -> cell -1 (ids 4, 0, 1 in hit order: 5 / 3 -> 1), -1.5 -> cell -2, 0.5 -> cell 0
    "negative coordinates": ([(-0.5, 0, 0), (-1.0, 0, 0), (-1.5, 0, 0), (0.5, 0, 0), (-0.25, 0, 0)], (0, 0, 0), 3.0, 1.0, [2, 1, 3]),
    # ids 0, 3, 4 share a cell: 7 / 3 -> 2, and frame 2 lies 127 m away
    "a truncated mean that names a frame outside the radius": ([(0.2, 0.2, 0), (50, 50, 0), (90, 90, 0), (0.4, 0.4, 0), (0.6, 0.6, 0)], (0, 0, 0), 2.0, 1.0, [2]),
    # cell 0 holds ids 0, 1, 3: 4 / 3 -> 1; cell 5 holds ids 2, 4: 3
    "the means of two cells": ([(0.5, 0.5, 0), (0.5, 0.5, 0), (5.5, 0.5, 0), (0.5, 0.5, 0), (5.5, 0.5, 0)], (3, 0, 0), 4.0, 1.0, [1, 3]),
}
# two cells with the same truncated mean: ids 0 and 4 in one, id 2 in the other — the selection names frame 2 twice
TWICE = ([(0.5, 0.5, 0), (9, 9, 9), (5.5, 0.5, 0), (9, 9, 9), (0.5, 0.5, 0)], (3, 0, 0), 4.0, 1.0, [2, 2])


@pytest.fixture(scope="module")
def shaped(pkg, ieskf):
    c = make(pkg, ieskf)
    cases = list(GEOMETRY.values()) + [TWICE]
    c.archive_init(len(cases), 8, 64)
    for s, case in enumerate(cases):
        fill(c, s, poses6(case[0]))
    yield c, cases
    c.close()


def test_geometry_cases(shaped):
    c, cases = shaped
    got, res = c.keyposes_select_batch([(s, centre, radius, leaf) for s, (_, centre, radius, leaf, _) in enumerate(cases)])
    for s, (xyz, centre, radius, leaf, by_hand) in enumerate(cases):
        assert ids_of(got)[s] == by_hand == host_select(poses6(xyz), centre, radius, leaf), s
        assert by_hand == c.archive_select_radius(s, centre, radius, leaf).tolist()
        assert res[s]["status"] == 0 and res[s]["host"] == 0
    assert res[1]["hits"] == 1  # the boundary: (3, 4, 0) alone, at d == r2
    outside = cases[4]
    assert np.linalg.norm(np.asarray(outside[0][2]) - np.asarray(outside[1])) > outside[2]  # frame 2 is no hit
    # an id named twice enters the list once, behind the survivors
    s = len(cases) - 1
    lists, _ = c.keyposes_surround_batch([(s, *TWICE[1:4])] * 2, [[], [4, 2, 0]])
    assert lists == [[2], [2]] == [host.surround_update([], [2, 2]), host.surround_update([4, 2, 0], [2, 2])]


def test_equal_distances_are_ordered_by_id(pkg, ieskf):
    """poses mirrored about the centre: the loop candidate is the smaller id of the nearest pair that the gap lets through"""
    xyz = [(2, 0, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (-2, 0, 0)]
    times = [0.0, 50.0, 0.0, 0.0, 0.0, 0.0]  # id 1 lies inside the gap
    with make(pkg, ieskf) as c:
        c.archive_init(1, 8, 64)
        fill(c, 0, poses6(xyz), times)
        got = c.keyposes_find_loop_batch([(0, (0, 0, 0), 5.0, 50.0, 30.0), (0, (0, 0, 0), 1.0, 50.0, 60.0), (0, (0, 0, 0), 5.0, 50.0, 50.0)])
        want = [host.find_loop(poses6(xyz), times, (0, 0, 0), r, 50.0, gap) for r, gap in ((5.0, 30.0), (1.0, 60.0), (5.0, 50.0))]
        # the nearest (id 1) is refused by the gap and the next of the four at d = 1 is taken: the smallest id; every hit
        # within the gap: none; fabs(time - now) == min_gap_s exactly (ids 0, 2 .. 5 at 50 s): not taken
        assert got == want == [2, -1, -1]


def test_sequential_sum_of_a_long_run(big):
    """ids 2000 .. 8000 on one point: the f32 sum taken one id after the other gives a mean of 4999, a pairwise sum 5000"""
    ids = np.arange(2000, 8001).astype(F)
    seq = F(0)
    for v in ids:
        seq = F(seq + v)
    assert int(seq / F(len(ids))) == 4999 and int(np.sum(ids, dtype=F) / F(len(ids))) == 5000  # (numpy sums pairwise)
    c, poses = big
    got, res = c.keyposes_select_batch([(0, (0, 0, 0), 1.0, 1.0)])
    assert ids_of(got) == [[4999]] == [host_select(poses[0], (0, 0, 0), 1.0, 1.0)]
    assert res[0] == dict(n=1, hits=6001, status=0, host=0)


def test_more_hits_than_the_kernel_sorts_are_served_by_the_host(big):
    c, poses = big
    q = [(1, (0, 0, 0), 1.0, 1.0), (0, (0, 0, 0), 1.0, 1.0)]
    got, res = c.keyposes_select_batch(q)
    assert ids_of(got) == [host_select(poses[1], *q[0][1:]), [4999]]
    assert res[0] == dict(n=1, hits=8193, status=0, host=1) and res[1]["host"] == 0
    assert c.keyposes_stats()["host_entries"] == 1 and c.keyposes_stats()["hits"] == 8193 + 6001
    lists, res = c.keyposes_surround_batch(q, [[5, 4096, 7], [4999, 1]])
    assert lists == [host.surround_update([5, 4096, 7], ids_of(got)[0]), [4999]] and [r["host"] for r in res] == [1, 0]


@pytest.fixture(scope="module")
def big(pkg, ieskf):
    c = make(pkg, ieskf)
    far = poses6([(500.0, 500.0, 0.0)] * 2000 + [(0.25, 0.25, 0.25)] * 6001)
    many = poses6([(0.5, 0.5, 0.5)] * 8193)
    c.archive_init(2, 8193, 20000)
    fill(c, 0, far)
    fill(c, 1, many)
    yield c, (far, many)
    c.close()


# ---- 3. capacity, batches, errors --------------------------------------------------------------------------------------
def test_capacity_is_per_entry(pkg, ieskf):
    wide = poses6([(-1000, -1000, 0), (1000, 1000, 0)])
    near = poses6([(0, 0, 0), (1.5, 0, 0), (3.5, 0, 0)])
    with make(pkg, ieskf) as c:
        c.archive_init(2, 4, 16)
        fill(c, 0, near)
        fill(c, 1, wide)
        q = [(0, (0, 0, 0), 10.0, 1.0), (1, (0, 0, 0), 3000.0, 0.01), (0, (1, 0, 0), 10.0, 1.0)]
        assert host_select(wide, (0, 0, 0), 3000.0, 0.01) is None
        got, res = c.keyposes_select_batch(q)
        assert ids_of(got) == [[0, 1, 2], None, [0, 1, 2]] and [r["status"] for r in res] == [0, E_CAPACITY, 0]
        assert res[1]["hits"] == 2 and res[1]["n"] == 0
        lists, res = c.keyposes_surround_batch(q, [[2], [1, 0], []])
        assert lists == [[2, 0, 1], [1, 0], [0, 1, 2]] and [r["status"] for r in res] == [0, E_CAPACITY, 0]
        # a stride too small refuses the entry alone
        got, res = c.keyposes_select_batch([(0, (0, 0, 0), 10.0, 1.0), (0, (0, 0, 0), 1.0, 1.0)], stride=2)
        assert ids_of(got) == [None, [0]] and [r["status"] for r in res] == [E_CAPACITY, 0]
        lists, res = c.keyposes_surround_batch([(0, (0, 0, 0), 10.0, 1.0), (0, (0, 0, 0), 1.0, 1.0)], [[2], [2, 1]], stride=2)
        assert lists == [[2], [0]] and [r["status"] for r in res] == [E_CAPACITY, 0]


def test_an_entrys_bits_do_not_depend_on_its_batch(pkg, ieskf):
    p0, p2 = lattice(300, 7), lattice(90, 8)
    with make(pkg, ieskf) as c:
        c.archive_init(3, 300, 1024)
        fill(c, 0, p0)
        fill(c, 2, p2)  # slot 1 stays empty
        q = (0, (0.5, 0.0, 0.0), 5.0, 0.7)
        alone, ra = c.keyposes_select_batch([q])
        first, r1 = c.keyposes_select_batch([q, (1, (0, 0, 0), 5.0, 1.0), (2, (0, 0, 0), 3.0, 1.0)])
        last, r2 = c.keyposes_select_batch([(2, (0, 0, 0), 3.0, 1.0), (1, (0, 0, 0), 5.0, 1.0), q])
        assert ids_of(alone)[0] == ids_of(first)[0] == ids_of(last)[2] == host_select(p0, *q[1:]) and ra[0] == r1[0] == r2[2]
        assert ids_of(first)[1] == [] and r1[1] == dict(n=0, hits=0, status=0, host=0)
        assert ids_of(first)[2] == ids_of(last)[0] == host_select(p2, (0, 0, 0), 3.0, 1.0)
        # the same slot twice, with different centres
        two, _ = c.keyposes_select_batch([q, (0, (-4.0, 3.0, 0.0), 2.0, 0.7)])
        assert ids_of(two) == [host_select(p0, *q[1:]), host_select(p0, (-4.0, 3.0, 0.0), 2.0, 0.7)] and ids_of(two)[0] != ids_of(two)[1]
        lq = (0, (0.5, 0.0, 0.0), 5.0, 400.0, 200.0)
        assert c.keyposes_find_loop_batch([lq]) == c.keyposes_find_loop_batch([(2, (0, 0, 0), 3.0, 0.0, 1.0), (1, (0, 0, 0), 5.0, 0.0, 1.0), lq])[2:]
        assert c.keyposes_find_loop_batch([lq])[0] == host.find_loop(p0, np.arange(300.0), *lq[1:]) >= 0


def test_errors_and_the_mode(pkg, ieskf):
    with make(pkg, ieskf) as c:
        assert c.keyposes_mode() == HOST
        with pytest.raises(RuntimeError, match=str(E_STATE)):  # before lins_archive_init
            c.keyposes_select_batch([(0, (0, 0, 0), 1.0, 1.0)])
        with pytest.raises(RuntimeError, match=str(E_STATE)):
            c.keyposes_find_loop_batch([])
        c.archive_init(2, 4, 16)
        fill(c, 0, poses6([(0, 0, 0), (1, 0, 0)]))
        assert c.keyposes_select_batch([]) == ([], []) and c.keyposes_find_loop_batch([]) == [] and c.keyposes_surround_batch([], []) == ([], [])
        for bad in ((2, (0, 0, 0), 1.0, 1.0), (-1, (0, 0, 0), 1.0, 1.0), (0, (0, 0, 0), -1.0, 1.0), (0, (0, 0, 0), float("nan"), 1.0),
                    (0, (float("inf"), 0, 0), 1.0, 1.0), (0, (0, 0, 0), 1.0, 0.0), (0, (0, 0, 0), 1.0, float("nan")), (0, (0, 0, 0), 1.0, 1e-45)):
            with pytest.raises(RuntimeError, match=str(E_ARG)):
                c.keyposes_select_batch([(0, (0, 0, 0), 1.0, 1.0), bad])
        for lst in ([2], [-1], [0, 1, 5]):  # a list id that is no frame of the slot
            with pytest.raises(RuntimeError, match=str(E_ARG)):
                c.keyposes_surround_batch([(0, (0, 0, 0), 1.0, 1.0)], [lst])
        with pytest.raises(RuntimeError, match=str(E_ARG)):
            c.keyposes_find_loop_batch([(0, (0, 0, 0), -1.0, 0.0, 1.0)])
        for now, gap in ((float("nan"), 1.0), (float("inf"), 1.0), (0.0, float("nan"))):
            with pytest.raises(RuntimeError, match=str(E_INPUT)):
                c.keyposes_find_loop_batch([(0, (0, 0, 0), 1.0, now, gap)])
        with pytest.raises(RuntimeError, match=str(E_ARG)):
            c.keyposes_set_mode(2)
        # the refusals changed nothing
        assert ids_of(c.keyposes_select_batch([(0, (0, 0, 0), 5.0, 0.1)])[0]) == [[0, 1]]
        c.keyposes_set_mode(DEVICE)
        assert c.keyposes_mode() == DEVICE
        c.keyposes_set_mode(HOST)
        assert c.keyposes_mode() == HOST


# ---- 4. the mirror follows every call that writes poses -----------------------------------------------------------------
def test_mirror_follows_set_poses(pkg, ieskf):
    p = poses6([(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)])
    q = (0, (0, 0, 0), 2.5, 0.1)
    with make(pkg, ieskf) as c:
        c.archive_init(1, 8, 64)
        fill(c, 0, p)
        assert ids_of(c.keyposes_select_batch([q])[0]) == [[0, 1, 2]]
        moved = p.copy()
        moved[1, 0], moved[3, 0] = 40.0, -1.0  # frame 1 leaves the radius, frame 3 enters it on the other side
        c.archive_set_poses(0, 1, moved[1:])
        assert ids_of(c.keyposes_select_batch([q])[0]) == [[3, 0, 2]] == [host_select(moved, *q[1:])] == [c.archive_select_radius(*q).tolist()]
        assert c.keyposes_find_loop_batch([(0, (40, 0, 0), 0.0, 100.0, 1.0)]) == [1]
        assert c.archive_push(0, PT, NONE, NONE, poses6([(0.5, 0, 0)])[0], time=9.0) == 4  # ... and a push behind it
        assert ids_of(c.keyposes_select_batch([q])[0]) == [[3, 0, 4, 2]] == [c.archive_select_radius(*q).tolist()]


def test_mirror_follows_push_scans(pkg, ieskf):
    with ch.context(pkg, ieskf) as c:
        ch.setup(c)
        assert ids_of(c.keyposes_select_batch([(0, (0, 0, 0), 5.0, 0.1), (1, (0, 0, 0), 5.0, 0.1)])[0]) == [[], []]
        for step, x in enumerate((1.0, 3.0)):
            ch.feed(c, step)
            c.local_map_build_streams([0, 1], [0, 1])
            assert c.archive_push_scans([0, 1], poses6([(x, 0, 0), (-x, 0, 0)]), [float(step)] * 2) == [step, step]
            got = ids_of(c.keyposes_select_batch([(0, (0, 0, 0), 2.0, 0.1), (1, (-3, 0, 0), 0.0, 0.1)])[0])
            assert got == [c.archive_select_radius(0, (0, 0, 0), 2.0, 0.1).tolist(), c.archive_select_radius(1, (-3, 0, 0), 0.0, 0.1).tolist()]
            assert got == [[[0], []], [[0], [1]]][step]


def test_mirror_follows_the_pose_graphs_apply(pkg, ieskf):
    with make(pkg, ieskf) as c:
        lsc.init(c, 1)
        lsc.push(c, 0, "loop")
        before = np.array([f[3] for f in lsc.frames()], F)  # the poses the archive was pushed
        at = lambda poses, k: (0, tuple(float(v) for v in poses[k, :3]), 0.0, 1e-3)  # radius 0 on frame k's own position
        assert ids_of(c.keyposes_select_batch([at(before, 9)])[0]) == [[9]]  # (the mirror is current before the step)
        res = c.loop_step([(0, lsc.centre(), lsc.NOW)], lsc.params(ieskf.lib()))
        assert res[0]["outcome"] == defs.LOOP_CLOSED
        after = c.pose_graph_poses(0)
        assert not np.array_equal(before[9, :3], after[9, :3])
        got = ids_of(c.keyposes_select_batch([at(after, 9), at(before, 9)])[0])
        assert got == [c.archive_select_radius(*at(after, 9)).tolist(), c.archive_select_radius(*at(before, 9)).tolist()] and got[0] == [9]


# ---- 5. the callers -------------------------------------------------------------------------------------------------------
STREAMS = [0, 1, 2]
LEAF = 0.02  # (every key pose its own voxel, as tests/test_gpu_surround.py runs the step)
FORCED = 1


def run_modes(pkg, ieskf, radius, mode_of_step, off_at=None, force_keys=False):
    """lins_streams_map_step with the surround mode on, on two contexts: a selects as mode_of_step(step) says, b on the host.
    Per step what both gave; at the end every stored frame of both."""
    out = []
    with ch.context(pkg, ieskf) as a, ch.context(pkg, ieskf) as b:
        for c in (a, b):
            ch.setup(c)
            sm.init(c, ch.N, ch.INTERVAL)
            sm.surround(c, True, radius, LEAF)
        device_hits = 0
        for step in range(ch.STEPS):
            a.keyposes_set_mode(mode_of_step(step))
            for c in (a, b):
                ch.feed(c, step)
                if force_keys and step > 0:
                    st = sm.get_pose(c, FORCED)
                    st["prev"] = st["prev"] + F(10)
                    sm.set_pose(c, FORCED, st)
                if step == off_at:
                    sm.surround(c, False)
            ra, rb = sm.step(a, STREAMS, ch.odoms(step)), sm.step(b, STREAMS, ch.odoms(step))
            ran = sum(r["status"] != defs.MAP_STEP_SKIPPED for r in ra)
            on = off_at is None or step < off_at
            if on and mode_of_step(step) == DEVICE and ran:
                device_hits += a.keyposes_stats()["hits"]
            out.append(dict(a=ra, b=rb, lists_a=[sm.surround_list(a, s) for s in STREAMS], lists_b=[sm.surround_list(b, s) for s in STREAMS],
                            clouds_a=[[sm.download(a, k, w) for w in range(6)] for k in range(ran)],
                            clouds_b=[[sm.download(b, k, w) for w in range(6)] for k in range(ran)],
                            poses_a=[sm.get_pose(a, s) for s in STREAMS], poses_b=[sm.get_pose(b, s) for s in STREAMS],
                            counts=[(a.archive_count(s), b.archive_count(s)) for s in STREAMS]))
        assert b.keyposes_stats() == dict(device_ms=0.0, host_entries=0, hits=0)  # b never selected on the device ...
        assert device_hits > 0  # ... and a did
        specs = [(s, [i], 7, 0.0, 0) for s in STREAMS for i in range(a.archive_count(s))]
        for c in (a, b):
            c.archive_assemble(specs)
        out.append(dict(frames=[(a.archive_download(k), b.archive_download(k)) for k in range(len(specs))]))
    return out


def assert_same_modes(run):
    for step, o in enumerate(run[:-1]):
        for s in STREAMS:
            assert ch.same_result(o["a"][s], o["b"][s]), (step, s, o["a"][s], o["b"][s])
            assert ch.same_state(o["poses_a"][s], o["poses_b"][s]), (step, s)
            assert o["counts"][s][0] == o["counts"][s][1]
            assert o["lists_a"][s] == o["lists_b"][s], (step, s, o["lists_a"][s], o["lists_b"][s])
        assert len(o["clouds_a"]) == len(o["clouds_b"])
        for k, (p, q) in enumerate(zip(o["clouds_a"], o["clouds_b"])):
            assert all(x.shape == y.shape and np.array_equal(ch.bits(x), ch.bits(y)) for x, y in zip(p, q)), (step, k)
    assert run[-1]["frames"] and all(np.array_equal(ch.bits(p), ch.bits(q)) for p, q in run[-1]["frames"])


def test_surround_step_with_a_list_longer_than_the_ring(pkg, ieskf):
    run = run_modes(pkg, ieskf, 50.0, lambda step: DEVICE, force_keys=True)
    assert_same_modes(run)
    assert max(len(lst) for o in run[:-1] for lst in o["lists_a"]) > ch.WINDOW
    assert any(r["status"] == defs.MAP_STEP_SKIPPED for o in run[:-1] for r in o["a"])
    assert all(r["iters"] > 0 for o in run[1:-1] for r in o["a"] if r["status"] == 0)


def test_surround_step_with_a_small_radius_that_erases(pkg, ieskf):
    run = run_modes(pkg, ieskf, 0.25, lambda step: DEVICE)
    assert_same_modes(run)
    assert sum(any(v not in after["lists_a"][s] for v in before["lists_a"][s]) for before, after in zip(run[:-2], run[1:-1]) for s in STREAMS) > 0


def test_surround_step_with_the_modes_switched_in_mid_sequence(pkg, ieskf):
    """the selection moves between the device and the host from step to step, and the surround mode goes off at step 6"""
    run = run_modes(pkg, ieskf, 50.0, lambda step: DEVICE if step in (0, 1, 4, 5, 7) else HOST, off_at=6, force_keys=True)
    assert_same_modes(run)
    assert run[7]["lists_a"] == run[5]["lists_a"] and any(run[5]["lists_a"])


def test_loop_step_detects_on_the_device(pkg, ieskf):
    kinds = ("loop", "inside", "loop")
    scan = lsc.build_scan()
    got = {}
    with make(pkg, ieskf) as a, make(pkg, ieskf) as b:
        for name, c, mode in (("device", a, DEVICE), ("host", b, HOST)):
            lsc.init(c, 4)  # (slot 3 keeps no frames)
            for s, kind in enumerate(kinds):
                lsc.push(c, s, kind)
            c.keyposes_set_mode(mode)
            res = c.loop_step([(s, lsc.centre(), lsc.NOW) for s in range(4)], lsc.params(ieskf.lib()))
            got[name] = ([lsc.frozen(r) for r in res], [lsc.state_of(c, s, scan) for s in range(3)], [r["outcome"] for r in res],
                         [r["closest_id"] for r in res])
    assert got["device"][0] == got["host"][0] and got["device"][1] == got["host"][1]
    assert got["device"][2] == [defs.LOOP_CLOSED, defs.LOOP_NONE, defs.LOOP_CLOSED, defs.LOOP_NONE]
    assert got["device"][3][1] == got["device"][3][3] == -1 and 0 <= got["device"][3][0] <= 5
