"""The mapping node with loopClosureEnableFlag off on the device (LM:1247-1315): the local map built from a list of
archive frames (include/lins_map.h lins_local_map_build_surround / _surround_streams) against the CPU restatement
(lins_host_surround_map) and against the two calls it composes (lins_archive_assemble, lins_local_map_build); the scans
of large map jobs split at every chunk size; batch independence; scan-to-map on the built clouds; and the step mode
(include/lins_streams_map.h lins_streams_map_surround) against the explicit chain — lins_archive_select_radius,
lins_host_surround_update, lins_local_map_build_surround_streams, the rounds, host transform_update / key_rule, the two
pushes — on a second context, bit for bit in results, lists, clouds and pose states.  Ring window 3, frames of 300 to
1 500 points."""
import importlib

import numpy as np
import pytest

import boot_common as bc
import map_step_chain as ch
from local_map_synth import room_scan, trajectory
from map_step_chain import defs, host, sm

pytestmark = pytest.mark.gpu
PKG = "lins---lidar-inertial-slam_amd"
sl = importlib.import_module(PKG + ".streams_slam")

F = np.float32
WINDOW = 3
SMALL = dict(n_corner=60, n_surf=500, n_outlier=30)
ROOM = dict(n_corner=300, n_surf=1100, n_outlier=100)
CORNER, SURF_OUTLIER = defs.SUBMAP_CORNER, defs.SUBMAP_SURF | defs.SUBMAP_OUTLIER
INT_MAX = 2 ** 31 - 1
bits = ch.bits


def make_frames(n, seed, **kw):
    poses = trajectory(n, seed=seed)
    return [room_scan(100 * seed + i, poses[i], **kw) + (poses[i],) for i in range(n)], poses


@pytest.fixture(scope="module")
def small_frames():
    fr, poses = make_frames(8, 1, **SMALL)
    fr[2] = (fr[2][0], fr[2][1], fr[2][2][:0], fr[2][3])  # a frame without outliers
    fr[4] = (fr[4][0][:1], fr[4][1][:0], fr[4][2][:0], fr[4][3])  # a one-point frame
    return fr, poses


@pytest.fixture
def ctx(pkg, ieskf):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    yield c
    c.close()


def fill(c, slot, frames):
    for i, (co, su, ou, p) in enumerate(frames):
        assert c.archive_push(slot, co, su, ou, p, time=float(i)) == i


def clouds_of(c, k):
    return [c.local_map_download(k, w) for w in range(6)]


def same_clouds(a, b):
    return all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---- 1. the build ---------------------------------------------------------------------------------------------------
LISTS = [[], [3], [0, 1, 2, 3, 4, 5, 6], [5, 0, 3], [2], [4], [4, 2]]


def test_build_against_the_restatement_and_the_calls_it_composes(ctx, small_frames):
    fr, poses = small_frames
    ctx.local_map_init(1, WINDOW, 4096)
    ctx.archive_init(1, 16, 1 << 16)
    fill(ctx, 0, fr)
    for i in range(2):  # the ring holds frames of its own: a surround build neither reads nor changes them
        ctx.local_map_push(0, *fr[i])
    scans = [room_scan(900 + k, poses[k % 8], **SMALL) for k in range(len(LISTS))]
    scans[1] = (scans[1][0][:0], scans[1][1], scans[1][2][:0])
    slots = [0] * len(LISTS)
    sizes = ctx.local_map_build_surround(slots, LISTS, scans)
    got = [clouds_of(ctx, k) for k in range(len(LISTS))]
    assert len(LISTS[2]) > WINDOW
    # the CPU restatement
    for k, lst in enumerate(LISTS):
        want, ws = host.surround_map(fr, lst, scans[k])
        assert sizes[k] == ws, (k, sizes[k], ws)
        assert same_clouds(got[k], want), k
        assert sizes[k]["frames"] == len(lst) and sizes[k]["status"] == 0
    assert sizes[0]["n"][:2] == [0, 0] and sizes[5]["n"][:2] == [1, 0]
    # lins_archive_assemble of the two specs
    specs = [(0, lst, cl, leaf, 0) for lst in LISTS for cl, leaf in ((CORNER, 0.2), (SURF_OUTLIER, 0.4))]
    info = ctx.archive_assemble(specs)
    for k in range(len(LISTS)):
        for w in range(2):
            z = info[2 * k + w]
            assert np.array_equal(bits(ctx.archive_download(2 * k + w)), bits(got[k][w])), (k, w)
            assert (z["n"], z["status"]) == (sizes[k]["n"][w], 0)
            assert z["box_min"] == sizes[k]["box_min"][w] and z["box_dim"] == sizes[k]["box_dim"][w], (k, w)
    # lins_local_map_build's scan clouds; its map side is still the ring of two frames
    ring = ctx.local_map_build(slots, scans)
    for k in range(len(LISTS)):
        assert ring[k]["n"][2:] == sizes[k]["n"][2:] and ring[k]["frames"] == 2
        assert same_clouds(clouds_of(ctx, k)[2:], got[k][2:]), k
    want, ws = host.local_map(fr[:2], scans[3], WINDOW)
    assert ring[3] == ws and same_clouds(clouds_of(ctx, 3), want)


def test_pushes_work_on_a_surround_build(ctx, small_frames):
    fr, poses = small_frames
    ctx.local_map_init(1, WINDOW, 4096)
    ctx.archive_init(1, 16, 1 << 16)
    fill(ctx, 0, fr[:4])
    scan = room_scan(950, poses[4], **SMALL)
    ctx.local_map_build_surround([0], [[1, 3]], [scan])
    ds = clouds_of(ctx, 0)[2:5]
    ctx.local_map_push_scans([0], [poses[4]])
    assert ctx.archive_push_scans([0], [poses[4]], [4.0]) == [4]
    new = tuple(ds) + (poses[4],)
    sizes = ctx.local_map_build_surround([0], [[4, 0]], [scan])
    want, ws = host.surround_map(fr[:4] + [new], [4, 0], scan)
    assert sizes[0] == ws and same_clouds(clouds_of(ctx, 0), want)
    sizes = ctx.local_map_build([0], [scan])  # the ring got the frame too
    want, ws = host.local_map([new], scan, WINDOW)
    assert sizes[0] == ws and same_clouds(clouds_of(ctx, 0), want)


def test_split_scans_give_the_same_bits_at_every_chunk(ctx):
    fr, poses = make_frames(7, 2, n_corner=200, n_surf=1200, n_outlier=100)
    ctx.local_map_init(2, WINDOW, 4096)
    ctx.archive_init(2, 8, 1 << 16)
    fill(ctx, 0, fr)
    fill(ctx, 1, fr[:2])
    lists = [list(range(7)), [1, 0]]
    scans = [room_scan(960 + k, poses[k], **SMALL) for k in range(2)]
    assert sum(len(f[1]) + len(f[2]) for f in fr) > 16 * 512 and sum(len(f[0]) for f in fr) > 1024  # (17 and 3 tiles)
    want = [host.surround_map(fr, lists[0], scans[0]), host.surround_map(fr[:2], lists[1], scans[1])]
    for chunk in (1, 2, 0, INT_MAX):  # every map job split; the surf job alone (and entry 1's not); the default; none
        ctx.archive_set_scan_chunk(chunk)
        sizes = ctx.local_map_build_surround([0, 1], lists, scans)
        for k in range(2):
            assert sizes[k] == want[k][1], (chunk, k, sizes[k], want[k][1])
            assert same_clouds(clouds_of(ctx, k), want[k][0]), (chunk, k)
    assert want[0][1]["n"][1] > 1024


def test_batch_independence(ctx, small_frames):
    fr, poses = small_frames
    other, _ = make_frames(5, 3, **SMALL)
    ctx.local_map_init(3, WINDOW, 4096)
    ctx.archive_init(3, 16, 1 << 16)
    fill(ctx, 0, fr)
    fill(ctx, 2, other)  # (slot 1's archive stays empty)
    x = (0, [5, 0, 3], room_scan(970, poses[2], **SMALL))
    y = (2, [4, 1, 2, 0], room_scan(971, poses[5], **SMALL))
    e = (1, [], room_scan(972, poses[0], **SMALL))

    def build(entries):
        sizes = ctx.local_map_build_surround([t[0] for t in entries], [t[1] for t in entries], [t[2] for t in entries])
        return [(sizes[k], clouds_of(ctx, k)) for k in range(len(entries))]

    alone = build([x])[0]
    first, last = build([x, e, y]), build([y, e, x])
    for got in (first[0], last[2]):
        assert got[0] == alone[0] and same_clouds(got[1], alone[1])
    assert first[2][0] == last[0][0] and same_clouds(first[2][1], last[0][1])
    assert first[1][0]["n"][:2] == [0, 0] and first[1][0]["frames"] == 0 and first[1][0]["n"][2] > 0
    assert alone[0] == host.surround_map(fr, x[1], x[2])[1]


def test_scan2map_on_a_surround_build_equals_the_explicit_problem(ctx):
    fr, poses = make_frames(9, 4, **ROOM)
    ctx.local_map_init(2, WINDOW, 4096)
    ctx.archive_init(2, 16, 1 << 16)
    fill(ctx, 0, fr)
    fill(ctx, 1, fr[:3])
    lists = [[6, 0, 1, 2, 3, 4, 5], [2, 0]]
    at = [6, 2]
    truth = [poses[i] + np.array([0.05, 0.03, 0.0, 0.0, 0.0, 0.01], F) for i in at]
    scans = [room_scan(980 + k, truth[k], n_corner=300, n_surf=1500, n_outlier=100) for k in range(2)]
    sizes = ctx.local_map_build_surround([0, 1], lists, scans)
    t0 = [np.array([p[3], p[4], p[5], p[0], p[1], p[2]], F) for p in poses[at]]
    got = ctx.scan2map_batch([defs.MapProblem.local(t) for t in t0])
    explicit = []
    for k in range(2):
        cl = clouds_of(ctx, k)
        explicit.append(defs.MapProblem(cl[0], cl[1], cl[2], cl[5], t0[k]))
    want = ctx.scan2map_batch(explicit)
    for g, w in zip(got, want):
        assert np.array_equal(bits(g["transform"]), bits(w["transform"]))
        assert (g["iters"], g["converged"], g["degenerate"], g["n_sel"]) == (w["iters"], w["converged"], w["degenerate"], w["n_sel"])
    assert all(s["status"] == 0 for s in sizes) and all(g["iters"] > 0 for g in got)


# ---- 2. the step ----------------------------------------------------------------------------------------------------
STREAMS = [0, 1, 2]
LEAF = 0.02  # (every key pose its own voxel: the list is the radius search's answer)
FORCED = 1  # the stream whose every scan is made a key frame (previousRobotPosPoint moved 10 m away before each step)


class Chain:
    """context b as tests/map_step_chain.explicit_step sees it: its "local map" call is the explicit surround chain —
    lins_archive_select_radius around the remembered centre, lins_host_surround_update, one
    lins_local_map_build_surround_streams — with lists and centres kept here"""

    def __init__(self, c, radius, leaf):
        self.c, self.radius, self.leaf = c, radius, leaf
        self.lists = {s: [] for s in STREAMS}
        self.centre = {s: np.zeros(3, F) for s in STREAMS}

    def __getattr__(self, name):
        return getattr(self.c, name)

    def local_map_build_streams(self, slots, streams):
        new = []
        for s in slots:
            have = self.c.archive_count(s)
            ds = self.c.archive_select_radius(s, self.centre[s], self.radius, self.leaf).tolist() if have else []
            new.append(host.surround_update(self.lists[s] if have else [], ds))
        sizes = self.c.local_map_build_surround_streams(slots, new, streams)
        for s, lst, z in zip(slots, new, sizes):
            if z["status"] == 0:
                self.lists[s] = lst
        return sizes

    def note(self, streams, res):
        for s, r in zip(streams, res):
            if r["status"] == 0:
                self.centre[s] = r["transform"][3:6].copy()  # currentRobotPosPoint (LM:1655-1658)


def step_clouds(c, n, step_call):
    get = (lambda k, w: sm.download(c, k, w)) if step_call else c.local_map_download
    return [[get(k, w) for w in range(6)] for k in range(n)]


def run_pair(pkg, ieskf, radius, steps=ch.STEPS, off_at=None, force_keys=False):
    """context a: lins_streams_map_step with the mode on (off from step off_at on); context b: the explicit chain (the
    recent-frame chain from off_at on).  Per step what both gave.  force_keys: stream FORCED stores every scan."""
    out = []
    with ch.context(pkg, ieskf) as a, ch.context(pkg, ieskf) as b:
        for c in (a, b):
            ch.setup(c)
        sm.init(a, ch.N, ch.INTERVAL)
        sm.surround(a, True, radius, LEAF)
        chain = Chain(b, radius, LEAF)
        states = [ch.fresh_state() for _ in STREAMS]
        for step in range(steps):
            for c in (a, b):
                ch.feed(c, step)
            on = off_at is None or step < off_at
            if force_keys and step > 0:
                st = sm.get_pose(a, FORCED)
                st["prev"] = st["prev"] + F(10)
                sm.set_pose(a, FORCED, st)
                states[FORCED]["prev"] = states[FORCED]["prev"] + F(10)
            if step == off_at:
                sm.surround(a, False)
            ra = sm.step(a, STREAMS, ch.odoms(step))
            rb = ch.explicit_step(chain if on else b, states, STREAMS, ch.odometry(step))
            chain.note(STREAMS, rb)
            ran = sum(r["status"] != defs.MAP_STEP_SKIPPED for r in ra)
            out.append(dict(on=on, a=ra, b=rb, lists_a=[sm.surround_list(a, s) for s in STREAMS], lists_b=[list(chain.lists[s]) for s in STREAMS],
                            clouds_a=step_clouds(a, ran, True), clouds_b=step_clouds(b, ran, False), poses_a=[sm.get_pose(a, s) for s in STREAMS],
                            poses_b=[dict(s) for s in states], counts=[(a.archive_count(s), b.archive_count(s)) for s in STREAMS]))
            print("step %d radius %g lists %s key %s" % (step, radius, out[-1]["lists_a"], [r["key_frame"] for r in ra]))
        # the stored frames: every archive frame of both contexts, as one unfiltered cloud each
        specs = [(s, [i], CORNER | SURF_OUTLIER, 0.0, 0) for s in STREAMS for i in range(a.archive_count(s))]
        for c in (a, b):
            c.archive_assemble(specs)
        out.append(dict(frames=[(a.archive_download(k), b.archive_download(k)) for k in range(len(specs))]))
    return out


def assert_same_pair(run):
    for step, o in enumerate(run[:-1]):
        for s in STREAMS:
            assert ch.same_result(o["a"][s], o["b"][s]), (step, s, o["a"][s], o["b"][s])
            assert ch.same_state(o["poses_a"][s], o["poses_b"][s]), (step, s)
            assert o["counts"][s][0] == o["counts"][s][1]
            if o["on"]:
                assert o["lists_a"][s] == o["lists_b"][s], (step, s, o["lists_a"][s], o["lists_b"][s])
        assert len(o["clouds_a"]) == len(o["clouds_b"])
        for k, (p, q) in enumerate(zip(o["clouds_a"], o["clouds_b"])):
            assert same_clouds(p, q), (step, k)
    assert run[-1]["frames"] and all(np.array_equal(bits(p), bits(q)) for p, q in run[-1]["frames"])


@pytest.fixture(scope="module")
def wide_run(pkg, ieskf):
    return run_pair(pkg, ieskf, 50.0, force_keys=True)


def test_step_equals_the_explicit_chain(wide_run):
    assert_same_pair(wide_run)
    lists = [o["lists_a"][s] for o in wide_run[:-1] for s in STREAMS]
    assert max(len(lst) for lst in lists) > ch.WINDOW  # a map of more frames than the ring holds
    assert [o["a"][FORCED]["key_frame"] for o in wide_run[:-1]] == [1] * ch.STEPS
    assert all(r["iters"] > 0 for o in wide_run[1:-1] for r in o["a"] if r["status"] == 0)
    assert any(r["status"] == defs.MAP_STEP_SKIPPED for o in wide_run[:-1] for r in o["a"])  # a gated entry keeps its list
    o3, o4 = wide_run[3], wide_run[4]
    assert o4["a"][2]["status"] == defs.MAP_STEP_SKIPPED and o4["lists_a"][2] == o3["lists_a"][2]


def test_step_with_a_small_radius_erases(pkg, ieskf):
    """radius 0.25 m against the key-frame rule's 0.3 m: once a stream stores its next key frame, the one before it is
    out of reach of the new centre — it leaves the list then, if a step between the two has not erased it already"""
    run = run_pair(pkg, ieskf, 0.25)
    assert_same_pair(run)
    erased = 0
    for before, after in zip(run[:-2], run[1:-1]):
        for s in STREAMS:
            erased += any(v not in after["lists_a"][s] for v in before["lists_a"][s])
    assert erased > 0


def test_mode_switched_off_in_mid_sequence_continues_with_the_ring(pkg, ieskf):
    run = run_pair(pkg, ieskf, 50.0, steps=6, off_at=4)
    assert_same_pair(run)
    assert [o["on"] for o in run[:-1]] == [True] * 4 + [False] * 2
    assert all(o["a"][s]["status"] == 0 and o["a"][s]["iters"] > 0 for o in run[4:-1] for s in (0, 1))
    # the list stays as the last surround step left it
    assert run[5]["lists_a"] == run[3]["lists_a"]


def test_slam_step_with_the_mode_on_equals_process_raw_and_the_step(pkg, ieskf):
    sweeps = 6
    data = [bc.load(host, s, sweeps) for s in bc.SEQS]
    n = len(data)
    streams = list(range(n))
    with ch.context(pkg, ieskf, n) as a, ch.context(pkg, ieskf, n) as b:
        for c in (a, b):
            c.streams_init(n)
            c.streams_machine_init()
            c.local_map_init(n, WINDOW, ch.MAX_PTS)
            c.archive_init(n, 2 * sweeps, 1 << 19)
            sm.init(c, n, 0.1)
            sm.surround(c, True, 50.0, LEAF)
        stepped = 0
        for k in range(sweeps):
            raws, rows, t = [d["raws"][k] for d in data], [d["rows"][k] for d in data], [bc.scan_time(k)] * n
            _, st_a, map_a, _ = sl.slam_step(a, raws, rows, t)
            st_b = b.streams_process_raw(raws, rows, t)[3]
            assert list(st_a) == list(st_b)
            recs = sl.odometry(b)
            run = [s for s in streams if st_b[s] == 3]  # RUNNING
            map_b = [ch.skipped() for _ in streams]
            if run:
                for s, r in zip(run, sm.step(b, run, [sm.odom(recs[s]["transform_sum"], t[s]) for s in run])):
                    map_b[s] = r
            for s in streams:
                assert ch.same_result(map_a[s], map_b[s]), (k, s, map_a[s], map_b[s])
                assert sm.surround_list(a, s) == sm.surround_list(b, s)
                assert ch.same_state(sm.get_pose(a, s), sm.get_pose(b, s))
                stepped += map_a[s]["status"] == 0
        assert stepped >= 3 and any(sm.surround_list(a, s) for s in streams)


# ---- 3. the contract ------------------------------------------------------------------------------------------------
def test_mode_contract(pkg, ieskf):
    with ch.context(pkg, ieskf) as c:
        ch.setup(c, archive=False)
        with pytest.raises(RuntimeError, match="-6"):  # before lins_streams_map_init
            sm.surround(c, True)
        sm.init(c, ch.N, ch.INTERVAL)
        with pytest.raises(RuntimeError, match="-6"):  # without an archive
            sm.surround(c, True)
        sm.surround(c, False)
        assert sm.surround_list(c, 0) == []
    with ch.context(pkg, ieskf) as c:
        ch.setup(c)
        sm.init(c, ch.N, ch.INTERVAL)
        c.pose_graph_init(ch.N, 2 * ch.STEPS, 2)
        for bad in ((-1.0, 1.0), (float("nan"), 1.0), (50.0, 0.0), (50.0, float("nan"))):
            with pytest.raises(RuntimeError, match="-1"):
                sm.surround(c, True, *bad)
        sm.loop(c, True)
        with pytest.raises(RuntimeError, match="-6"):  # the node's flag selects one of the two
            sm.surround(c, True)
        sm.loop(c, False)
        sm.surround(c, True)
        with pytest.raises(RuntimeError, match="-6"):
            sm.loop(c, True)
        sm.surround(c, False)
        sm.loop(c, True)
        with pytest.raises(RuntimeError, match="-1"):
            sm.surround_list(c, ch.N)
        # switching on clears every list, and lins_streams_map_init switches the mode off
        sm.loop(c, False)
        sm.surround(c, True, 50.0, LEAF)
        for step in range(2):
            ch.feed(c, step)
            sm.step(c, STREAMS, ch.odoms(step))
        assert all(sm.surround_list(c, s) == [0] for s in STREAMS)
        sm.surround(c, True, 50.0, LEAF)
        assert all(sm.surround_list(c, s) == [] for s in STREAMS)
        sm.init(c, ch.N, ch.INTERVAL)  # (the archive keeps its frames: a step with the mode still on would list some)
        ch.feed(c, 2)
        res = sm.step(c, STREAMS, ch.odoms(2))
        assert all(r["status"] == 0 for r in res) and all(sm.surround_list(c, s) == [] for s in STREAMS)


def test_build_contract_and_a_refused_call_changes_nothing(pkg, ieskf, small_frames):
    fr, poses = small_frames
    scan = room_scan(990, poses[1], **SMALL)
    make = lambda: ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    with make() as c:
        with pytest.raises(RuntimeError, match="-6"):  # neither store
            c.local_map_build_surround([0], [[]], [scan])
        c.archive_init(1, 16, 1 << 16)
        with pytest.raises(RuntimeError, match="-6"):  # no local map
            c.local_map_build_surround([0], [[]], [scan])
    with make() as c:
        c.local_map_init(2, WINDOW, 4096)
        with pytest.raises(RuntimeError, match="-6"):  # no archive
            c.local_map_build_surround([0], [[]], [scan])
    with make() as c, make() as fresh:
        for x in (c, fresh):
            x.local_map_init(2, WINDOW, 4096)
            x.archive_init(1, 16, 1 << 16)
            fill(x, 0, fr[:4])
        first = c.local_map_build_surround([0], [[1, 2]], [scan])
        kept = clouds_of(c, 0)
        for slots, ids in (([0], [[4]]), ([0], [[0, -1]]), ([1], [[]]), ([-1], [[]]), ([2], [[]]), ([0, 0], [[1], [1, 7]])):
            with pytest.raises(RuntimeError, match="-1"):  # an id that is no frame; a slot that is not one of both stores
                c.local_map_build_surround(slots, ids, [scan] * len(slots))
        # the last build is still there, as it was
        c._local_sizes = first
        assert same_clouds(clouds_of(c, 0), kept)
        # ... and the next build gives the bits of a context that never saw the refusals
        got, want = c.local_map_build_surround([0], [[3, 0]], [scan]), fresh.local_map_build_surround([0], [[3, 0]], [scan])
        assert got == want and same_clouds(clouds_of(c, 0), clouds_of(fresh, 0))
        assert got[0] == host.surround_map(fr[:4], [3, 0], scan)[1]
