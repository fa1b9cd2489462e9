"""The mapping node's local map on the device (include/lins_map.h lins_local_map_*) against the CPU restatement
(host/local_map.cpp, itself pinned to tests/local_map_np.py by tests/test_local_map_host.py), and scan-to-map on the
built clouds (LINS_MAP_LOCAL) against the same call with the clouds passed explicitly."""
import importlib

import numpy as np
import pytest

from local_map_synth import room_scan, trajectory

pytestmark = pytest.mark.gpu
defs = importlib.import_module("lins---lidar-inertial-slam_amd._ctypes_defs")
host = importlib.import_module("lins---lidar-inertial-slam_amd.host")

SMALL = dict(n_corner=60, n_surf=500, n_outlier=30)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def assert_same_build(ctx, k, frames, scan, got_sizes, window=50):
    want, ws = host.local_map(frames, scan, window)
    assert got_sizes == ws, (k, got_sizes, ws)
    for c in range(6):
        assert np.array_equal(bits(ctx.local_map_download(k, c)), bits(want[c])), (k, c)


def frame(seed, pose, **kw):
    return room_scan(seed, pose, **kw) + (pose,)


@pytest.fixture
def ctx(pkg, ieskf):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    yield c
    c.close()


def test_build_matches_host_for_slots_at_different_fill_levels(ctx):
    poses = trajectory(60, seed=1)
    fills = [0, 1, 49, 50, 53]
    ctx.local_map_init(len(fills), 50, 2048)
    frames = []
    for s, f in enumerate(fills):
        fr = [frame(1000 * s + i, poses[i], **SMALL) for i in range(f)]
        for c, su, o, p in fr:
            ctx.local_map_push(s, c, su, o, p)
        frames.append(fr)
    slots = [0, 1, 2, 3, 4, 2]  # (a slot may serve two entries)
    scans = [room_scan(77 + k, poses[k], **SMALL) for k in range(len(slots))]
    scans[0] = (scans[0][0][:0], scans[0][1], scans[0][2][:0])  # empty clouds
    sizes = ctx.local_map_build(slots, scans)
    for k, s in enumerate(slots):
        assert_same_build(ctx, k, frames[s], scans[k], sizes[k])
    assert sizes[0]["n"][:2] == [0, 0] and sizes[1]["frames"] == 1 and sizes[4]["frames"] == 50
    ms, pts = ctx.local_map_stats()
    assert ms > 0 and pts > 0


def test_build_of_a_full_window_of_room_scans(ctx):
    """50 frames of ~4.6 k points: ~230 k map input points — a multi-pass sort over many workgroups"""
    poses = trajectory(50, seed=2)
    ctx.local_map_init(1, 50, 8192)
    fr = [frame(i, poses[i]) for i in range(50)]
    for c, s, o, p in fr:
        ctx.local_map_push(0, c, s, o, p)
    scan = room_scan(999, poses[10], n_corner=470, n_surf=8200, n_outlier=200)
    sizes = ctx.local_map_build([0], [scan])
    assert sum(len(f[0]) + len(f[1]) + len(f[2]) for f in fr) > 230000
    assert_same_build(ctx, 0, fr, scan, sizes[0])
    assert sizes[0]["n"][1] > 10000


def test_build_with_one_voxel_of_ten_thousand_points(ctx):
    rng = np.random.default_rng(5)
    ctx.local_map_init(2, 50, 32768)
    blob = np.concatenate([0.3 + rng.uniform(0, 0.15, (10000, 3)), rng.uniform(0, 1, (10000, 1))], 1).astype(np.float32)
    lattice = np.stack(np.meshgrid(np.arange(-8, 8), np.arange(-8, 8), np.arange(-2, 2)), -1).reshape(-1, 3) * 0.2
    lat = np.concatenate([lattice, np.ones((len(lattice), 1))], 1).astype(np.float32)
    neg = np.concatenate([-rng.uniform(0, 40, (3000, 3)), np.zeros((3000, 1))], 1).astype(np.float32)
    pose = (1.0, -2.0, 0.5, 0.0, 0.0, 0.0)
    fr = [(blob[:2000], np.concatenate([blob, lat, lat]), neg, pose)]
    ctx.local_map_push(0, *fr[0])
    scans = [(blob, np.concatenate([lat, blob]), neg), (lat, lat, lat)]
    sizes = ctx.local_map_build([0, 1], scans)
    assert_same_build(ctx, 0, fr, scans[0], sizes[0])
    assert_same_build(ctx, 1, [], scans[1], sizes[1])


def test_push_scans_equals_push_of_the_downloaded_clouds_and_set_pose_equals_a_rebuilt_ring(ctx):
    poses = trajectory(12, seed=3)
    ctx.local_map_init(2, 5, 4096)
    for s in range(2):  # the same four frames on both rings
        for i in range(4):
            ctx.local_map_push(s, *frame(i, poses[i], **SMALL))
    scans = [room_scan(50 + k, poses[4 + k], **SMALL) for k in range(2)]
    ctx.local_map_build([0, 1], scans)
    ds = [[ctx.local_map_download(k, c) for c in (2, 3, 4)] for k in range(2)]
    # slot 0 gets the scan on the device, slot 1 the same clouds from the host: twice, so both rings drop a frame
    for rep in range(2):
        ctx.local_map_push_scans([0], [poses[6 + rep]])
        ctx.local_map_push(1, ds[0][0], ds[0][1], ds[0][2], poses[6 + rep])
    probe = room_scan(60, poses[7], **SMALL)
    sz = ctx.local_map_build([0, 1], [probe, probe])
    assert sz[0] == sz[1] and sz[0]["frames"] == 5
    for c in range(6):
        assert np.array_equal(bits(ctx.local_map_download(0, c)), bits(ctx.local_map_download(1, c))), c
    # set_pose: moving the frame one before the newest equals the ring rebuilt with that pose
    newp = poses[6] + np.array([0.1, -0.05, 0.02, 0.01, -0.01, 0.05], np.float32)
    ctx.local_map_set_pose(0, 1, newp)
    ring = [frame(i, poses[i], **SMALL) for i in range(1, 4)] + [tuple(ds[0]) + (newp,), tuple(ds[0]) + (poses[7],)]
    got = ctx.local_map_build([0], [probe])
    assert_same_build(ctx, 0, ring, probe, got[0], window=5)


def test_scan2map_on_the_local_map_matches_explicit_clouds_and_the_oracles(ctx, oracle):
    from oracle import ref

    poses = trajectory(40, seed=4)
    ctx.local_map_init(3, 50, 8192)
    fills = [30, 12, 3]
    for s, f in enumerate(fills):
        for i in range(f):
            ctx.local_map_push(s, *frame(100 * s + i, poses[i], n_corner=300, n_surf=2500, n_outlier=100))
    truth = [poses[f - 1] + np.array([0.05, 0.03, 0.0, 0.0, 0.0, 0.01], np.float32) for f in fills]
    scans = [room_scan(500 + s, truth[s], n_corner=470, n_surf=6000, n_outlier=200) for s in range(3)]
    sizes = ctx.local_map_build([0, 1, 2], scans)
    t0 = [np.array([p[3], p[4], p[5], p[0], p[1], p[2]], np.float32) for p in poses[[f - 1 for f in fills]]]
    got = ctx.scan2map_batch([defs.MapProblem.local(t) for t in t0])
    explicit = []
    for k in range(3):
        cl = [ctx.local_map_download(k, c) for c in range(6)]
        explicit.append(defs.MapProblem(cl[0], cl[1], cl[2], cl[5], t0[k]))
    want = ctx.scan2map_batch(explicit)
    for g, w in zip(got, want):
        assert np.array_equal(bits(g["transform"]), bits(w["transform"]))
        assert (g["iters"], g["converged"], g["degenerate"], g["n_sel"]) == (w["iters"], w["converged"], w["degenerate"], w["n_sel"])
    checks = [oracle.scan2map] + ([ref.scan2map] if ref.available() else [])
    for p, g in zip(explicit, got):
        for fn in checks:
            w = fn(p)
            assert (g["iters"], g["converged"], g["degenerate"], g["n_sel"]) == (w["iters"], w["converged"], w["degenerate"], w["n_sel"])
            assert np.abs(g["transform"] - w["transform"]).max() <= 2e-5
    assert all(s["status"] == 0 for s in sizes) and got[0]["iters"] > 0


def test_closed_loop_local_map_against_the_explicit_loop(pkg, ieskf):
    """build -> scan2map (LINS_MAP_LOCAL) -> the 0.3 m key-frame rule -> push_scans, four slots with their own seeds,
    against the same loop driven through explicit clouds and push — same bits at every step; final poses near truth"""
    n_steps, n = 60, 4
    trajs = [trajectory(n_steps, seed=20 + s) for s in range(n)]
    a = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    b = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    try:
        for c in (a, b):
            c.local_map_init(n, 50, 8192)
        kw = dict(n_corner=300, n_surf=3000, n_outlier=100)
        for s in range(n):  # the first key frame at the true first pose
            f = frame(7000 + 100 * s, trajs[s][0], **kw)
            a.local_map_push(s, *f)
            b.local_map_push(s, *f)
        last_key = [trajs[s][0].copy() for s in range(n)]
        est = [trajs[s][0].copy() for s in range(n)]
        for step in range(1, n_steps):
            scans = [room_scan(8000 + 100 * s + step, trajs[s][step], **kw) for s in range(n)]
            sa = a.local_map_build(list(range(n)), scans)
            sb = b.local_map_build(list(range(n)), scans)
            assert sa == sb
            cl = [[b.local_map_download(k, c) for c in range(6)] for k in range(n)]
            for k in range(n):
                for c in range(6):
                    assert np.array_equal(bits(a.local_map_download(k, c)), bits(cl[k][c])), (step, k, c)
            # guess: the previous estimate moved by the true increment (an odometry prior)
            guess = [est[s] + (trajs[s][step] - trajs[s][step - 1]) for s in range(n)]
            t0 = [np.array([g[3], g[4], g[5], g[0], g[1], g[2]], np.float32) for g in guess]
            ra = a.scan2map_batch([defs.MapProblem.local(t) for t in t0])
            rb = b.scan2map_batch([defs.MapProblem(cl[k][0], cl[k][1], cl[k][2], cl[k][5], t0[k]) for k in range(n)])
            keys, poses = [], []
            for k in range(n):
                assert np.array_equal(bits(ra[k]["transform"]), bits(rb[k]["transform"])), (step, k)
                assert ra[k]["iters"] == rb[k]["iters"] and ra[k]["n_sel"] == rb[k]["n_sel"]
                t = ra[k]["transform"]
                est[k] = np.array([t[3], t[4], t[5], t[0], t[1], t[2]], np.float32)
                if np.linalg.norm(est[k][:3] - last_key[k][:3]) >= 0.3:  # LM:1655-1669 (translation part)
                    keys.append(k), poses.append(est[k])
                    last_key[k] = est[k].copy()
            a.local_map_push_scans(keys, poses)
            for k, p in zip(keys, poses):
                b.local_map_push(k, cl[k][2], cl[k][3], cl[k][4], p)
        for s in range(n):
            assert np.abs(est[s][:3] - trajs[s][-1][:3]).max() < 0.03, (s, est[s], trajs[s][-1])
            assert np.abs(est[s][3:] - trajs[s][-1][3:]).max() < 0.005, (s, est[s], trajs[s][-1])
    finally:
        a.close()
        b.close()


def test_error_paths(pkg, ieskf):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    try:
        e = np.zeros((0, 4), np.float32)
        pt = np.ones((3, 4), np.float32)
        with pytest.raises(ieskf.LinsError, match="-6"):  # build before init
            c.local_map_build([0], [(pt, pt, pt)])
        with pytest.raises(ieskf.LinsError, match="-6"):  # LINS_MAP_LOCAL without a build
            c.scan2map_batch([defs.MapProblem.local(np.zeros(6, np.float32))])
        c.local_map_init(2, 50, 16)
        with pytest.raises(ieskf.LinsError, match="-1"):
            c.local_map_push(2, pt, pt, pt, (0, 0, 0, 0, 0, 0))
        with pytest.raises(ieskf.LinsError, match="-1"):
            c.local_map_build([-1], [(pt, pt, pt)])
        with pytest.raises(ieskf.LinsError, match="-3"):  # over-capacity frame
            c.local_map_push(0, np.ones((10, 4), np.float32), np.ones((7, 4), np.float32), e, (0, 0, 0, 0, 0, 0))
        bad = pt.copy()
        bad[1, 0] = np.nan
        with pytest.raises(ieskf.LinsError, match="-4"):
            c.local_map_push(0, bad, pt, pt, (0, 0, 0, 0, 0, 0))
        with pytest.raises(ieskf.LinsError, match="-4"):
            c.local_map_push(0, pt, pt, pt, (0, 0, np.inf, 0, 0, 0))
        with pytest.raises(ieskf.LinsError, match="-4"):
            c.local_map_build([0], [(pt, bad, pt)])
        with pytest.raises(ieskf.LinsError, match="-1"):
            c.local_map_set_pose(0, 0, (0, 0, 0, 0, 0, 0))  # (an empty ring has no frame of age 0)
        c.local_map_push(0, pt, pt, pt, (0, 0, 0, 0, 0, 0))
        c.local_map_build([0, 1], [(pt, pt, pt), (pt, pt, pt)])
        with pytest.raises(ieskf.LinsError, match="-6"):  # another batch size
            c.scan2map_batch([defs.MapProblem.local(np.zeros(6, np.float32))])
        p = defs.MapProblem.local(np.zeros(6, np.float32))
        p.reuse_resident_map = True
        with pytest.raises(ieskf.LinsError, match="-1"):
            c.scan2map_batch([p, defs.MapProblem.local(np.zeros(6, np.float32))])
        mixed = defs.MapProblem(pt, pt, pt, pt, np.zeros(6, np.float32))
        with pytest.raises(ieskf.LinsError, match="-1"):
            c.scan2map_batch([mixed, defs.MapProblem.local(np.zeros(6, np.float32))])
        r = c.scan2map_batch([defs.MapProblem.local(np.zeros(6, np.float32))] * 2)  # tiny maps: LM:1636 -> iters 0
        assert [x["iters"] for x in r] == [0, 0]
        with pytest.raises(ieskf.LinsError, match="-1"):
            c.local_map_push_scans([2], [(0, 0, 0, 0, 0, 0)])
        with pytest.raises(ieskf.LinsError, match="-3"):  # the scan's DS clouds (3 x 1 point) fit; 16-point frames do not
            c.local_map_init(1, 50, 2)
            c.local_map_build([0], [(pt, pt, pt)])
            c.local_map_push_scans([0], [(0, 0, 0, 0, 0, 0)])
        # a VoxelGrid box of more than 2^31 cells: LINS_E_CAPACITY for that entry, the other entry built
        c.local_map_init(2, 50, 16)
        far = np.array([[-9e5, -9e5, -9e5, 0], [9e5, 9e5, 9e5, 0]], np.float32)
        s = c.local_map_build([0, 1], [(far, pt, pt), (pt, pt, pt)])
        assert s[0]["status"] == -3 and s[0]["n"] == [0] * 6 and s[1]["status"] == 0 and s[1]["n"][2] == 1
        with pytest.raises(ieskf.LinsError, match="-6"):
            c.local_map_push_scans([0], [(0, 0, 0, 0, 0, 0)])
    finally:
        c.close()
