"""The device calls of the mapping node's bookkeeping DIRECTLY against the reference's compiled text
(oracle/_ref/liblins_ref_mapnode.so, which travels with the repository snapshot; nothing here reads the reference's tree):
the cases of tests/test_ref_mapnode.py with the device in the host restatement's place.

    local_map_build, local_map_build_surround (+ keyposes_surround_batch)   extractSurroundingKeyFrames, both branches
    keyposes_find_loop_batch (65 entries once), keyposes_select_batch, archive_assemble   detectLoopClosure, publishGlobalMap
    streams_map.step                                                       run(): the sequence, three streams
    pose_graph_apply                                                        correctPoses
    loop_step                                                               performLoopClosure: detection and glue

Clouds, ids and decisions are bit for bit (VoxelGrid centroids of three or more points: the bound of
tests/ref_mapnode_cases.py).  Where the device differs from the host by ocml against glibc the bars are the ones the
project already holds it to, imported: 4 x map_pose_cases.E_HOST_* for the map-pose angles (tests/test_gpu_map_pose.py),
map_synth.SCAN2MAP_BAR (tests/test_gpu_map_rounds.py's BAR) for the scan-to-map transform.  One bar is neither of those two:
pose_graph_apply's f32 fields are held to the bar tests/test_ref_mapnode.py holds the HOST's correctPoses to
(ref_mapnode_cases.BAR x E_CORRECT_REL, relative: the reference side's one rounding to f32 against longdouble, times 4) —
the device extracts the angles with ocml where the node uses libm, then both round once."""
import importlib
import os

import numpy as np
import pytest

import archive_np
import map_pose_cases as mpc
import map_pose_np as mp
import map_step_chain as ch
import ref_mapnode_cases as rc
from ref_mapnode_cases import F, bits, same_bits
from map_synth import SCAN2MAP_BAR as ROUNDS_BAR
from ref_mapnode_cases import BAR as CORRECT_BAR, E_CORRECT_REL

pytestmark = pytest.mark.gpu
PKG = "lins---lidar-inertial-slam_amd"
host = importlib.import_module(PKG + ".host")
sm = importlib.import_module(PKG + ".streams_map")
defs = importlib.import_module(PKG + "._ctypes_defs")
WAVE_PLUS_ONE = 65


@pytest.fixture(scope="module")
def m():
    from oracle import ref_mapnode as r

    if not r.available():
        if os.environ.get("LINS_REQUIRE_REF") == "1":
            pytest.fail("LINS_REQUIRE_REF=1 and oracle/_ref/liblins_ref_mapnode.so is neither built nor buildable here")
        pytest.skip("oracle/_ref/liblins_ref_mapnode.so not built and the reference is not present")
    r.lib()
    return r


@pytest.fixture
def ctx(pkg, ieskf):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    yield c
    c.close()


def build_clouds(c, k=0):
    return [c.local_map_download(k, w) for w in range(6)]


# ---- c. extractSurroundingKeyFrames, loop closure on: lins_local_map_build ------------------------------------------------------
@pytest.mark.parametrize("non_key_between", [0, 2])
def test_local_map_build_against_the_node(m, ctx, non_key_between):
    """The ring of 50 against the node's deque at every scan up to 60 key frames.  With a key frame at every scan the two hold
    the same frames throughout.  With scans between that are no key frames the reference doubles its newest frame at 50
    (tests/test_ref_mapnode.py: the stated departure); there the device is held to the project's rule — the last 50 frames,
    each once — bit for bit, and the node's map is shown to be another."""
    n_key = 61 if non_key_between == 0 else 60  # (the scan that makes frame k + 1 sees k: a map of 60 frames either way)
    ctx.local_map_init(1, 50, 256)
    poses = rc.line_poses(n_key + 1, 1.0, seed=7)
    d, model = rc.Driven(loop=True), rc.RefDeque()
    seen = dict(same=0, departed=0, loose=0, counts=set(), all_counts=set())
    scan_now = [None]

    def check(node):
        K = node.scalars()["key_frames"]
        ids, ours = model.extract(K), list(range(max(0, K - 50), K))
        seen["all_counts"].add(K)
        frames = node.frames()
        sizes = ctx.local_map_build([0], [scan_now[0]])[0]
        assert sizes["status"] == 0 and sizes["frames"] == len(ours)
        got = build_clouds(ctx)
        seen["loose"] += rc.check_scan_side(m, node, scan_now[0], got, K)
        if ids == ours:
            seen["loose"] += rc.check_map_side(m, node, frames, ids, got, K)
            seen["same"] += 1
            seen["counts"].add(K)
        else:  # the departure: the node's frames are not the project's
            assert sorted(set(ids)) != ours and len(ids) == 50
            rc.check_map_side(m, node, frames, ids, host.local_map([frames[i] for i in ids], scan_now[0], 50)[0], K)  # the node, on its own frames
            corner, surf = rc.map_inputs(frames, ours)
            assert same_bits(got[0], rc.lm.voxel_grid(corner, 0.2)) and same_bits(got[1], rc.lm.voxel_grid(surf, 0.4))  # the device, on the project's
            assert not same_bits(node.cloud(m.MAP_CORNER), corner)
            seen["departed"] += 1

    for k in range(n_key):
        scan_now[0] = rc.small_scan(100 + k, poses[k], frame_id=k)
        assert d.step(scan_now[0], rc.six(poses[k]), before_save=check)
        ctx.local_map_push(0, *d.node.key_frame(k), d.node.frames()[k][3])
        for j in range(non_key_between):
            p = rc.six(poses[k])
            p[3] += F(0.05 * (j + 1))
            scan_now[0] = rc.small_scan(500 + k, poses[k], frame_id=k)
            assert not d.step(scan_now[0], p, before_save=check)
    print("local_map_build against the node:", {k: v for k, v in seen.items() if "counts" not in k})
    assert {1, 2, 49}.issubset(seen["counts"]) and seen["same"] > 50 and 60 in seen["all_counts"]
    if non_key_between == 0:
        assert seen["departed"] == 0 and {50, 51, 60}.issubset(seen["counts"])
    else:
        assert seen["departed"] >= 2 * 10  # from the second scan at 50 frames on


# ---- d. loop closure off: lins_keyposes_surround_batch, lins_local_map_build_surround ---------------------------------------
@pytest.mark.parametrize("mode", ["host", "device"])
def test_surround_list_and_build_against_the_node(m, ctx, mode):
    ctx.keyposes_set_mode(defs.KEYPOSES_DEVICE if mode == "device" else defs.KEYPOSES_HOST)
    xs = np.concatenate([np.arange(0, 120, 6.0), 120 + 0.4 * np.arange(1, 8), np.arange(120, -1, -8.0)])
    rng = np.random.default_rng(3)
    poses = np.zeros((len(xs), 6), F)
    poses[:, 0], poses[:, 1], poses[:, 5] = xs, rng.uniform(-0.3, 0.3, len(xs)), rng.uniform(-3, 3, len(xs))
    ctx.local_map_init(1, 3, 256)
    ctx.archive_init(1, len(xs) + 1, 256 * (len(xs) + 1))
    d = rc.Driven(loop=False)
    lst, seen, scan_now = [], dict(erased=0, reentered=0, loose=0, max_len=0), [None]

    def check(node):
        nonlocal lst
        frames = node.frames()
        if not frames:
            return
        centre = node.floats(m.P_CURRENT)[:3]
        new, res = ctx.keyposes_surround_batch([(0, centre, 50.0, 1.0)], [lst])
        assert res[0]["status"] == 0 and new[0] == node.surround_list(), (lst, new[0], node.surround_list())
        seen["erased"] += any(v not in new[0] for v in lst[:-1])
        seen["reentered"] += len(frames) > 25 and any(v < len(frames) - 15 for v in new[0])
        lst = new[0]
        seen["max_len"] = max(seen["max_len"], len(lst))
        sizes = ctx.local_map_build_surround([0], [lst], [scan_now[0]])[0]
        assert sizes["status"] == 0 and sizes["frames"] == len(lst)
        got = build_clouds(ctx)
        seen["loose"] += rc.check_map_side(m, node, frames, lst, got) + rc.check_scan_side(m, node, scan_now[0], got)

    for k in range(len(xs)):
        scan_now[0] = rc.small_scan(k, poses[k], frame_id=k)
        assert d.step(scan_now[0], rc.six(poses[k]), before_save=check)
        f = d.node.frames()[k]
        assert ctx.archive_push(0, *f, time=d.time) == k
    print("surround against the node:", mode, seen)
    assert seen["erased"] > 0 and seen["reentered"] > 0 and 5 < seen["max_len"] < len(xs)


# ---- e, i. detectLoopClosure, publishGlobalMap: lins_keyposes_find_loop_batch, _select_batch, lins_archive_assemble ----------
def _archive_on_both(m, c, poses, times, scans=None, slot=0):
    d = rc.Driven(loop=True)
    for k, p in enumerate(poses):
        d.time = float(times[k])
        assert d.step(scans[k] if scans else rc.small_scan(40 + k, p), rc.six(p)), k
    frames = d.node.frames()
    for k, f in enumerate(frames):
        assert c.archive_push(slot, *f, time=float(times[k])) == k
    return d.node, frames


def test_find_loop_batch_of_65_and_the_submaps_against_the_node(m, ctx):
    poses = rc.line_poses(40, 0.5, seed=4)
    poses[39, :3] = poses[3, :3] + np.array([0.1, 0.0, 0.0], F)
    times = np.r_[np.arange(39) * 1.0, 100.0]
    scans = [rc.small_scan(40 + k, poses[k]) for k in range(40)]
    spaced = np.zeros((8, 4), F)
    spaced[:, 0], spaced[:, 1] = 3.0 * np.arange(8), 1.0
    spaced[:, 3] = [-1.0, -0.5, -0.0, 0.0, 5.0, -2.5, -0.999, 1e-3]
    scans[39] = (spaced.copy(), spaced[::-1].copy() + F(0.5), scans[39][2])
    ctx.archive_init(1, 64, 1 << 14)
    node, frames = _archive_on_both(m, ctx, poses, times, scans)
    # 65 queries in one batch — a second wave with a single lane: the four gaps around 30 s seen from frame 20's own place
    # (saved at t = 20: at 29.5 and 30.0 s it is inside the gap and an older neighbour is the candidate, at 30.5 and 31.0 s it
    # is the candidate itself), no candidate at all, the two windows below, then centres along the walk at times that put some
    # of the frames in reach inside the gap and some outside
    rng = np.random.default_rng(21)
    queries = [(poses[20, :3].copy(), 20.0 + gap) for gap in (29.5, 30.0, 30.5, 31.0)]
    queries += [(np.array([1000.0, 0, 0], F), 100.0), (poses[30, :3] + F(0.05), 100.0), (poses[39, :3].copy(), 100.0)]
    while len(queries) < WAVE_PLUS_ONE:
        k = int(rng.integers(0, 40))
        queries.append(((poses[k, :3] + rng.uniform(-0.4, 0.4, 3)).astype(F), float(rng.uniform(20.0, 80.0))))
    got = ctx.keyposes_find_loop_batch([(0, c, 5.0, now, 30.0) for c, now in queries])
    want = []
    for c, now in queries:
        node.set_floats(m.P_CURRENT, np.r_[c, F(0)])
        node.set_time(now)
        want.append(node.scalars()["closestHistoryFrameID"] if node.detect_loop() else -1)
    assert got == want
    assert want[2:4] == [20, 20] and 0 <= want[0] < 20 and 0 <= want[1] < 20 and want[4] == -1 and want[5] == 30 and want[6] == 3 and len(set(want)) > 10
    # the submaps of two of them: the window clipped at 0 (closest 3) and at the latest id (closest 30)
    loose = 0
    for q in (6, 5):
        c, now = queries[q]
        node.set_floats(m.P_CURRENT, np.r_[c, F(0)])
        node.set_time(now)
        assert node.detect_loop()
        latest, hist = archive_np.latest_spec(40), archive_np.history_spec(40, want[q])
        info = ctx.archive_assemble([dict(slot=0, **latest), dict(slot=0, **hist)])
        assert [i["status"] for i in info] == [0, 0]
        assert same_bits(ctx.archive_download(0), node.cloud(m.LOOP_LATEST))
        raw, _ = archive_np.submap(frames, hist["ids"], hist["clouds"], 0.0)
        assert same_bits(node.cloud(m.LOOP_HISTORY), raw)
        loose += rc.assert_voxel_cloud(node.cloud(m.LOOP_HISTORY_DS), ctx.archive_download(1), raw, 0.4, q)
        assert (hist["ids"][0], hist["ids"][-1]) == ((0, 28) if q == 6 else (5, 39))
    kept = node.cloud(m.LOOP_LATEST)[:, 3]
    assert len(kept) == 13 and not (kept <= -1.0).any() and (kept == F(-0.5)).any()  # LM:1080: (int) truncates
    print(f"find_loop batch of {len(queries)}: {sum(w >= 0 for w in want)} candidates; history windows: {loose} voxels of >= 3 points differ in the last bits")


def test_global_map_against_the_node(m, ctx):
    poses = rc.line_poses(45, 13.0, seed=16)
    poses[10:16, 0] = poses[10, 0] + 0.3 * np.arange(6)
    ctx.archive_init(1, 64, 1 << 14)
    node, frames = _archive_on_both(m, ctx, poses, np.arange(45.0))
    centre = node.floats(m.P_CURRENT)[:3]
    ids, res = ctx.keyposes_select_batch([(0, centre, 500.0, 1.0)])
    assert res[0]["status"] == 0 and 0 not in ids[0] and len(ids[0]) < 39
    assert np.array_equal(ids[0], ctx.archive_select_radius(0, centre, 500.0, 1.0))
    info = ctx.archive_assemble([dict(slot=0, ids=ids[0], clouds=archive_np.ALL, leaf=0.4, flags=0)])
    assert info[0]["status"] == 0 and info[0]["frames"] == len(ids[0])
    raw, _ = archive_np.submap(frames, ids[0], archive_np.ALL, 0.0)
    got = node.global_map()
    loose = rc.assert_voxel_cloud(got, ctx.archive_download(0), raw, 0.4)
    print(f"global map: {len(got)} points of {len(raw)} from {len(ids[0])} frames, {loose} voxels of >= 3 points differ in the last bits")
    assert len(got) > 100


# ---- g. correctPoses: lins_pose_graph_apply --------------------------------------------------------------------------------------
def test_pose_graph_apply_against_correct_poses(m, ctx):
    """a chain of 30 frames with two loop factors solved ON THE DEVICE; its f64 estimate written into the node, correctPoses();
    the node's key poses against the poses the device applied to its archive — the f32 fields bit for bit (one rounding of
    the same f64 numbers on both sides; the angle extraction is libm's on the node and ocml's on the device only inside the
    solve, which the node does not run) — and the archive's submap after the apply against the node's history cloud"""
    rng = np.random.default_rng(12)
    poses = rc.line_poses(30, 2.0, seed=12)
    poses[:, 3:5] = rng.uniform(-1.0, 1.0, (30, 2))
    ctx.archive_init(1, 32, 1 << 14)
    node, frames = _archive_on_both(m, ctx, poses, np.arange(30.0))
    ctx.pose_graph_init(1, 32, 4)
    six = [rc.six(f[3]) for f in frames]
    for k in range(30):
        assert ctx.pose_graph_push(0, six[k - 1] if k else None, six[k]) == k
    for latest, closest in ((29, 2), (20, 5)):
        ctx.pose_graph_add_loop(0, latest, closest, poses[closest] + np.array([0.3, -0.2, 0.1, 0.01, -0.02, 0.015], F), 0.2)
    assert ctx.pose_graph_solve([0])[0]["iterations"] > 0
    ctx.pose_graph_apply(0)
    est = ctx.debug_pose_graph_poses_f64(0)
    ours = ctx.pose_graph_poses(0)
    node.set_estimate(est)
    node.stage(m.CORRECT)
    p3, p6, t = node.key_poses()
    got = p6[:, [0, 1, 2, 4, 5, 6]]
    assert np.abs(got[:, :3] - poses[:, :3]).max() > 1e-3
    # frame 0 is the prior: the device keeps its f32 bits, the node re-extracts them from R — within one rounding
    same = (bits(ours) == bits(got))
    print(f"pose_graph_apply: {int(same.sum())} of {same.size} fields bit-equal; largest difference {float(np.abs(ours.astype(np.float64) - got).max()):.3g}")
    # (ocml's asin / atan2 against libm's before the one rounding to f32: the bar tests/test_ref_mapnode.py holds the host to)
    assert (np.abs(ours.astype(np.float64) - got.astype(np.float64)) <= CORRECT_BAR * E_CORRECT_REL * np.abs(got.astype(np.float64))).all()
    assert same[:, :3].all()  # the translations: no transcendental on either side
    # the archive after the apply: the window around frame 3 assembled from the poses each side holds.  The node's is the
    # numpy model of ITS corrected poses; the device's is held to the model of the poses the device applied — one and the same
    # comparison wherever the two sets of poses are bit-equal, and then the device's cloud is also held to the node's directly
    node.set_floats(m.P_CURRENT, np.r_[got[3, :3], F(0)])
    node.set_time(100.0)
    assert node.detect_loop()
    closest = node.scalars()["closestHistoryFrameID"]
    hist = archive_np.history_spec(30, closest)
    ctx.archive_assemble([dict(slot=0, **hist)])
    node_frames = node.frames()
    raw, _ = archive_np.submap(node_frames, hist["ids"], hist["clouds"], 0.0)
    assert same_bits(node.cloud(m.LOOP_HISTORY), raw)
    dev_frames = [f[:3] + (tuple(float(v) for v in ours[k]),) for k, f in enumerate(node_frames)]
    raw_dev, _ = archive_np.submap(dev_frames, hist["ids"], hist["clouds"], 0.0)
    assert same_bits(ctx.archive_download(0), rc.lm.voxel_grid(raw_dev, 0.4))
    if same.all():
        rc.assert_voxel_cloud(node.cloud(m.LOOP_HISTORY_DS), ctx.archive_download(0), raw, 0.4)


# ---- e, h. performLoopClosure: lins_loop_step ----------------------------------------------------------------------------------
def test_loop_step_against_perform_loop_closure(m, ctx, ieskf):
    """lins_loop_step on an archive the node holds too: its detection (latest, closest, the two clouds) against
    detectLoopClosure; then the node's performLoopClosure with its stand-in ICP answering WHAT THE DEVICE'S ALIGNMENT
    FOUND — transformation, converged, fitness — so that the glue is what is compared: the accept rule, poseFrom, the
    factor's pair.  And the candidate that is the latest frame itself: the stated departure, both sides."""
    poses = rc.line_poses(40, 0.5, seed=4)
    poses[:, 3:5] = np.random.default_rng(15).uniform(-0.05, 0.05, (40, 2))
    poses[39] = poses[3] + np.array([0.1, 0.0, 0.0, 0.0, 0.0, 0.0], F)  # the same place seen again, stored 0.1 m off
    times = np.r_[np.arange(39) * 1.0, 100.0]
    scans = [rc.small_scan(40 + k, poses[k]) for k in range(40)]
    scans[39] = scans[3]
    ctx.archive_init(2, 64, 1 << 15)
    ctx.pose_graph_init(2, 64, 2)
    node, frames = _archive_on_both(m, ctx, poses, times, scans)
    six = [rc.six(f[3]) for f in frames]
    for k in range(40):
        assert ctx.pose_graph_push(0, six[k - 1] if k else None, six[k]) == k
    node.set_time(100.0)
    centre = node.floats(m.P_CURRENT)[:3]
    r = ctx.loop_step([(0, centre, 100.0)])[0]
    assert r["status"] == 0 and r["outcome"] in (defs.LOOP_CLOSED, defs.LOOP_REJECTED)
    assert node.detect_loop()
    s = node.scalars()
    assert (r["latest_id"], r["closest_id"]) == (s["latestFrameIDLoopCloure"], s["closestHistoryFrameID"]) == (39, 3)
    assert same_bits(ctx.archive_download(0), node.cloud(m.LOOP_LATEST))
    hist = archive_np.history_spec(40, 3)
    raw, _ = archive_np.submap(frames, hist["ids"], hist["clouds"], 0.0)
    rc.assert_voxel_cloud(node.cloud(m.LOOP_HISTORY_DS), ctx.archive_download(1), raw, 0.4)
    icp = r["icp"]
    added, calls = node.perform_loop(icp["transform"].astype(F), icp["converged"], icp["fitness"])
    assert calls == 1 and added == int(r["outcome"] == defs.LOOP_CLOSED) == int(host.loop_accept(icp["converged"], icp["fitness"]))
    print(f"loop_step: outcome {r['outcome']}, converged {icp['converged']}, fitness {icp['fitness']:.4g}, {icp['iterations']} iterations")
    assert r["outcome"] == defs.LOOP_CLOSED  # (the clouds of one place seen twice: the alignment is good)
    ij, z, var = node.factors()
    assert ij[-1].tolist() == [0, 39, 3] and np.array_equal(var[-1], [float(F(icp["fitness"]))] * 6)
    pf, pt = m.Node.last_between()
    ref_from = np.array([pf[3], pf[4], pf[5], pf[0], pf[1], pf[2]])
    print("poseFrom: device", r["pose_from"], "node", ref_from.astype(F))
    assert same_bits(r["pose_from"], ref_from.astype(F))  # the glue is host text in the step: the bits of tests/test_ref_mapnode.py
    # the candidate that is the latest frame itself
    three = rc.line_poses(3, 4.0, seed=6)
    d = rc.Driven(loop=True)
    for k in range(3):
        d.time = float(k)
        assert d.step(rc.small_scan(40 + k, three[k]), rc.six(three[k]))
        f = d.node.frames()[k]
        assert ctx.archive_push(1, *f, time=float(k)) == k
        assert ctx.pose_graph_push(1, rc.six(d.node.frames()[k - 1][3]) if k else None, rc.six(f[3])) == k
    d.node.set_time(40.0)
    assert d.node.detect_loop() and d.node.scalars()["closestHistoryFrameID"] == d.node.scalars()["latestFrameIDLoopCloure"] == 2  # the reference
    assert ctx.keyposes_find_loop_batch([(1, d.node.floats(m.P_CURRENT)[:3], 5.0, 40.0, 30.0)]) == [2]
    own = ctx.loop_step([(1, d.node.floats(m.P_CURRENT)[:3], 40.0)])[0]
    assert own["outcome"] == defs.LOOP_NONE and ctx.pose_graph_count(1) == (3, 0)  # the project


# ---- a, f, j. run(): lins_streams_map_step ------------------------------------------------------------------------------------
def rigid_diff(a, b):
    (Ra, ta), (Rb, tb) = mp.rigid(a), mp.rigid(b)
    return float(np.abs(Ra - Rb).max()), float(np.abs(ta - tb).max())


def test_streams_map_step_against_run(m, pkg, ieskf):
    """The 8 scans and odometry rows of tests/map_step_chain.py, three streams in one device context, against three nodes
    through run().  Before every step the device side is set to the reference's state — the map pose by
    lins_streams_map_set_pose, the rings by pushing the node's key frames — so a last-bit difference of scan-to-map cannot
    compound.  Per step and stream: the gate, the start pose, the six clouds, the key decision, the stored pose and the
    poses after."""
    nodes = [m.Node(loop=True) for _ in range(ch.N)]
    staged = [m.Node(loop=True) for _ in range(ch.N)]
    worst = dict(start_rot=0.0, start_trans=0.0, transform=0.0, key_pose=0.0)
    n_keys, n_skipped, loose = [0] * ch.N, 0, 0
    with ch.context(pkg, ieskf) as c:
        c.streams_init(ch.N)
        c.local_map_init(ch.N, 50, ch.MAX_PTS)
        sm.init(c, ch.N, ch.INTERVAL)
        last_time = [-1.0] * ch.N
        for step in range(ch.STEPS):
            ch.feed(c, step)
            odo = ch.odometry(step)
            c.local_map_init(ch.N, 50, ch.MAX_PTS)  # empty rings, then the node's frames
            sm.init(c, ch.N, ch.INTERVAL)
            scans, frames_before = [], []
            for s in range(ch.N):
                # the scan as the mapping node reads it of the stream's odometry step (corner last, surf last, outlier last)
                scans.append(tuple(c.streams_map_cloud(s, w) for w in range(3)))
                fr = staged[s].frames()
                frames_before.append(fr)
                for f in fr:
                    c.local_map_push(s, *f)
                sm.set_pose(c, s, dict(bef=staged[s].floats(m.T_BEF), aft=staged[s].floats(m.T_AFT), tobe=staged[s].floats(m.T_TOBE),
                                       last=staged[s].floats(m.T_LAST), prev=staged[s].floats(m.P_PREVIOUS)[:3], n_frames=len(fr), last_time=last_time[s]))
                total, time, roll, pitch, has_imu = odo[s]
                for node in (nodes[s], staged[s]):
                    node.feed(*scans[s], total, time)
                    if has_imu:
                        node.imu(time, roll, pitch)
            res = sm.step(c, list(range(ch.N)), ch.odoms(step))
            entry = 0
            for s in range(ch.N):
                total, time, roll, pitch, has_imu = odo[s]
                ran = nodes[s].run()
                assert bool(staged[s].stage(m.GATE)) == ran == (res[s]["status"] != defs.MAP_STEP_SKIPPED), (step, s)
                if not ran:
                    n_skipped += 1
                    continue
                last_time[s] = time
                assert res[s]["status"] == 0
                staged[s].stage(m.ASSOCIATE)
                dr, dt = rigid_diff(res[s]["tobe_start"], staged[s].floats(m.T_TOBE))
                worst["start_rot"], worst["start_trans"] = max(worst["start_rot"], dr), max(worst["start_trans"], dt)
                staged[s].stage(m.EXTRACT), staged[s].stage(m.DOWNSAMPLE)
                got = [sm.download(c, entry, w) for w in range(6)]
                entry += 1
                fr = frames_before[s]
                if fr:
                    loose += rc.check_map_side(m, staged[s], fr, list(range(len(fr))), got, (step, s))
                loose += rc.check_scan_side(m, staged[s], scans[s], got, (step, s))
                for k in (m.SCAN2MAP, m.SAVE):
                    staged[s].stage(k)
                saved = staged[s].scalars()["key_frames"] - len(fr)
                assert res[s]["key_frame"] == saved, (step, s)
                worst["transform"] = max(worst["transform"], float(np.abs(res[s]["transform"] - nodes[s].floats(m.T_AFT)).max()))
                if saved:
                    n_keys[s] += 1
                    p6 = staged[s].key_poses()[1][-1]
                    worst["key_pose"] = max(worst["key_pose"], float(np.abs(rc.key_pose(res[s]["key_pose"]) - p6[[0, 1, 2, 4, 5, 6]]).max()))
                    assert res[s]["ring_age"] == 0
                for k in (m.CORRECT, m.PUBLISH, m.CLEAR):
                    staged[s].stage(k)
                assert nodes[s].same_state(staged[s]) == 0, (step, s)
                st = sm.get_pose(c, s)
                assert st["n_frames"] == len(fr) + saved and st["last_time"] == time
                for f, what in (("bef", m.T_BEF), ("aft", m.T_AFT), ("tobe", m.T_TOBE), ("last", m.T_LAST)):
                    worst["transform"] = max(worst["transform"], float(np.abs(st[f] - staged[s].floats(what)).max()))
                assert same_bits(st["bef"], total if (fr and res[s]["iters"] > 0) else staged[s].floats(m.T_BEF))
    print("streams_map.step against run():", {k: float(f"{v:.3g}") for k, v in worst.items()}, f"key frames {n_keys}, skipped {n_skipped}, "
          f"{loose} voxels of >= 3 points differ in the last bits; bars: start {4 * mpc.E_HOST_ROT:.3g} / {4 * mpc.E_HOST_TRANS:.3g} m, transform {ROUNDS_BAR:.3g}")
    assert worst["start_rot"] <= 4 * mpc.E_HOST_ROT and worst["start_trans"] <= 4 * mpc.E_HOST_TRANS
    assert worst["transform"] <= ROUNDS_BAR and worst["key_pose"] <= ROUNDS_BAR
    assert all(k >= 3 for k in n_keys) and n_skipped == 1
