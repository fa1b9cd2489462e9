"""The pose graph on the device (include/lins_map.h lins_pose_graph_*) against the CPU restatement
(host/pose_graph.cpp, itself pinned to the numpy checker by tests/test_pose_graph_host.py): the solve case by case,
batch independence bit for bit, the write-back into the archive, the local map's ring and a stream's map pose, the loop
thread end to end (find_loop -> assemble -> ICP -> pose_from -> add_loop -> solve -> apply), and the errors.

DEVICE_BAR: host and device run one text (csrc/pose_graph.h) and differ only where libm does (sin, cos, atan2 in Exp / Log
and in the six-float conversions).  Measured on an MI355X over the cases below, default parameters: the largest difference
of an f64 pose entry is 6.4e-14 (translation, m; rotation entries 5.7e-15); the bar is 4 x that, for last-place differences
carried through the solve.  It stays far below the host-against-checker bar (4.5e-8, tests/test_pose_graph_host.py)."""
import importlib

import numpy as np
import pytest

import loop_icp_cases as licp
import pose_graph_cases as cases
import pose_graph_np as pnp

pytestmark = pytest.mark.gpu
host = importlib.import_module("lins---lidar-inertial-slam_amd.host")
sm = importlib.import_module("lins---lidar-inertial-slam_amd.streams_map")

DEVICE_BAR = 4 * 6.4e-14
HOST_CHECKER_BAR = 8 * 5.59e-9
MAX_LOOPS = 4


@pytest.fixture
def ctx(pkg, ieskf):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    yield c
    c.close()


class DevGraph:
    """push / add_loop of one slot, as pose_graph_cases.fill wants them"""

    def __init__(self, ctx, slot):
        self.ctx, self.slot = ctx, slot

    def push(self, last6, aft6):
        return self.ctx.pose_graph_push(self.slot, last6, aft6)

    def add_loop(self, b, a, pf, var):
        return self.ctx.pose_graph_add_loop(self.slot, b, a, pf, var)


def host_solved(c):
    g = host.PoseGraph(len(c["aft"]), MAX_LOOPS)
    cases.fill(g, c)
    return g, g.solve()


def test_device_against_host_case_by_case(ctx):
    worst = 0.0
    for c in cases.host_cases() + cases.gpu_extra_cases():
        n = len(c["aft"])
        ctx.pose_graph_init(1, n, MAX_LOOPS)
        cases.fill(DevGraph(ctx, 0), c)
        assert ctx.pose_graph_count(0) == (n, len(c["loops"]))
        got = ctx.pose_graph_solve([0])[0]
        g, want = host_solved(c)
        T, Tw = ctx.debug_pose_graph_poses_f64(0), g.poses_f64()
        d = np.abs(T - Tw)
        print("%-26s N %3d L %d  iterations %2d / %2d  reason %d / %d  |dR| %.2e |dt| %.2e  cost %.6g -> %.6g" % (
            c["name"], n, len(c["loops"]), got["iterations"], want["iterations"], got["reason"], want["reason"], d[:, :9].max(), d[:, 9:].max(),
            got["cost_before"], got["cost_after"]))
        assert (got["iterations"], got["reason"], got["status"]) == (want["iterations"], want["reason"], 0), c["name"]
        assert got["iterations"] > 0 and got["cost_after"] < got["cost_before"]
        assert abs(got["cost_after"] - want["cost_after"]) <= 1e-9 * want["cost_after"]
        assert d.max() <= DEVICE_BAR, (c["name"], d.max())
        worst = max(worst, d.max())
        # the prior frame keeps its bits; an f32 field handed back is the restatement's, or its neighbour where the f64 value sits on a rounding tie
        P, Pw = ctx.pose_graph_poses(0), g.poses()
        assert np.array_equal(P[0].view(np.int32), pnp.key_pose_of6(c["aft"][0]).view(np.int32))
        assert np.array_equal(T[0], host.pose_from6(c["aft"][0]))
        assert np.all(np.abs(P.astype(np.float64) - Pw) <= np.spacing(np.abs(Pw))), c["name"]  # field by field: one ulp of its own size
    print("largest device-host difference of a pose entry: %.3e (bar %.3e)" % (worst, DEVICE_BAR))
    assert DEVICE_BAR < HOST_CHECKER_BAR


@pytest.mark.parametrize("n", [1, 2, 70])
def test_loop_free_graph_returns_its_bits(ctx, n):
    aft = cases.trajectory(60 + n, n)
    ctx.pose_graph_init(2, n, 1)
    cases.fill(DevGraph(ctx, 1), dict(aft=aft, loops=[]))
    r = ctx.pose_graph_solve([1, 0])
    assert all((x["iterations"], x["reason"], x["status"]) == (0, 0, 0) for x in r)
    want = np.array([pnp.key_pose_of6(p) for p in aft])
    assert np.array_equal(ctx.pose_graph_poses(1).view(np.int32), want.view(np.int32))
    assert ctx.pose_graph_stats()[1] == 0


def batch_cases():
    h, e = cases.host_cases(), cases.gpu_extra_cases()
    loop_free = dict(name="loop_free", aft=cases.trajectory(77, 50), loops=[])
    return [h[0], h[2], e[5], e[-1], loop_free]  # N = 3, 40, 65, 72, 50; L = 1, 2, 1, 4, 0


def run_groups(ctx, groups):
    """fresh graphs of batch_cases() in slots 0 .. 4, solved group by group -> per slot (result, f64 poses, f32 poses)"""
    cs = batch_cases()
    ctx.pose_graph_init(len(cs), 80, MAX_LOOPS)
    for s, c in enumerate(cs):
        cases.fill(DevGraph(ctx, s), c)
    res = {}
    for grp in groups:
        for s, r in zip(grp, ctx.pose_graph_solve(grp)):
            res[s] = r
    return [(tuple(sorted(res[s].items())), ctx.debug_pose_graph_poses_f64(s).tobytes(), ctx.pose_graph_poses(s).tobytes()) for s in range(len(cs))]


def test_a_problems_bits_do_not_depend_on_its_batch(ctx):
    together = run_groups(ctx, [[0, 1, 2, 3, 4]])
    assert run_groups(ctx, [[0], [1], [2], [3], [4]]) == together
    assert run_groups(ctx, [[4, 3, 2, 1, 0]]) == together
    # ... nor on what the context solved before: other graphs in between, then the same call
    assert run_groups(ctx, [[3], [1, 4], [0, 2]]) == together
    # the slot without loops inside a batch that iterates is untouched
    cs = batch_cases()
    want = np.array([pnp.key_pose_of6(p) for p in cs[4]["aft"]])
    assert together[4][2] == want.tobytes() and dict(together[4][0])["iterations"] == 0
    assert all(dict(together[s][0])["iterations"] > 0 for s in range(4))


def test_a_solve_does_not_depend_on_what_the_allocation_held_before(ctx):
    """one allocation throughout: the graphs of batch_cases() in slots 0 .. 4 and AGAIN in slots 5 .. 9; the first copies
    are solved in one call, then — the scratch, the states and the "still running" words used — the second copies in
    other groupings; slot s + 5 has the bits of slot s.  A fresh context solving the same call gives them too."""
    cs = batch_cases()

    def fill(c):
        c.pose_graph_init(2 * len(cs), 80, MAX_LOOPS)
        for s in range(2 * len(cs)):
            cases.fill(DevGraph(c, s), cs[s % len(cs)])

    def state(c, s, r):
        return tuple(sorted(r.items())), c.debug_pose_graph_poses_f64(s).tobytes(), c.pose_graph_poses(s).tobytes()

    fill(ctx)
    first = [state(ctx, s, r) for s, r in zip(range(5), ctx.pose_graph_solve([0, 1, 2, 3, 4]))]
    second = {}
    for grp in ([8], [6, 9], [7, 5]):
        for s, r in zip(grp, ctx.pose_graph_solve(grp)):
            second[s] = state(ctx, s, r)
    assert [second[s + 5] for s in range(5)] == first
    # the same call repeated on the used allocation: the solved graphs stop in their first trial where they stand
    again = ctx.pose_graph_solve([0, 1, 2, 3, 4])
    assert all(1 <= r["iterations"] <= 2 and abs(r["cost_after"] - dict(first[s][0])["cost_after"]) <= 1e-11 * r["cost_after"]
               for s, r in enumerate(again) if s < 4)
    assert again[4]["iterations"] == 0


def tiny_frames(n):
    """n key frames of tiny clouds with the poses of a short arc"""
    poses = licp.trajectory(12, seed=5)[:n]
    return [licp.room_scan(900 + i, poses[i], n_corner=40, n_surf=300, n_outlier=30) + (poses[i],) for i in range(n)]


def six_of_key(p):
    """PointTypePose (x, y, z, roll, pitch, yaw) -> six floats (t[0..5] of transformAftMapped)"""
    return np.array([p[3], p[4], p[5], p[0], p[1], p[2]], np.float32)


def test_apply_writes_back_what_the_set_pose_calls_would(pkg, ieskf, ctx):
    frames = tiny_frames(3)
    scan = licp.room_scan(950, frames[2][3], n_corner=40, n_surf=300, n_outlier=30)
    spec = [dict(slot=0, ids=[0, 1, 2], clouds=7, leaf=0.4, flags=0)]
    other = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    try:
        for c in (ctx, other):
            c.archive_init(1, 4, 4096)
            c.local_map_init(1, 2, 1024)  # window 2 < 3 frames: the ring holds frames 1 and 2
            for i, f in enumerate(frames):
                c.archive_push(0, *f, time=float(i))
                c.local_map_push(0, *f)
        ctx.streams_init(1)
        sm.init(ctx, 1)
        ctx.pose_graph_init(1, 8, 2)
        for i, f in enumerate(frames):
            assert ctx.pose_graph_push(0, six_of_key(frames[i - 1][3]) if i else None, six_of_key(f[3])) == i
        moved = cases.corrected(six_of_key(frames[2][3]), 0.3, 2.0, 5)
        ctx.pose_graph_add_loop(0, 2, 0, moved, 1e-6)
        r = ctx.pose_graph_solve([0])[0]
        assert r["iterations"] > 0
        before = sm.get_pose(ctx, 0)
        ctx.pose_graph_apply(0, 0)
        poses = ctx.pose_graph_poses(0)
        assert np.abs(poses[2] - frames[2][3]).max() > 0.05  # the solve moved the newest frame
        other.archive_set_poses(0, 0, poses)
        other.local_map_set_pose(0, 0, poses[2])
        other.local_map_set_pose(0, 1, poses[1])
        clouds = []
        for c in (ctx, other):
            info = c.archive_assemble(spec)
            sizes = c.local_map_build([0], [scan])
            clouds.append((info[0]["n"], c.archive_download(0).tobytes(), sizes[0]["n"], [c.local_map_download(0, w).tobytes() for w in range(6)]))
        assert clouds[0][0] > 0 and clouds[0][2][0] > 0 and clouds[0] == clouds[1]
        after = sm.get_pose(ctx, 0)
        newest = six_of_key(poses[2])
        for k in ("aft", "last", "tobe"):
            assert np.array_equal(np.asarray(after[k], np.float32).view(np.int32), newest.view(np.int32)), k
        assert np.array_equal(np.asarray(after["bef"]), np.asarray(before["bef"])) and after["n_frames"] == before["n_frames"]
    finally:
        other.close()


def test_loop_thread_end_to_end(ctx):
    """12 key frames along a closed loop, the latest stored with a drifted pose: detect, assemble, align, add, solve, apply"""
    frames, _, wrong, _ = licp.archive_case()
    latest = len(frames) - 1
    ctx.archive_init(1, 16, sum(len(f[0]) + len(f[1]) + len(f[2]) for f in frames))
    ctx.pose_graph_init(1, 16, 2)
    for i, f in enumerate(frames):
        assert ctx.archive_push(0, *f, time=float(i)) == ctx.pose_graph_push(0, six_of_key(frames[i - 1][3]) if i else None, six_of_key(f[3])) == i
    closest = ctx.archive_find_loop(0, wrong[:3], 7.0, float(latest), 5.0)
    assert 0 <= closest <= 5
    ids = list(range(max(0, closest - 4), min(latest, closest + 4) + 1))
    ctx.archive_assemble([dict(slot=0, ids=[latest], clouds=3, leaf=0.0, flags=1), dict(slot=0, ids=ids, clouds=3, leaf=0.4, flags=0)])
    icp = ctx.loop_icp([(0, 1)])[0]
    assert icp["converged"] == 1 and icp["fitness"] <= 0.3
    pose_from = host.loop_pose_from(icp["transform"], wrong)
    ctx.pose_graph_add_loop(0, latest, closest, pose_from, 1e-6)
    r = ctx.pose_graph_solve([0])[0]
    assert r["iterations"] > 0 and r["cost_after"] < 0.5 * r["cost_before"]
    ctx.pose_graph_apply(0)
    # the checker's prediction of the same graph
    c = dict(aft=np.array([six_of_key(f[3]) for f in frames]), loops=[(latest, closest, pose_from, 1e-6)])
    G = cases.graph_of(c)
    F = pnp.build(G)
    Tn, _ = pnp.solve(F, pnp.initial(G))
    T = ctx.debug_pose_graph_poses_f64(0)
    assert np.abs(T - pnp.flat(Tn)).max() <= HOST_CHECKER_BAR
    # the latest frame moves towards pose_from — as far as the checker says it does
    goal = pnp.pose_from_lidar(pose_from)[1]
    t0, t1, tn = pnp.pose_from6(c["aft"][latest])[1], T[latest, 9:], Tn[latest][1]
    print("latest frame: %.3f m from pose_from before, %.3f m after (checker %.3f m)" % (
        np.linalg.norm(t0 - goal), np.linalg.norm(t1 - goal), np.linalg.norm(tn - goal)))
    assert np.linalg.norm(t1 - goal) < 0.5 * np.linalg.norm(t0 - goal)
    assert abs(np.linalg.norm(t1 - goal) - np.linalg.norm(tn - goal)) <= HOST_CHECKER_BAR
    # the archive holds the solved poses: its assembly of the latest frame moved with it
    want = ctx.pose_graph_poses(0)
    before = ctx.archive_download(0)
    ctx.archive_assemble([dict(slot=0, ids=[latest], clouds=3, leaf=0.0, flags=1)])
    shift = np.abs(ctx.archive_download(0)[:, :3] - before[:, :3]).max()
    assert shift > 0.25 * np.abs(want[latest, :3] - wrong[:3]).max() > 0.0


def test_errors_leave_the_context_usable(ctx, ieskf):
    c = cases.host_cases()[2]
    with pytest.raises(ieskf.LinsError, match="-6"):  # LINS_E_STATE before lins_pose_graph_init
        ctx.pose_graph_push(0, None, c["aft"][0])
    with pytest.raises(ieskf.LinsError, match="-6"):
        ctx.pose_graph_solve([0])
    ctx.pose_graph_init(1, len(c["aft"]), 3)
    cases.fill(DevGraph(ctx, 0), c)  # two loops
    pf = cases.corrected(c["aft"][10], 0.1, 0.5, 7)
    ctx.pose_graph_add_loop(0, 10, 2, pf, 1e-6)
    with pytest.raises(ieskf.LinsError, match="-3"):  # LINS_E_CAPACITY at max_loops + 1
        ctx.pose_graph_add_loop(0, 11, 2, pf, 1e-6)
    with pytest.raises(ieskf.LinsError, match="-3"):
        ctx.pose_graph_push(0, c["aft"][-1], c["aft"][-1])
    for bad in ((5, 5), (40, 0), (0, -1)):
        with pytest.raises(ieskf.LinsError, match="-1"):
            ctx.pose_graph_add_loop(0, bad[0], bad[1], pf, 1e-6)
    with pytest.raises(ieskf.LinsError, match="-4"):
        ctx.pose_graph_add_loop(0, 10, 2, pf, 0.0)
    with pytest.raises(ieskf.LinsError, match="-1"):
        ctx.pose_graph_solve([0, 0])
    with pytest.raises(ieskf.LinsError, match="-1"):
        ctx.pose_graph_solve([1])
    assert ctx.pose_graph_count(0) == (len(c["aft"]), 3)
    g = host.PoseGraph(len(c["aft"]), 3)
    cases.fill(g, c)
    g.add_loop(10, 2, pf, 1e-6)
    want, got = g.solve(), ctx.pose_graph_solve([0])[0]
    assert (got["iterations"], got["reason"]) == (want["iterations"], want["reason"])
    assert np.abs(ctx.debug_pose_graph_poses_f64(0) - g.poses_f64()).max() <= DEVICE_BAR
