"""Shared set-up of the loop-step tests (not a test): the 12-frame archive case of loop_icp_cases pushed to the archive,
the local map's ring and the pose graph of a slot, the parameters the tests run with, and the EXPLICIT chain a caller had
to write before lins_loop_step (INTEGRATION.md §2e''''): lins_archive_find_loop -> lins_archive_assemble ->
lins_loop_icp_batch -> lins_pose_graph_poses + lins_host_loop_pose_from -> lins_pose_graph_add_loop ->
lins_pose_graph_solve -> lins_pose_graph_apply, with the decisions of csrc/host/loop_step.h between them.
lins_loop_step must give the same bits.  tests/test_loop_step_inputs.py asserts on the CPU what the GPU tests rest on."""
import importlib

import numpy as np

import loop_icp_cases as licp

PKG = "lins---lidar-inertial-slam_amd"
defs = importlib.import_module(PKG + "._ctypes_defs")
host = importlib.import_module(PKG + ".host")

F = np.float32
# the archive case is 12 frames, one a second: a gap of 5 s leaves frames 0 .. 5 as candidates, the window is +-4 frames
# (as tests/test_gpu_pose_graph.py test_loop_thread_end_to_end runs the chain)
RADIUS, GAP, H, NOW = 7.0, 5.0, 4, 11.0
MAX_FRAMES, MAX_LOOPS, WINDOW, MAX_PTS = 16, 2, 4, 1024


def frames():
    return licp.archive_case()[0]


def centre():
    return licp.archive_case()[2][:3]  # the latest frame's (drifted) position: currentRobotPosPoint


def times(kind):
    """"loop": one frame a second, so frames 0 .. 5 lie beyond the gap at NOW; "inside": every frame within the gap"""
    return [float(i) for i in range(12)] if kind == "loop" else [NOW - 0.25 * (11 - i) for i in range(12)]


def params(lib, **kw):
    d = dict(search_radius=RADIUS, min_gap_s=GAP, search_num=H)
    d.update(kw)
    return defs.loop_step_params(lib, **d)


def six_of_key(p):
    """PointTypePose (x, y, z, roll, pitch, yaw) -> six floats (t[0..5] of transformAftMapped)"""
    return np.array([p[3], p[4], p[5], p[0], p[1], p[2]], F)


def init(c, n_slots, max_loops=MAX_LOOPS):
    fr = frames()
    c.archive_init(n_slots, MAX_FRAMES, n_slots * sum(len(f[0]) + len(f[1]) + len(f[2]) for f in fr))
    c.local_map_init(n_slots, WINDOW, MAX_PTS)
    c.pose_graph_init(n_slots, MAX_FRAMES, max_loops)


def push(c, slot, kind):
    """the archive case into the archive, the ring and the graph of `slot`"""
    fr, t = frames(), times(kind)
    for i, f in enumerate(fr):
        assert c.archive_push(slot, *f, time=t[i]) == c.pose_graph_push(slot, six_of_key(fr[i - 1][3]) if i else None, six_of_key(f[3])) == i
        c.local_map_push(slot, *f)


def info_zero():
    return dict(n=0, frames=0, points_in=0, box_min=[0, 0, 0], box_dim=[0, 0, 0], status=0)


def result_zero():
    return dict(outcome=defs.LOOP_NONE, status=0, latest_id=-1, closest_id=-1, latest=info_zero(), history=info_zero(),
                icp=defs.LoopIcpResultC().as_dict(), pose_from=np.zeros(6, F), graph=defs.PoseGraphResultC().as_dict())


def explicit_chain(c, slot, centre_, now, prm, stream=-1, max_loops=MAX_LOOPS, last_pair=(-1, -1)):
    """the seven calls for one slot on context c -> the result dict lins_loop_step would give.  last_pair: the pair of the
    slot's most recent loop factor, which a caller of the chain has to remember itself."""
    r = result_zero()
    latest = r["latest_id"] = c.archive_count(slot) - 1
    if latest < 0:
        return r
    closest = r["closest_id"] = c.archive_find_loop(slot, centre_, prm.search_radius, now, prm.min_gap_s)
    what = host.loop_candidate(latest, closest, *last_pair)
    if what != -1:
        r["outcome"] = what
        return r
    if c.pose_graph_count(slot)[1] >= max_loops:
        r["status"] = -3  # LINS_E_CAPACITY
        return r
    ids = host.loop_window(latest, closest, prm.search_num)
    r["latest"], r["history"] = c.archive_assemble([dict(slot=slot, ids=[latest], clouds=3, leaf=0.0, flags=1),
                                                    dict(slot=slot, ids=ids, clouds=3, leaf=prm.history_leaf, flags=0)])
    if r["latest"]["status"] or r["history"]["status"]:
        r["status"] = r["latest"]["status"] or r["history"]["status"]
        return r
    icp = r["icp"] = c.loop_icp([(0, 1)], prm.icp)[0]
    r["outcome"] = defs.LOOP_REJECTED
    if not (host.loop_accept(icp["converged"], icp["fitness"], prm.max_fitness) and host.loop_variance(icp["fitness"])[0]):
        return r
    wrong = c.pose_graph_poses(slot, latest, 1)[0]
    r["pose_from"] = host.loop_pose_from(icp["transform"], wrong)
    c.pose_graph_add_loop(slot, latest, closest, r["pose_from"], icp["fitness"])
    r["graph"] = c.pose_graph_solve([slot], prm.graph)[0]
    c.pose_graph_apply(slot, stream)
    r["outcome"] = defs.LOOP_CLOSED
    return r


def frozen(x):
    """a result (or any nest of dicts / lists / arrays / numbers) as something == compares bit for bit"""
    if isinstance(x, dict):
        return tuple((k, frozen(x[k])) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, float):
        return np.float64(x).tobytes()
    return x


def state_of(c, slot, scan):
    """what a step leaves behind for a slot, as bytes: the graph (counts, f64 and f32 poses, the first loop's Z), an
    assembly of the latest frame from the archive, and the six clouds of a local-map build from the ring"""
    n, loops = c.pose_graph_count(slot)
    c.archive_assemble([dict(slot=slot, ids=[n - 1], clouds=3, leaf=0.0, flags=1)])
    latest = c.archive_download(0)
    sizes = c.local_map_build([slot], [scan])
    clouds = [c.local_map_download(0, w).tobytes() for w in range(6)]
    z = [c.debug_pose_graph_loop_z(slot, l).tobytes() for l in range(loops)]
    return (n, loops, c.debug_pose_graph_poses_f64(slot).tobytes(), c.pose_graph_poses(slot).tobytes(), z, len(latest), latest.tobytes(),
            frozen(sizes[0]), clouds)


def build_scan():
    """a scan for state_of's local-map build: a room scan at the latest frame's true pose"""
    return licp.room_scan(950, licp.archive_case()[3], n_corner=40, n_surf=300, n_outlier=30)
