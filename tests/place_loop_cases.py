"""The end-to-end case of place recognition (tests/test_place_loop_inputs.py on the CPU, tests/test_gpu_place_loop.py on
the device): a dozen small room frames, the last a revisit of frame 1 whose STORED pose is wrong by more than the loop
search radius and by several sectors of yaw, so that lins_archive_find_loop finds nothing and only the scans can.

The room of tests/local_map_synth.py is a rectangle: it looks the same after a half turn about its centre, and frame 7
of the trajectory stands where that half turn takes frame 1.  Without more, frame 7 wins (d = 0.071 against 0.081).
Three wall pieces that no half turn maps onto the room or onto each other make the place unambiguous; with them frame 1
wins at d = 0.130 against 0.227 for frame 7 and >= 0.44 for every other frame (tests/test_place_loop_inputs.py asserts
the margin)."""
import functools
import importlib

import numpy as np

import local_map_synth as lms
import loop_icp_cases as licp

PKG = "lins---lidar-inertial-slam_amd"
host = importlib.import_module(PKG + ".host")
F = np.float32
N, REVISITED, EXTRA, SEED = 12, 1, 300, 3
RADIUS, GAP, H, NOW = 5.0, 3.0, 4, 11.0  # the loop search radius of the reference; one frame a second
UP = 2                                   # the fixtures of local_map_synth are z-up
# The loop factor's variance, as tests/test_gpu_pose_graph.py::test_loop_thread_end_to_end passes it.  With the
# reference's own (the ICP's fitness, ~0.09, against 1e-6 per odometry factor) the graph leaves the last frame where
# odometry put it, to 0.01 %, in this case and in the identity-start archive case alike: 7.146 m and 0.373 m.
LOOP_VARIANCE = 1e-6
DS = 2 * np.pi / 60
TRUE_OFFSET = np.array([0.3, -0.2, 0.0, 0.0, 0.0, 0.55])   # the revisit: a third of a metre off frame 1, turned 5.25 sectors
STORED_ERROR = np.array([6.5, 3.0, 0.1, 0.02, -0.02, 0.45])  # 7.2 m and 4.3 sectors: what odometry drift left
# (origin, u, v) of the three wall pieces
PIECES = (((3.0, 7.0, -1.5), (0.0, -5.0, 0.0), (0.0, 0.0, 6.0)), ((-12.0, -6.0, -1.5), (8.0, 0.0, 0.0), (0.0, 0.0, 2.5)),
          ((10.0, -3.0, -1.5), (3.0, 3.0, 0.0), (0.0, 0.0, 6.0)))


def scan(seed, pose):
    """local_map_synth.room_scan with EXTRA surf points on the wall pieces"""
    corner, surf, outlier = lms.room_scan(seed, pose, **licp.SMALL)
    rng = np.random.default_rng(seed + 77)
    k = rng.integers(0, len(PIECES), EXTRA)
    a, b = rng.uniform(0, 1, EXTRA), rng.uniform(0, 1, EXTRA)
    org, u, v = (np.array([p[i] for p in PIECES], np.float64)[k] for i in range(3))
    pm = org + a[:, None] * u + b[:, None] * v + rng.normal(0, 0.01, (EXTRA, 3))
    extra = np.concatenate([lms.to_sensor(pm, pose), rng.uniform(0, 100, (EXTRA, 1))], 1).astype(F)
    return corner, np.concatenate([surf, extra]), outlier


@functools.lru_cache(maxsize=None)
def case():
    """(frames [(corner, surf, outlier, stored pose)], true pose of the last frame, its stored pose)"""
    poses = lms.trajectory(N, seed=SEED)
    true = (poses[REVISITED].astype(np.float64) + TRUE_OFFSET).astype(F)
    wrong = (true.astype(np.float64) + STORED_ERROR).astype(F)
    seen = [poses[i] for i in range(N - 1)] + [true]
    stored = [poses[i] for i in range(N - 1)] + [wrong]
    return [scan(7000 + i, seen[i]) + (stored[i],) for i in range(N)], true, wrong


def six_of_key(p):
    return np.array([p[3], p[4], p[5], p[0], p[1], p[2]], F)


def window(closest, latest):
    return list(range(max(0, closest - H), min(latest, closest + H) + 1))


@functools.lru_cache(maxsize=None)
def host_chain():
    """the chain on the CPU restatement -> dict(search, T0, icp, pose_from, final (the last frame's pose after solve),
    row (every candidate's smallest distance))"""
    frames, true, wrong = case()
    prm = host.place_params(up_axis=UP)
    D = [host.place_descriptor(*f[:3], params=prm) for f in frames]
    times = np.arange(N, dtype=np.float64)
    r = dict(search=host.place_search(D[-1], D, times, NOW, GAP, skip_id=N - 1))
    r["row"] = [float(host.place_distance(D[-1], D[i]).min()) for i in range(N - 1)]
    c, k = r["search"]["id"], r["search"]["shift"]
    r["T0"] = host.place_guess(wrong, frames[c][3], k, UP)
    src = host.submap(frames, [N - 1], 3, 0.0, 1)[0]
    tgt = host.submap(frames, window(c, N - 1), 3, 0.4, 0)[0]
    r["icp"] = host.loop_icp_from(src, tgt, r["T0"])
    r["pose_from"] = host.loop_pose_from(r["icp"]["transform"], wrong)
    r["final"] = solved(frames, [(N - 1, c, r["pose_from"], LOOP_VARIANCE)])[N - 1]
    return r


def solved(frames, loops):
    g = host.PoseGraph(16, 2)
    for i, f in enumerate(frames):
        assert g.push(six_of_key(frames[i - 1][3]) if i else None, six_of_key(f[3])) == i
    for lp in loops:
        assert g.add_loop(*lp) == 0
    g.solve()
    out = g.poses().copy()
    g.close()
    return out


@functools.lru_cache(maxsize=None)
def bound():
    """(error the identity-start archive case of loop_icp_cases leaves in its last frame's position after the same chain
    on the CPU restatement, the bound for this case: twice that, for the larger start error)"""
    frames, specs, wrong, true = licp.archive_case()
    closest = host.find_loop(np.array([f[3] for f in frames]), np.arange(12.0), wrong[:3], 7.0, 11.0, 5.0)
    src = host.submap(frames, [11], 3, 0.0, 1)[0]
    tgt = host.submap(frames, window(closest, 11), 3, 0.4, 0)[0]
    icp = host.loop_icp(src, tgt)
    final = solved(frames, [(11, closest, host.loop_pose_from(icp["transform"], wrong), LOOP_VARIANCE)])[11]
    err = float(np.linalg.norm(final[:3].astype(np.float64) - true[:3]))
    return err, 2.0 * err
