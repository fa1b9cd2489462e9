"""Seeded graph cases of the pose-graph tests (tests/test_pose_graph_host.py, tests/test_gpu_pose_graph.py).

A case is a dict: name, aft (N, 6) f32 — the six floats (pitch, yaw, roll, y, z, x) frame k is pushed with; last[k] =
aft[k - 1], as the mapping node leaves transformLast — and loops: (latest, closest, pose_from, variance), pose_from the
(x, y, z, roll, pitch, yaw) lins_host_loop_pose_from would hand over: where the alignment says the latest frame is.  The
trajectories are arcs of 15-30 m radius with a few centimetres of wobble; every coordinate stays below 100 m."""
import numpy as np

import pose_graph_np as pnp

PREFIX_BLOCK = 32  # csrc/pose_graph.h kPrefixBlock: increments composed left to right in one block


def trajectory(seed, n, radius=20.0, turn=2 * np.pi, centre=(30.0, -20.0)):
    """n six-float poses along an arc: heading about the mapping node's vertical axis (p[1]), small pitch / roll"""
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, 1.0, max(n, 2))[:n]
    yaw = turn * s + 0.3
    p = np.zeros((n, 6))
    p[:, 1] = (yaw + np.pi) % (2 * np.pi) - np.pi
    p[:, 0] = 0.03 * np.sin(5 * s) + rng.normal(0, 0.004, n)
    p[:, 2] = 0.02 * np.cos(3 * s) + rng.normal(0, 0.004, n)
    # t = (p[5], p[3], p[4]) in the axes GTSAM sees: the arc lies in the (x, y) plane there, z wobbles
    p[:, 5] = centre[0] + radius * np.cos(yaw) + rng.normal(0, 0.02, n)
    p[:, 3] = centre[1] + radius * np.sin(yaw) + rng.normal(0, 0.02, n)
    p[:, 4] = 0.5 * s + rng.normal(0, 0.01, n)
    return p.astype(np.float32)


def corrected(aft_row, dtrans, drot_deg, seed):
    """pose_from for a loop: the pushed pose of the latest frame moved by dtrans metres and drot_deg degrees"""
    rng = np.random.default_rng(seed)
    R, t = pnp.pose_from6(aft_row)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    dr = rng.normal(size=3)
    dr /= np.linalg.norm(dr)
    Rn = pnp.so3_exp(np.deg2rad(drot_deg) * ax) @ R
    return pnp.lidar_of_pose((Rn, t + dtrans * dr))


def case(name, seed, n, loops, **kw):
    """loops: (latest, closest, metres, degrees, variance)"""
    aft = trajectory(seed, n, **kw)
    return dict(name=name, aft=aft,
                loops=[(b, a, corrected(aft[b], m, deg, seed * 100 + i), var) for i, (b, a, m, deg, var) in enumerate(loops)])


def last_of(aft):
    last = np.zeros_like(aft)
    last[1:] = aft[:-1]
    return last


def host_cases():
    """the cases of the issue's list (test 4)"""
    return [
        case("n3_loop_2_0", 1, 3, [(2, 0, 0.05, 0.5, 1e-6)], turn=0.3),
        case("n40_whole_chain_1m_5deg", 2, 40, [(39, 0, 1.0, 5.0, 1e-6)]),
        case("nested", 3, 40, [(38, 2, 0.4, 2.0, 1e-6), (30, 10, 0.2, 1.0, 1e-6)]),
        case("overlapping", 4, 40, [(25, 3, 0.3, 1.5, 1e-6), (37, 15, 0.3, 1.5, 1e-6)]),
        case("shared_endpoint", 5, 40, [(39, 5, 0.3, 2.0, 1e-6), (39, 20, 0.2, 1.0, 1e-6)]),
        case("strong_1e-6", 6, 40, [(39, 1, 0.5, 3.0, 1e-6)]),
        case("weak_0.3", 6, 40, [(39, 1, 0.5, 3.0, 0.3)]),
    ]


def gpu_extra_cases():
    """what the device's shapes add: N = 2, N around the prefix block, loops on block edges, L = 1 .. 4 (max_loops = 4)"""
    B = PREFIX_BLOCK
    out = [case("n2", 11, 2, [(1, 0, 0.05, 0.5, 1e-6)], turn=0.1)]
    for n in (B - 1, B, B + 1, B + 2, 2 * B + 1, 2 * B + 2):
        out.append(case("n%d" % n, 20 + n, n, [(n - 1, 0, 0.3, 2.0, 1e-6)]))
    # increments B + 1 .. 2 B are exactly block 1: the loop (2 B, B) spans that block and nothing else
    out.append(case("block_edge", 12, 2 * B + 8, [(2 * B, B, 0.2, 1.0, 1e-6)]))
    out.append(case("four_loops", 13, 2 * B + 8, [(2 * B + 7, 0, 0.5, 2.0, 1e-6), (50, 10, 0.2, 1.0, 1e-4), (40, 33, 0.1, 0.5, 1e-6),
                                                  (5, 60, 0.2, 1.0, 0.01)]))
    return out


def graph_of(c, estimate6=None):
    """the checker's graph of a case; the loops' measurements are formed from estimate6 (default: the poses as pushed)"""
    est = c["aft"] if estimate6 is None else estimate6
    return dict(aft=c["aft"], last=last_of(c["aft"]),
                loops=[(b, a, pnp.loop_measurement(pf, est[a]), var) for b, a, pf, var in c["loops"]])


def fill(g, c):
    """push a case into a graph object with push(last6, aft6) / add_loop(latest, closest, pose_from, fitness)"""
    last = last_of(c["aft"])
    for k in range(len(c["aft"])):
        g.push(last[k] if k else None, c["aft"][k])
    for b, a, pf, var in c["loops"]:
        g.add_loop(b, a, pf, var)
