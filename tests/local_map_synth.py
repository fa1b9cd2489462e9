"""Synthetic room scans for the local-map tests: sensor-frame corner / surf / outlier clouds seen from a key pose
(x, y, z, roll, pitch, yaw), with the pose convention of transformPointCloud (LM:627-650) — p_map = R p + t,
R = Ry(pitch) Rx(roll) Rz(yaw)."""
import numpy as np

from map_synth import rot

L, W, H = 30.0, 20.0, 6.0
O = np.array([-L / 2, -W / 2, -1.5])
EX, EY, EZ = np.array([L, 0, 0.0]), np.array([0, W, 0.0]), np.array([0, 0, H])


def _planes(rng, n):
    """n points on the floor and the four walls"""
    parts = [(O, EX, EY), (O, EX, EZ), (O + EY, EX, EZ), (O, EY, EZ), (O + EX, EY, EZ)]
    k = rng.integers(0, 5, n)
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    org = np.array([p[0] for p in parts])[k]
    u = np.array([p[1] for p in parts])[k]
    v = np.array([p[2] for p in parts])[k]
    return org + a[:, None] * u + b[:, None] * v


def _edges(rng, n):
    """n points on the room's vertical and floor edges"""
    segs = [(c, EZ) for c in (O, O + EX, O + EY, O + EX + EY)] + [(O, EX), (O + EY, EX), (O, EY), (O + EX, EY)]
    k = rng.integers(0, len(segs), n)
    a = rng.uniform(0, 1, n)
    return np.array([s[0] for s in segs])[k] + a[:, None] * np.array([s[1] for s in segs])[k]


def to_sensor(pm, pose):
    pose = np.asarray(pose, np.float64)
    R = rot(pose[3], pose[4], pose[5])
    return (pm - pose[:3]) @ R


def room_scan(seed, pose, n_corner=470, n_surf=4000, n_outlier=200, noise=0.01):
    """(corner, surf, outlier) sensor-frame clouds, (n, 4) f32 with intensity"""
    rng = np.random.default_rng(seed)
    def cloud(pm):
        ps = to_sensor(pm + rng.normal(0, noise, pm.shape), pose)
        return np.concatenate([ps, rng.uniform(0, 100, (len(ps), 1))], 1).astype(np.float32)
    outl = _planes(rng, n_outlier) + rng.normal(0, 0.3, (n_outlier, 3))
    return cloud(_edges(rng, n_corner)), cloud(_planes(rng, n_surf)), cloud(outl)


def trajectory(n, seed=0):
    """n key poses (x, y, z, roll, pitch, yaw) along a loop inside the room"""
    rng = np.random.default_rng(seed)
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    xs, ys = 8 * np.cos(t), 5 * np.sin(t)
    return np.stack([xs, ys, 0.2 + 0.05 * np.sin(3 * t), rng.normal(0, 0.01, n), rng.normal(0, 0.01, n), t + 0.3], 1).astype(np.float32)
