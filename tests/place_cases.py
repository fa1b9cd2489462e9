"""The frames the place-recognition tests share (tests/test_place_host.py on the CPU, tests/test_gpu_place.py on the
device).  A frame is (corner, surf, outlier), (n, 4) f32 each; clouds are built in polar form about the up axis so that
the test decides how near a cell edge a point may come."""
import functools

import numpy as np

F = np.float32
NR, NS = 20, 60
R_MAX, LIFT = 80.0, 2.0
DS, DR = 2 * np.pi / NS, R_MAX / NR
E = np.zeros((0, 4), F)


def polar_cloud(rho, theta, h, up=1, lift=LIFT):
    """points with the given planar range, azimuth (from axis (up + 1) % 3 towards (up + 2) % 3) and lifted height h"""
    rho, theta, h = (np.atleast_1d(np.asarray(v, np.float64)) for v in (rho, theta, h))
    p = np.zeros((len(rho), 4))
    p[:, (up + 1) % 3], p[:, (up + 2) % 3], p[:, up] = rho * np.cos(theta), rho * np.sin(theta), h - lift
    p[:, 3] = np.arange(len(rho))
    return p.astype(F)


def place(seed, n=400, up=1, turn=0, jitter=0.0, drop=0.0):
    """a random place seen after a yaw of `turn` sectors: every point at least 0.2 m and 0.01 rad inside its cell, heights
    in [0.5, 6] (lifted), far from the floor; jitter: uniform height noise of a revisit, drop: the share of points not seen
    again.  A feature the unturned frame sees at azimuth phi this frame sees at phi + turn * DS."""
    rng = np.random.default_rng(seed)
    ring, sec = rng.integers(0, NR, n), rng.integers(0, NS, n)
    rho = (ring + rng.uniform(0.05, 0.95, n)) * DR
    theta = -np.pi + (sec + rng.uniform(0.1, 0.9, n)) * DS
    h = rng.uniform(0.5, 6.0, n)
    rev = np.random.default_rng(seed * 7919 + turn * 31 + 1)
    keep = rev.uniform(0, 1, n) >= drop
    h = h + rev.uniform(-jitter, jitter, n)
    theta = theta + turn * DS
    theta = np.where(theta >= np.pi, theta - 2 * np.pi, theta)
    return polar_cloud(rho[keep], theta[keep], h[keep], up)


def frame(cloud):
    """a cloud cut into the three clouds of a key frame"""
    n = len(cloud)
    return cloud[:n // 5].copy(), cloud[n // 5:n - n // 10].copy(), cloud[n - n // 10:].copy()


@functools.lru_cache(maxsize=None)
def winner_cases(up=1):
    """[(query frame, candidate frames, times, true id, true shift)]: the query is place s, the candidates are twelve
    other places and, at `true id`, the query's place turned by `true shift` sectors and lightly perturbed"""
    out = []
    for s, (turn, at) in enumerate([(7, 3), (0, 0), (53, 12), (30, 6), (1, 9), (59, 5)]):
        cands = [frame(place(1000 + 50 * s + i, up=up)) for i in range(12)]
        cands.insert(at, frame(place(100 + s, up=up, turn=turn, jitter=0.02, drop=0.05)))
        out.append((frame(place(100 + s, up=up)), cands, np.arange(13, dtype=np.float64), at, turn))
    return out


def _f32_below(x):
    return np.nextafter(F(x), F(-np.inf))


@functools.lru_cache(maxsize=None)
def edge_frames(up=1):
    """{name: frame}: the cells' and the floor's edges, exactly"""
    f = {}
    f["empty"] = (E, E, E)
    f["single"] = (polar_cloud(10.3, 0.4, 3.0, up), E, E)
    f["rho0"] = (E, polar_cloud(0.0, 0.0, 1.0, up), E)
    at_rmax = polar_cloud(R_MAX, 0.0, 1.0, up)
    at_rmax[0, (up + 1) % 3], at_rmax[0, (up + 2) % 3] = F(R_MAX), F(0)
    f["at_rmax"] = (at_rmax, polar_cloud(12.0, 1.0, 1.5, up), E)
    edge = polar_cloud(4.0, 0.0, 1.0, up)
    edge[0, (up + 1) % 3], edge[0, (up + 2) % 3] = F(4.0), F(0)  # exactly 4 m: ring 1, azimuth exactly 0
    f["ring_edge_az0"] = (edge, E, E)
    az = np.zeros((3, 4), F)
    az[:, up] = F(1.0 - LIFT)
    az[0, (up + 1) % 3], az[0, (up + 2) % 3] = F(-9.0), F(0.0)    # +pi
    az[1, (up + 1) % 3], az[1, (up + 2) % 3] = F(-17.0), -F(0.0)  # -pi
    az[2, (up + 1) % 3], az[2, (up + 2) % 3] = F(25.0), -F(0.0)   # -0
    f["az_pi"] = (E, E, az)
    fl = polar_cloud([6.0, 14.0, 22.0], [0.5, 1.5, 2.5], [0, 0, 0], up)
    at = F(2.0 ** -10) - F(LIFT)  # exactly representable: h = 2^-10
    fl[:, up] = [_f32_below(at), at, np.nextafter(at, F(np.inf))]
    f["floor"] = (fl, E, E)
    f["one_column"] = (E, polar_cloud(np.arange(NR) * DR + 1.7, np.full(NR, 0.3), np.linspace(1, 5, NR), up), E)
    return f


def half_turn_scene(up=1):
    """(query frame, candidate frame): the candidate is a place and the same place turned by half a turn, in one frame,
    seen after a yaw of 4 sectors: shifts 4 and 34 tie exactly"""
    q = place(555, n=300, up=up)
    sym = np.concatenate([q, q * np.array([1, 1, 1, 1], F)])
    a, b = (up + 1) % 3, (up + 2) % 3
    sym[len(q):, a] *= -1
    sym[len(q):, b] *= -1
    rho = np.hypot(sym[:, a].astype(np.float64), sym[:, b].astype(np.float64))
    theta = np.arctan2(sym[:, b].astype(np.float64), sym[:, a].astype(np.float64))
    return frame(sym), frame(polar_cloud(rho, theta + 4 * DS, sym[:, up].astype(np.float64) + LIFT, up)), 4
