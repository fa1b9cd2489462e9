"""The problems the loop-closure ICP tests share (tests/test_loop_icp_inputs.py asserts on the CPU what the GPU tests
of tests/test_gpu_loop_icp.py rest on).  Built once per process."""
import functools
import importlib

import numpy as np

import loop_icp_np as lnp
from local_map_synth import room_scan, trajectory

F = np.float32
# Seeds of loop_icp_np.problem / of the archive case.  CHOSEN, by a scan over seeds 0 .. 39 on the CPU restatement, so
# that no stop quantity of any round comes near its threshold (test_loop_icp_inputs.py states and asserts the margins):
# the device's sums differ from the restatement's in the last bits, and a quantity that sat on its threshold could stop
# the two loops in different rounds.
WHOLE_LOOP_SEEDS = (20, 15)
ARCHIVE_SEED = 3
SMALL = dict(n_corner=60, n_surf=500, n_outlier=40)
# the four stop thresholds of lins_loop_icp_default_params, in the order of the trace's `stop`
THRESHOLDS = dict(rotation=0.99999, translation=1e-6, abs_mse=1e-6, rel_mse=1e-5)


@functools.lru_cache(maxsize=None)
def whole_loop_problems():
    """[(source, target, wrong pose, true pose)]"""
    return [lnp.problem(s) for s in WHOLE_LOOP_SEEDS]


@functools.lru_cache(maxsize=None)
def archive_case():
    """12 key frames along a closed loop; the latest is stored with a pose that is off by loop_icp_np.ERR.  Returns
    (frames [(corner, surf, outlier, pose)], specs, wrong pose, true pose): specs[0] the latest frame as
    latestSurfKeyFrameCloud (corner | surf, leaf 0, DROP_NEGATIVE), specs[1] a history window as
    nearHistorySurfKeyFrameCloudDS (frames 0 .. 8: closest = 4, +-4; corner | surf, leaf 0.4)."""
    poses = trajectory(12, seed=ARCHIVE_SEED)
    frames = [room_scan(7000 + 100 * ARCHIVE_SEED + i, poses[i], **SMALL) + (poses[i],) for i in range(12)]
    true = poses[11].copy()
    wrong = (true.astype(np.float64) + lnp.ERR).astype(F)
    frames[11] = frames[11][:3] + (wrong,)
    frames[11][1][:7, 3] = -F(2.0)  # a few points that DROP_NEGATIVE drops
    specs = [dict(slot=0, ids=[11], clouds=3, leaf=0.0, flags=1), dict(slot=0, ids=list(range(9)), clouds=3, leaf=0.4, flags=0)]
    return frames, specs, wrong, true


@functools.lru_cache(maxsize=None)
def archive_clouds():
    """(source, target) of archive_case by the CPU restatement of the assembly (host.submap)"""
    host = importlib.import_module("lins---lidar-inertial-slam_amd.host")
    frames, specs, _, _ = archive_case()
    return tuple(host.submap(frames, sp["ids"], sp["clouds"], sp["leaf"], sp["flags"])[0] for sp in specs)


def all_whole_loop_clouds():
    """every (source, target) a GPU whole-loop test runs"""
    return [(p[0], p[1]) for p in whole_loop_problems()] + [archive_clouds()]


# ---- search fixtures: (name, source, target); T is the identity, the queries are the source points -----------------
def _cloud(xyz):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.concatenate([xyz, np.arange(len(xyz), dtype=F)[:, None]], 1)


@functools.lru_cache(maxsize=None)
def search_cases():
    rng = np.random.default_rng(5)
    out = []
    q = _cloud(rng.uniform(-4, 4, (70, 3)))
    for ng in (0, 1, 5, 511, 512, 513):
        out.append((f"ng={ng}", q, _cloud(rng.uniform(-4, 4, (ng, 3)))))
    # the integer lattice 0 .. 4 cubed; queries at cell centres (eight lattice points at the same d) and on cell faces
    # (four at the same d): the smallest index wins
    lat = _cloud(np.stack(np.meshgrid(*[np.arange(5.0)] * 3, indexing="ij"), -1).reshape(-1, 3))
    centres = np.stack(np.meshgrid(*[np.arange(4.0) + 0.5] * 3, indexing="ij"), -1).reshape(-1, 3)
    faces = centres.copy()
    faces[:, 0] = np.floor(faces[:, 0])
    out.append(("lattice", _cloud(np.concatenate([centres, faces])), lat))
    # duplicated target points (equal d, differing index, the same cell)
    dup = rng.uniform(-3, 3, (200, 3))
    out.append(("duplicates", _cloud(rng.uniform(-3, 3, (64, 3))), _cloud(np.concatenate([dup, dup[::-1], dup[:50]]))))
    # queries one and three cells outside the box, and one 99.9 m away; the box is [0, 6)^3
    box = rng.uniform(0, 6, (400, 3))
    outside = [[-0.5, 3, 3], [6.5, 3, 3], [3, -2.5, 3], [3, 3, 8.5], [-2.5, -2.5, -2.5], [8.5, 6.5, -0.5], [3 + 99.9, 3, 3]]
    out.append(("outside", _cloud(outside), _cloud(box)))
    # boxes one cell thick, along every axis
    for a in range(3):
        slab = rng.uniform(0, 7, (300, 3))
        slab[:, a] = rng.uniform(0.1, 0.9, 300)
        qs = rng.uniform(-1, 8, (40, 3))
        out.append((f"slab{a}", _cloud(qs), _cloud(slab)))
    return out


@functools.lru_cache(maxsize=None)
def beyond_cap_case():
    """a query 150 m from a small target: beyond the cap of 100 m"""
    rng = np.random.default_rng(9)
    return _cloud([[150.0, 0.5, 0.5], [0.5, 0.5, 0.5]]), _cloud(rng.uniform(0, 2, (30, 3)))


# ---- the bar of "equal up to summation order and SVD algorithm" ----------------------------------------------------
# Measured on the CPU (tests/test_loop_icp_host.py prints it): the largest difference between the host restatement and
# the numpy statement over every round of every whole-loop problem above is 2.5e-15 in an entry of T and 0 in mse and
# fitness.  The bar is ten times that; where the measured difference is 0, ten times one unit in the last place of the
# values themselves (mse and fitness are ~0.08: 1.4e-17).  The device is held to the same bar against the restatement.
BAR_T = 2.5e-14
BAR_MSE = 1.4e-16
