"""Shared set-up of tests/test_gpu_map_pose.py and tests/test_gpu_streams_map_step.py (not a test): three streams on
seeded sequence scans, and the EXPLICIT chain a caller had to write before lins_streams_map_step — lins_map_associate_batch,
lins_local_map_build_streams, lins_scan2map_batch with LINS_MAP_LOCAL, host transform_update + key_rule, the two push
calls — with the pose state kept in Python.  lins_streams_map_step must give the same bits."""
import functools
import importlib

import numpy as np

PKG = "lins---lidar-inertial-slam_amd"
defs = importlib.import_module(PKG + "._ctypes_defs")
host = importlib.import_module(PKG + ".host")
sm = importlib.import_module(PKG + ".streams_map")

F = np.float32
N, STEPS, WINDOW, INTERVAL = 3, 8, 3, 0.3
MAX_PTS = 16384


def context(pkg, ieskf, n=N):
    return ieskf.IeskfContext(pkg.default_params(num_iter=8), max_batch=n, max_targets=16384)


@functools.lru_cache(maxsize=None)
def raws(step):
    """stream i's raw scan of step `step`: sweep `step` of the seeded sequence 70 + i"""
    return [host.synth_seq_raw_scan(70 + i, step) for i in range(N)]


@functools.lru_cache(maxsize=None)
def priors():
    st = np.zeros((N, 19))
    st[:, 6] = 1.0
    return st, np.stack([host.synth_pair(0).cov] * N)


def feed(c, step):
    """one odometry step of every stream"""
    st, cov = priors()
    c.streams_step_raw(raws(step), st, cov)


def setup(c, archive=True):
    c.streams_init(N)
    c.local_map_init(N, WINDOW, MAX_PTS)
    if archive:
        c.archive_init(N, 2 * STEPS, 1 << 19)


def odometry(step):
    """(transform_sum, time, imu_roll, imu_pitch, has_imu) per stream at `step`: synthetic transformSum rows — stream 0
    drifts 0.2 m per scan (not every scan moves 0.3 m from the last key frame), stream 1 0.5 m per scan, stream 2 0.5 m
    with the time stamp of step 4 repeating step 3's (the interval gate stops it); stream 1 has IMU angles"""
    rows = []
    for i, drift in enumerate((0.2, 0.5, 0.5)):
        s = np.array([0.002 * step, 0.01 * step * (i + 1), -0.003 * step, 0.02 * step, -0.01 * step, drift * step], F)
        t = 0.4 * (3 if (i == 2 and step == 4) else step)
        rows.append((s, t, F(0.01 * step), F(-0.02 * step), i == 1))
    return rows


def odoms(step, streams=range(N)):
    o = odometry(step)
    return [sm.odom(o[i][0], o[i][1], o[i][2], o[i][3], o[i][4]) for i in streams]


def fresh_state():
    return dict(bef=np.zeros(6, F), aft=np.zeros(6, F), tobe=np.zeros(6, F), last=np.zeros(6, F), prev=np.zeros(3, F), n_frames=0,
                last_time=-1.0)


def key_pose_of(t):
    return np.array([t[3], t[4], t[5], t[0], t[1], t[2]], F)


def skipped():
    z = np.zeros(6, F)
    return dict(tobe_start=z, transform=z, key_pose=z, iters=0, converged=0, degenerate=0, n_sel=0, status=defs.MAP_STEP_SKIPPED,
                key_frame=0, ring_age=-1, archive_id=-1)


def explicit_step(c, states, streams, odo, archive=True, clock=None):
    """the chain on context c; states: per-stream dicts (fresh_state), changed in place; odo: per entry
    (transform_sum, time, imu_roll, imu_pitch, has_imu).  Returns the result dicts lins_streams_map_step would.
    clock: a one-element list that collects the seconds spent inside the five library calls (tools/streams_map_step_rate.py)."""
    import time as _time

    def timed(fn, *a):
        t0 = _time.perf_counter()
        r = fn(*a)
        if clock is not None:
            clock[0] += _time.perf_counter() - t0
        return r

    out = [None] * len(streams)
    batch = []
    for k, s in enumerate(streams):
        if odo[k][1] - states[s]["last_time"] >= INTERVAL:  # LM:1821, f64
            batch.append(k)
        else:
            out[k] = skipped()
    if not batch:
        return out
    which = [streams[k] for k in batch]
    start = timed(sm.map_associate_batch, c, [states[s]["bef"] for s in which], [states[s]["aft"] for s in which], [odo[k][0] for k in batch])
    sizes = timed(c.local_map_build_streams, which, which)
    res = timed(c.scan2map_batch, [defs.MapProblem.local(t) for t in start])
    keys = []
    for j, k in enumerate(batch):
        st, (total, time, roll, pitch, has_imu) = states[which[j]], odo[k]
        r = dict(tobe_start=start[j].copy(), key_pose=np.zeros(6, F), key_frame=0, ring_age=-1, archive_id=-1, status=sizes[j]["status"],
                 iters=0, converged=0, degenerate=0, n_sel=0)
        if sizes[j]["status"] == 0:
            r.update((f, res[j][f]) for f in ("iters", "converged", "degenerate", "n_sel"))
            st["tobe"] = res[j]["transform"].copy()
            if sizes[j]["n"][0] > 10 and sizes[j]["n"][1] > 100:  # LM:1636
                st["tobe"], st["bef"], st["aft"] = host_update(st["tobe"], has_imu, roll, pitch, total, st["bef"], st["aft"])
            save, st["prev"] = sm.host_key_rule(st["prev"], st["aft"], st["n_frames"] > 0)
            if save:
                if st["n_frames"] == 0:  # LM:1676-1686
                    r["key_pose"] = st["tobe"].copy()
                else:  # LM:1699-1704, 1737-1749 with iSAM2 as the identity
                    r["key_pose"] = st["aft"].copy()
                    st["tobe"] = st["aft"].copy()
                st["last"] = r["key_pose"].copy()
                st["n_frames"] += 1
                r["key_frame"] = 1
                keys.append(j)
            st["last_time"] = time
        r["transform"] = st["aft"].copy()
        out[k] = r
    if keys:
        poses = [key_pose_of(out[batch[j]]["key_pose"]) for j in keys]
        timed(c.local_map_push_scans, keys, poses)
        ids = timed(c.archive_push_scans, keys, poses, [odo[batch[j]][1] for j in keys]) if archive else [-1] * len(keys)
        for j, i in zip(keys, ids):
            out[batch[j]]["ring_age"], out[batch[j]]["archive_id"] = 0, i
    return out


def host_update(tobe, has_imu, roll, pitch, total, bef, aft):
    return sm.host_transform_update(tobe, has_imu, roll, pitch, total, bef, aft)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def same_result(a, b):
    """two result dicts equal, float fields by their bits"""
    if set(a) != set(b):
        return False
    for f in a:
        if isinstance(a[f], np.ndarray):
            if not np.array_equal(bits(a[f]), bits(b[f])):
                return False
        elif a[f] != b[f]:
            return False
    return True


def same_state(a, b):
    return same_result({k: v for k, v in a.items()}, {k: v for k, v in b.items()})
