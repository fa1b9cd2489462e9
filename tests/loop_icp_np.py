"""An independent numpy statement of the loop-closure ICP's contract (include/lins_map.h): exhaustive search with the
f32 move and distance in the contract's operation order, Kabsch through np.linalg.svd in f64 on CENTRED points, plain
np.sum.  It shares no code with csrc/loop_icp_math.h: the host restatement is held against it by
tests/test_loop_icp_host.py — correspondences bit for bit, the rest within the bar that summation order and SVD
algorithm explain.  Also the fixtures the loop-closure tests share."""
import numpy as np

from local_map_synth import room_scan, trajectory
from map_synth import rot

F = np.float32
DBL_MAX = np.finfo(np.float64).max
NONE, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
DEFAULTS = dict(max_corr_dist=100.0, max_iterations=100, transformation_epsilon=1e-6, fitness_epsilon=1e-6, rel_mse=1e-5,
                rotation_threshold=0.99999, min_correspondences=3)


def move(T, S):
    """step 1: f32, ((m00 x + m01 y) + m02 z) + m03"""
    M = np.asarray(T, np.float64).reshape(4, 4).astype(F)
    x, y, z = (np.ascontiguousarray(S[:, k], F) for k in range(3))
    return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], 1).astype(F)


def correspondences(S, G, T, cap=0.0, chunk=256):
    """step 2 by exhaustive search: (idx (-1: none), d, moved points); ties go to the smaller index (np.argmin)"""
    S, G = np.asarray(S, F).reshape(-1, 4), np.asarray(G, F).reshape(-1, 4)
    X = move(T, S)
    idx, d = np.full(len(S), -1, np.int32), np.zeros(len(S), F)
    if len(G):
        for a in range(0, len(S), chunk):
            q = X[a:a + chunk]
            dx, dy, dz = (q[:, None, k] - G[None, :, k] for k in range(3))
            dd = ((dx * dx + dy * dy) + dz * dz).astype(F)
            j = np.argmin(dd, 1)
            idx[a:a + chunk], d[a:a + chunk] = j, dd[np.arange(len(q)), j]
        if cap > 0:
            far = ~(d <= F(cap) * F(cap))
            idx[far], d[far] = -1, 0
    return idx, d, X


def kabsch(X, Y):
    """the rigid (R, t) taking X onto Y in the least-squares sense, f64, centred, np.linalg.svd"""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    mx, my = X.sum(0) / len(X), Y.sum(0) / len(Y)
    H = (X - mx).T @ (Y - my)
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    R = V @ np.diag([1.0, 1.0, np.sign(np.linalg.det(V @ U.T))]) @ U.T
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = R, my - R @ mx
    return D


def round_from_pairs(X, Y, d, T, mse_prev, iterations, **kw):
    """steps 3-6 of one round from its correspondences — the moved points X, their targets Y, the f32 d of each — entering
    with T, mse_prev and `iterations` fitted rounds: the round's dict (T_in, n_corr, delta, T_out, stop, reason, mse);
    reason NONE: the loop goes on"""
    p = dict(DEFAULTS, **kw)
    T = np.asarray(T, np.float64).reshape(4, 4)
    r = dict(T_in=T.copy(), n_corr=len(X), delta=np.eye(4), stop=np.zeros(4), reason=NONE, mse=0.0, T_out=T.copy())
    if r["n_corr"] < p["min_correspondences"]:
        r["reason"] = NO_CORRESPONDENCES
        return r
    D = kabsch(np.asarray(X)[:, :3], np.asarray(Y)[:, :3])
    mse = float(np.sum(np.asarray(d).astype(np.float64)) / r["n_corr"])
    with np.errstate(over="ignore"):
        ad = abs(mse - mse_prev)
        q = np.array([0.5 * (np.trace(D[:3, :3]) - 1.0), float(D[:3, 3] @ D[:3, 3]), ad, ad / mse_prev])
    if iterations + 1 >= p["max_iterations"]:
        reason = ITERATIONS
    elif q[0] >= p["rotation_threshold"] and q[1] <= p["transformation_epsilon"]:
        reason = TRANSFORM
    elif q[2] < p["fitness_epsilon"]:
        reason = ABS_MSE
    elif q[3] < p["rel_mse"]:
        reason = REL_MSE
    else:
        reason = NONE
    r.update(delta=D, T_out=D @ T, stop=q, reason=reason, mse=mse)
    return r


def icp(S, G, max_rounds=0, **kw):
    """-> (rounds, result), the shapes of host.loop_icp_trace"""
    p = dict(DEFAULTS, **kw)
    S, G = np.asarray(S, F).reshape(-1, 4), np.asarray(G, F).reshape(-1, 4)
    T, mse_prev, rounds = np.eye(4), DBL_MAX, []
    res = dict(iterations=0, converged=0, reason=NONE, n_corr=0, mse=0.0)
    while res["reason"] == NONE and (max_rounds == 0 or len(rounds) < max_rounds):
        idx, d, X = correspondences(S, G, T, p["max_corr_dist"])
        ok = idx >= 0
        r = round_from_pairs(X[ok], G[idx[ok], :3], d[ok], T, mse_prev, res["iterations"], **kw)
        res["n_corr"] = r["n_corr"]
        rounds.append(r)
        if r["reason"] == NO_CORRESPONDENCES:
            res["reason"] = NO_CORRESPONDENCES
            break
        T = r["T_out"]
        res["iterations"] += 1
        mse_prev = res["mse"] = r["mse"]
        if r["reason"] != NONE:
            res["reason"], res["converged"] = r["reason"], 1
    idx, d, _ = correspondences(S, G, T, 0.0)
    ok = idx >= 0
    res["n_fitness"] = int(ok.sum())
    res["fitness"] = float(np.sum(d[ok].astype(np.float64)) / ok.sum()) if ok.any() else DBL_MAX
    res["transform"] = T
    return rounds, res


# ---- LM:1156-1166 ------------------------------------------------------------------------------------------------
def get_transformation(x, y, z, roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    t = np.eye(4)
    t[:3, :3], t[:3, 3] = Rz @ Ry @ Rx, (x, y, z)
    return t


def euler_of(t):
    return t[0, 3], t[1, 3], t[2, 3], np.arctan2(t[2, 1], t[2, 2]), np.arcsin(-t[2, 0]), np.arctan2(t[1, 0], t[0, 0])


def pose_from(T, wrong):
    """f64 statement of lins_host_loop_pose_from (which is f32): (x, y, z, roll, pitch, yaw)"""
    x, y, z, roll, pitch, yaw = euler_of(np.asarray(T, np.float64).reshape(4, 4).astype(F).astype(np.float64))
    w = np.asarray(wrong, F).astype(np.float64)
    return np.array(euler_of(get_transformation(z, x, y, yaw, roll, pitch) @ get_transformation(w[2], w[0], w[1], w[5], w[3], w[4])))


# ---- fixtures ------------------------------------------------------------------------------------------------------
SRC = dict(n_corner=40, n_surf=260, n_outlier=0)
TGT = dict(n_corner=60, n_surf=500, n_outlier=0)
ERR = np.array([0.3, 0.2, 0.1, 0.0, 0.0, np.deg2rad(2.0)])  # the injected pose error: (0.3, 0.2, 0.1) m, 2 deg of yaw


def to_map(cloud, pose):
    """a sensor-frame cloud in the map frame (f64 arithmetic, rounded to f32 once)"""
    pose = np.asarray(pose, np.float64)
    out = np.asarray(cloud, F).copy()
    out[:, :3] = (cloud[:, :3].astype(np.float64) @ rot(pose[3], pose[4], pose[5]).T + pose[:3]).astype(F)
    return out


def voxel_centroids(cloud, leaf):
    """a plain VoxelGrid (centroid per occupied voxel, f64 means) — fixture material, not the project's contract"""
    key = np.floor(cloud[:, :3].astype(np.float64) / leaf).astype(np.int64)
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv)
    return np.stack([np.bincount(inv, cloud[:, k].astype(np.float64)) / cnt for k in range(4)], 1).astype(F)


def problem(seed, n_frames=9, err=ERR):
    """(source, target, wrong pose, true pose): the target is n_frames room frames along the trajectory through leaf 0.4,
    the source one more frame at the middle pose, put into the map frame with the pose error added"""
    poses = trajectory(n_frames, seed=seed)
    frames = [room_scan(1000 * seed + i, poses[i], **TGT) for i in range(n_frames)]
    tgt = voxel_centroids(np.concatenate([to_map(np.concatenate(f[:2]), poses[i]) for i, f in enumerate(frames)]), 0.4)
    true = poses[n_frames // 2].astype(np.float64)
    wrong = (true + err).astype(F)
    s = room_scan(1000 * seed + 500, true, **SRC)
    return to_map(np.concatenate(s[:2]), wrong), tgt, wrong, true.astype(F)
