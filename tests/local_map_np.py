"""An independent numpy restatement of the mapping node's local map (LM:1201-1349) for the local-map tests: the window's
key frames moved into the map frame in f32 (transformPointCloud, LM:627-650) with the trigonometry of libm's cosf /
sinf (the float overloads the reference calls), concatenated oldest first, and VoxelGrid as the project states it —
f32 box, stable order by PCL's linear voxel index, sequential f32 sums per voxel in input order."""
import ctypes
import ctypes.util

import numpy as np

_m = ctypes.CDLL(ctypes.util.find_library("m"))
for _f in (_m.cosf, _m.sinf):
    _f.argtypes, _f.restype = [ctypes.c_float], ctypes.c_float

F = np.float32


def trig(pose):
    """updateTransformPointCloudSinCos (LM:612-624): ctRoll, stRoll, ctPitch, stPitch, ctYaw, stYaw, tInX, tInY, tInZ"""
    x, y, z, roll, pitch, yaw = [F(v) for v in pose]
    return [F(f(float(a))) for a in (roll, pitch, yaw) for f in (_m.cosf, _m.sinf)] + [x, y, z]


def transform(pts, pose):
    cr, sr, cp, sp, cy, sy, tx, ty, tz = trig(pose)
    p = np.asarray(pts, F).reshape(-1, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    x1 = cy * x - sy * y
    y1 = sy * x + cy * y
    z1 = z
    x2 = x1
    y2 = cr * y1 - sr * z1
    z2 = sr * y1 + cr * z1
    return np.stack([cp * x2 + sp * z2 + tx, y2 + ty, -sp * x2 + cp * z2 + tz, p[:, 3]], 1).astype(F)


def voxel_grid(pts, leaf):
    """-> (centroids in ascending voxel order, or None for a box of more than 2^31 cells)"""
    p = np.asarray(pts, F).reshape(-1, 4)
    if len(p) == 0:
        return np.zeros((0, 4), F)
    inv = F(1.0) / F(leaf)
    xyz = p[:, :3]
    minb = np.floor(xyz.min(0) * inv).astype(np.int64)
    div = np.floor(xyz.max(0) * inv).astype(np.int64) - minb + 1
    if int(div[0]) * int(div[1]) * int(div[2]) > 2 ** 31:
        return None
    ijk = np.floor(xyz * inv).astype(np.int64) - minb
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    order = np.argsort(idx, kind="stable")
    s = idx[order]
    starts = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    counts = np.diff(np.r_[starts, len(p)])
    # sequential sums, vectorised across voxels: step j adds the j-th point of every run that is that long (the runs
    # taken longest first, so the active ones are a prefix)
    by_len = np.argsort(-counts, kind="stable")
    st, cn = starts[by_len], counts[by_len]
    sums = np.zeros((len(st), 4), F)
    for j in range(int(cn[0])):
        k = int(np.count_nonzero(cn > j))
        sums[:k] += p[order[st[:k] + j]]
    out = np.zeros_like(sums)
    out[by_len] = sums / counts[by_len].astype(F)[:, None]
    return out


def box_1m(c):
    if len(c) == 0:
        return [0, 0, 0], [1, 1, 1]
    f = np.floor(c[:, :3]).astype(np.int64)
    lo, hi = f.min(0), f.max(0)
    return lo.tolist(), (hi - lo + 1).tolist()


def local_map(frames, scan, window=50):
    """-> (six clouds in LOCAL_* order, sizes dict) as lins_host_local_map / lins_local_map_build report them"""
    used = frames[max(0, len(frames) - window):]
    corner = [transform(f[0], f[3]) for f in used]
    surf = []
    for f in used:  # LM:1242-1246: surf_i, then outlier_i
        surf += [transform(f[1], f[3]), transform(f[2], f[3])]
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros((0, 4), F)
    maps = [cat(corner), cat(surf)]
    sizes = dict(frames=len(used), status=0)
    empty = [np.zeros((0, 4), F)] * 6
    if any((~np.isfinite(m[:, :3]) | (np.abs(m[:, :3]) > 1e6)).any() for m in maps):
        sizes["status"] = -4
        res = empty
    else:
        res = [voxel_grid(maps[0], 0.2), voxel_grid(maps[1], 0.4), voxel_grid(scan[0], 0.2), voxel_grid(scan[1], 0.4),
               voxel_grid(scan[2], 0.4)]
        if all(r is not None for r in res):
            res.append(voxel_grid(np.concatenate([res[3], res[4]]), 0.4))
        if any(r is None for r in res):
            sizes["status"] = -3
            res = empty
    sizes["n"] = [len(r) for r in res]
    b = [box_1m(res[0]), box_1m(res[1])]
    sizes["box_min"], sizes["box_dim"] = [b[0][0], b[1][0]], [b[0][1], b[1][1]]
    return res, sizes
