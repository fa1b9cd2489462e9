"""An independent numpy statement of the key-frame archive's selection and of the reference's three compositions
(publishGlobalMap LM:984-1031, detectLoopClosure LM:1043-1112) for the archive tests, built on local_map_np.transform /
voxel_grid: the radius search as the exact search ordered by (f32 squared distance, id), the key-pose VoxelGrid with the
truncated mean id, and the assembly — the chosen clouds of the chosen frames in the map frame, concatenated, filtered or
compacted."""
import numpy as np

from local_map_np import F, box_1m, transform, voxel_grid

CORNER, SURF, OUTLIER = 1, 2, 4
DROP_NEGATIVE = 1
ALL = CORNER | SURF | OUTLIER
H = 25  # historyKeyframeSearchNum


def radius_search(poses, centre, radius):
    """ids of the poses with ((dx*dx + dy*dy) + dz*dz) <= radius*radius in f32, ascending (that distance, id)"""
    p = np.asarray(poses, F).reshape(-1, 6)[:, :3]
    d = p - np.asarray(centre, F)
    sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert sq.dtype == F
    hit = np.flatnonzero(sq <= F(radius) * F(radius))
    return hit[np.lexsort((hit, sq[hit]))]


def select_radius(poses, centre, radius, pose_leaf):
    p = np.asarray(poses, F).reshape(-1, 6)
    hit = radius_search(p, centre, radius)
    pts = np.concatenate([p[hit, :3], hit.astype(F)[:, None]], 1)
    ds = voxel_grid(pts, pose_leaf)
    return ds[:, 3].astype(np.int32)  # (int) of the averaged intensity (LM:1007)


def find_loop(poses, times, centre, radius, now, min_gap_s):
    for i in radius_search(poses, centre, radius):
        if abs(float(times[i]) - float(now)) > min_gap_s:
            return int(i)
    return -1


def submap(frames, ids, clouds, leaf, flags=0):
    """frames: [(corner, surf, outlier, pose)] by id -> (cloud, info dict as lins_submap_info)"""
    parts = [transform(frames[i][q], frames[i][3]) for i in ids for q in range(3) if clouds & (1 << q)]
    cat = np.concatenate(parts) if parts else np.zeros((0, 4), F)
    info = dict(frames=len(ids), points_in=len(cat), status=0)
    if (~np.isfinite(cat[:, :3]) | (np.abs(cat[:, :3]) > 1e6)).any():
        info["status"], res = -4, cat[:0]
    elif leaf > 0:
        res = voxel_grid(cat, leaf)
        if res is None:
            info["status"], res = -3, cat[:0]
    elif flags & DROP_NEGATIVE:
        res = cat[cat[:, 3].astype(np.int32) >= 0]  # C's cast: truncation towards zero
    else:
        res = cat
    info["n"] = len(res)
    info["box_min"], info["box_dim"] = box_1m(res) if leaf > 0 else ([0, 0, 0], [1, 1, 1])
    return res, info


def global_map_spec(poses, centre):
    return dict(ids=select_radius(poses, centre, 500.0, 1.0), clouds=ALL, leaf=0.4, flags=0)


def history_spec(n_frames, closest):
    return dict(ids=np.arange(max(0, closest - H), min(n_frames - 1, closest + H) + 1), clouds=CORNER | SURF, leaf=0.4, flags=0)


def latest_spec(n_frames):
    return dict(ids=np.array([n_frames - 1]), clouds=CORNER | SURF, leaf=0.0, flags=DROP_NEGATIVE)
