"""The mapping node's run() for streams (include/lins_streams_map.h): per-stream map poses resident on the device, one
call per scan.  Functions over an ieskf.IeskfContext; the CPU restatement of the arithmetic is at the end
(liblins_host.so, include/lins_host.h lins_host_map_*).  Pose vectors are (rx, ry, rz, tx, ty, tz), f32."""
import ctypes as C

import numpy as np

from . import host as _host
from . import ieskf as _ieskf
from ._ctypes_defs import MapOdomC, MapPoseStateC, MapStepResultC, map_pose_state

_FP = C.POINTER(C.c_float)


def _rows(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 6)


def map_associate_batch(ctx, bef, aft, total):
    """lins_map_associate_batch: transformAssociateToMap on the device for (n, 6) rows of transformBefMapped,
    transformAftMapped, transformSum -> (n, 6) transformTobeMapped"""
    b, a, s = _rows(bef), _rows(aft), _rows(total)
    assert b.shape == a.shape == s.shape
    out = np.zeros_like(b)
    L = _ieskf.lib()
    L.lins_map_associate_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ctx._check(L.lins_map_associate_batch(ctx._h, len(b), b.ctypes.data, a.ctypes.data, s.ctypes.data, out.ctypes.data))
    return out


def init(ctx, n_streams, process_interval=0.3):
    L = _ieskf.lib()
    L.lins_streams_map_init.argtypes = [C.c_void_p, C.c_int, C.c_double]
    ctx._check(L.lins_streams_map_init(ctx._h, int(n_streams), float(process_interval)))


def get_pose(ctx, stream):
    """-> dict(bef, aft, tobe, last, prev, n_frames, last_time) of one stream (synchronises)"""
    s = MapPoseStateC()
    L = _ieskf.lib()
    L.lins_streams_map_get_pose.argtypes = [C.c_void_p, C.c_int, C.POINTER(MapPoseStateC)]
    ctx._check(L.lins_streams_map_get_pose(ctx._h, int(stream), C.byref(s)))
    return s.as_dict()


def set_pose(ctx, stream, state):
    """state: a dict as get_pose gives it (missing fields: as after init)"""
    s = map_pose_state(state)
    L = _ieskf.lib()
    L.lins_streams_map_set_pose.argtypes = [C.c_void_p, C.c_int, C.POINTER(MapPoseStateC)]
    ctx._check(L.lins_streams_map_set_pose(ctx._h, int(stream), C.byref(s)))


def loop(ctx, on=True):
    """lins_streams_map_loop: with it on, every step pushes the factor of each key frame it stores to the pose graph
    (slot = stream) and lins_loop_step finds graph and archive in step"""
    L = _ieskf.lib()
    L.lins_streams_map_loop.argtypes = [C.c_void_p, C.c_int]
    ctx._check(L.lins_streams_map_loop(ctx._h, int(bool(on))))


def surround(ctx, on=True, radius=50.0, pose_leaf=1.0):
    """lins_streams_map_surround: with it on, every step builds its local map from the key frames of the archive within
    `radius` of the robot (the mapping node with loopClosureEnableFlag off, LM:1247-1315) instead of the ring"""
    L = _ieskf.lib()
    L.lins_streams_map_surround.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float]
    ctx._check(L.lins_streams_map_surround(ctx._h, int(bool(on)), float(radius), float(pose_leaf)))


def surround_list(ctx, stream):
    """lins_streams_map_surround_list: the stream's surroundingExistingKeyPosesID as the last step left it"""
    L = _ieskf.lib()
    L.lins_streams_map_surround_list.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    cap = 64
    while True:
        ids = np.zeros(cap, np.int32)
        rc = L.lins_streams_map_surround_list(ctx._h, int(stream), ids.ctypes.data, cap)
        if rc == -3 and cap < (1 << 24):  # LINS_E_CAPACITY
            cap *= 8
            continue
        if rc < 0:
            ctx._check(rc)
        return ids[:rc].tolist()


def team(ctx, on=True, radius=50.0, pose_leaf=1.0):
    """lins_streams_map_team: with it on, every step builds its local map from the key frames of every slot of the
    stream's group (team_groups) that the team selection takes around the robot -> the C return code"""
    L = _ieskf.lib()
    L.lins_streams_map_team.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float]
    return L.lins_streams_map_team(ctx._h, int(bool(on)), float(radius), float(pose_leaf))


def team_groups(ctx, slots, groups):
    """lins_streams_map_team_groups: slots[k] joins group groups[k] (>= 0) or stands alone (-1) -> the C return code"""
    sv, gv = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(groups, np.int32)
    assert len(sv) == len(gv)
    L = _ieskf.lib()
    L.lins_streams_map_team_groups.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return L.lins_streams_map_team_groups(ctx._h, len(sv), sv.ctypes.data if len(sv) else None, gv.ctypes.data if len(sv) else None)


def team_group(ctx, slot):
    """lins_streams_map_team_group: the slot's group (-1: alone)"""
    g = C.c_int32(-2)
    L = _ieskf.lib()
    L.lins_streams_map_team_group.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    ctx._check(L.lins_streams_map_team_group(ctx._h, int(slot), C.byref(g)))
    return int(g.value)


def team_list(ctx, stream):
    """lins_streams_map_team_list: the (slot, id) pairs of the stream's last completed team build, as a list of tuples"""
    L = _ieskf.lib()
    L.lins_streams_map_team_list.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    cap = 64
    while True:
        pairs = np.zeros((cap, 2), np.int32)
        rc = L.lins_streams_map_team_list(ctx._h, int(stream), pairs.ctypes.data, cap)
        if rc == -3 and cap < (1 << 24):  # LINS_E_CAPACITY
            cap *= 8
            continue
        if rc < 0:
            ctx._check(rc)
        return [tuple(p) for p in pairs[:rc].tolist()]


def odom(transform_sum, time, imu_roll=0.0, imu_pitch=0.0, has_imu=False):
    o = MapOdomC()
    o.transform_sum[:] = [float(v) for v in np.asarray(transform_sum, np.float32)]
    o.imu_roll, o.imu_pitch, o.has_imu, o.time = float(imu_roll), float(imu_pitch), int(bool(has_imu)), float(time)
    return o


def step(ctx, streams, odoms):
    """lins_streams_map_step for the streams named; odoms: one odom(...) per entry -> the per-entry result dicts"""
    n = len(streams)
    assert len(odoms) == n
    sv = np.ascontiguousarray(streams, np.int32)
    arr = (MapOdomC * max(n, 1))(*odoms)
    out = (MapStepResultC * max(n, 1))()
    L = _ieskf.lib()
    L.lins_streams_map_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(MapOdomC), C.POINTER(MapStepResultC)]
    ctx._check(L.lins_streams_map_step(ctx._h, n, sv.ctypes.data, arr, out))
    return [out[k].as_dict() for k in range(n)]


def download(ctx, entry, which):
    """cloud `which` (LOCAL_*) of entry `entry` of the local map's last build — after a step that is the step's own
    build, whose sizes the caller has not seen — as an (n, 4) f32 array"""
    L = _ieskf.lib()
    L.lins_local_map_download.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    cap = 1 << 15
    while True:
        buf = np.zeros((cap, 4), np.float32)
        rc = L.lins_local_map_download(ctx._h, int(entry), int(which), buf.ctypes.data, cap)
        if rc == -3 and cap < (1 << 26):  # LINS_E_CAPACITY
            cap *= 4
            continue
        if rc < 0:
            ctx._check(rc)
        return buf[:rc].copy()


def last_ms(ctx):
    """HIP-event times (ms) of the associate and finish kernels of the last step"""
    a, b = C.c_float(0), C.c_float(0)
    L = _ieskf.lib()
    L.lins_last_streams_map_ms.argtypes = [C.c_void_p, _FP, _FP]
    ctx._check(L.lins_last_streams_map_ms(ctx._h, C.byref(a), C.byref(b)))
    return a.value, b.value


# ---- the CPU restatement (csrc/host/map_pose.cpp) ----------------------------------------------------------------
def _f6(v, n=6):
    a = np.array(v, np.float32).reshape(n).copy()
    return a, a.ctypes.data_as(_FP)


def host_associate(bef, aft, total):
    """lins_host_map_associate -> transformTobeMapped (6,) f32"""
    L = _host.lib()
    L.lins_host_map_associate.argtypes, L.lins_host_map_associate.restype = [_FP] * 4, None
    (_, pb), (_, pa), (_, ps), (out, po) = _f6(bef), _f6(aft), _f6(total), _f6(np.zeros(6))
    L.lins_host_map_associate(pb, pa, ps, po)
    return out


def host_transform_update(tobe, has_imu, imu_roll, imu_pitch, total, bef, aft):
    """lins_host_map_transform_update -> (tobe, bef, aft) after the call"""
    L = _host.lib()
    L.lins_host_map_transform_update.argtypes = [_FP, C.c_int, C.c_float, C.c_float, _FP, _FP, _FP]
    L.lins_host_map_transform_update.restype = None
    (t, pt), (_, ps), (b, pb), (a, pa) = _f6(tobe), _f6(total), _f6(bef), _f6(aft)
    L.lins_host_map_transform_update(pt, int(bool(has_imu)), float(imu_roll), float(imu_pitch), ps, pb, pa)
    return t, b, a


def host_key_rule(prev, aft, have_frames):
    """lins_host_map_key_rule -> (save, prev after the call)"""
    L = _host.lib()
    L.lins_host_map_key_rule.argtypes, L.lins_host_map_key_rule.restype = [_FP, _FP, C.c_int], C.c_int
    (p, pp), (_, pa) = _f6(prev, 3), _f6(aft)
    save = L.lins_host_map_key_rule(pp, pa, int(bool(have_frames)))
    return int(save), p
