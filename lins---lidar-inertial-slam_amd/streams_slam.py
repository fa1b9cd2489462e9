"""Streams end to end (include/lins_streams_slam.h): the odometry records derived on the device from the streams' resident
globalState_, the mapping step that reads transformSum from them, the transform fusion node, and the one call per scan.
Functions over an ieskf.IeskfContext; the CPU restatement of the arithmetic is at the end (liblins_host.so,
include/lins_host.h lins_host_odom_from_global / lins_host_pose_quat / lins_host_fuse)."""
import ctypes as C

import numpy as np

from . import host as _host
from . import ieskf as _ieskf
from ._ctypes_defs import FusedPoseC, MapStepResultC, SlamImuC, StreamOdomC

_FP = C.POINTER(C.c_float)
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int32)


def slam_imu(roll=0.0, pitch=0.0, has_imu=False):
    return SlamImuC(float(roll), float(pitch), int(bool(has_imu)), 0)


def _imu_array(imu, n):
    if imu is None:
        return None
    assert len(imu) == n
    return (SlamImuC * max(n, 1))(*imu)


def odometry(ctx, download=True):
    """lins_streams_odometry: every stream's record from its resident globalState_ -> one dict per stream (position,
    orientation (x, y, z, w), transform_sum, valid), or None with download=False (the records stay resident)"""
    n = ctx._streams
    out = (StreamOdomC * n)()
    L = _ieskf.lib()
    L.lins_streams_odometry.argtypes = [C.c_void_p, C.c_void_p]
    ctx._check(L.lins_streams_odometry(ctx._h, out if download else None))
    return [out[k].as_dict() for k in range(n)] if download else None


def map_step_resident(ctx, streams, times, imu=None):
    """lins_streams_map_step_resident for the streams named; times: one per entry; imu: None or one slam_imu(...) per
    entry -> the per-entry result dicts (as streams_map.step)"""
    n = len(streams)
    sv = np.ascontiguousarray(streams, np.int32)
    tv = np.ascontiguousarray(times, np.float64).reshape(n)
    arr = _imu_array(imu, n)
    out = (MapStepResultC * max(n, 1))()
    L = _ieskf.lib()
    L.lins_streams_map_step_resident.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MapStepResultC)]
    ctx._check(L.lins_streams_map_step_resident(ctx._h, n, sv.ctypes.data, tv.ctypes.data, arr, out))
    return [out[k].as_dict() for k in range(n)]


def fuse(ctx, streams):
    """lins_streams_fuse: the transform fusion node for the streams named -> one dict(transform_mapped, orientation) each"""
    n = len(streams)
    sv = np.ascontiguousarray(streams, np.int32)
    out = (FusedPoseC * max(n, 1))()
    L = _ieskf.lib()
    L.lins_streams_fuse.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(FusedPoseC)]
    ctx._check(L.lins_streams_fuse(ctx._h, n, sv.ctypes.data, out))
    return [out[k].as_dict() for k in range(n)]


def slam_step(ctx, raws, imu, scan_time, scan_imu=None, scan_period=0.1, imu_rp=None):
    """lins_streams_slam_step: one scan of every stream.  raws / imu / scan_time / scan_imu as
    IeskfContext.streams_process_raw; imu_rp: None or one slam_imu(...) per stream.
    Returns (results, status (n,), map result dicts, fused pose dicts), each per stream."""
    n = ctx._streams
    assert len(raws) == n
    raws = [np.ascontiguousarray(r, dtype=np.float32).reshape(-1, 4) for r in raws]
    pp = C.POINTER(_host.Point)
    rptrs = (pp * n)(*[r.ctypes.data_as(pp) for r in raws])
    rcnt = (C.c_int32 * n)(*[len(r) for r in raws])
    cnt, ptrs, _keep = ctx._imu_args(imu)
    st = np.ascontiguousarray(scan_time, dtype=np.float64).reshape(n)
    si = None if scan_imu is None else np.ascontiguousarray(scan_imu, dtype=np.float64).reshape(n, 6)
    rp = _imu_array(imu_rp, n)
    res = (_ieskf.ResultC * n)()
    status = np.zeros(n, np.int32)
    mp = (MapStepResultC * n)()
    fz = (FusedPoseC * n)()
    L = _ieskf.lib()
    L.lins_streams_slam_step.argtypes = [C.c_void_p, C.POINTER(pp), _IP, _IP, C.POINTER(_DP), _DP, _DP, C.c_double, C.c_void_p,
                                         C.POINTER(_ieskf.ResultC), _IP, C.POINTER(MapStepResultC), C.POINTER(FusedPoseC)]
    rc = L.lins_streams_slam_step(ctx._h, rptrs, rcnt, cnt, ptrs, si.ctypes.data_as(_DP) if si is not None else _DP(), st.ctypes.data_as(_DP),
                                  float(scan_period), rp, res, status.ctypes.data_as(_IP), mp, fz)
    ctx._check(rc)
    ctx._n = 0
    return [_ieskf.Result(r) for r in res], status, [mp[k].as_dict() for k in range(n)], [fz[k].as_dict() for k in range(n)]


# ---- the CPU restatement (csrc/host/odom.cpp) --------------------------------------------------------------------
def host_odom_from_global(global_state):
    """lins_host_odom_from_global -> dict(position, orientation (x, y, z, w), transform_sum, valid)"""
    g = np.ascontiguousarray(global_state, np.float64).reshape(19)
    out = StreamOdomC()
    L = _host.lib()
    L.lins_host_odom_from_global.argtypes, L.lins_host_odom_from_global.restype = [_DP, C.POINTER(StreamOdomC)], None
    L.lins_host_odom_from_global(g.ctypes.data_as(_DP), C.byref(out))
    return out.as_dict()


def host_pose_quat(t6):
    """lins_host_pose_quat -> the published orientation (x, y, z, w) of a pose (rx, ry, rz, tx, ty, tz), f64"""
    t = np.array(t6, np.float32).reshape(6).copy()
    q = np.zeros(4)
    L = _host.lib()
    L.lins_host_pose_quat.argtypes, L.lins_host_pose_quat.restype = [_FP, _DP], None
    L.lins_host_pose_quat(t.ctypes.data_as(_FP), q.ctypes.data_as(_DP))
    return q


def host_fuse(bef, aft, total):
    """lins_host_fuse -> dict(transform_mapped, orientation)"""
    b, a, s = (np.array(v, np.float32).reshape(6).copy() for v in (bef, aft, total))
    out = FusedPoseC()
    L = _host.lib()
    L.lins_host_fuse.argtypes, L.lins_host_fuse.restype = [_FP, _FP, _FP, C.POINTER(FusedPoseC)], None
    L.lins_host_fuse(b.ctypes.data_as(_FP), a.ctypes.data_as(_FP), s.ctypes.data_as(_FP), C.byref(out))
    return out.as_dict()
