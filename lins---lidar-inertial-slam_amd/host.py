"""Bindings for liblins_host.so (pure-CPU host pieces, include/lins_host.h):
StatePredictor mirror, feature front-end, transformToEnd, synthetic scan pairs.
"""
import ctypes as C
import os

import numpy as np

from ._ctypes_defs import (CLOUD_MAX, ERR_DIM, MAX_QUERY, STATE_DIM, Point, ScanPair)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

SYNTH_SEED = 0x4C494E53  # "LINS"


class FilterParams(C.Structure):
    _fields_ = [
        ("acc_n", C.c_double), ("gyr_n", C.c_double), ("acc_w", C.c_double), ("gyr_w", C.c_double),
        ("init_pos_std", C.c_double * 3), ("init_vel_std", C.c_double * 3), ("init_att_std", C.c_double * 3),
        ("init_acc_std", C.c_double * 3), ("init_gyr_std", C.c_double * 3),
    ]


class Filter(C.Structure):
    _fields_ = [
        ("state", C.c_double * STATE_DIM),
        ("cov", C.c_double * (ERR_DIM * ERR_DIM)),
        ("noise", C.c_double * 144),
        ("acc_last", C.c_double * 3), ("gyr_last", C.c_double * 3),
        ("time", C.c_double),
        ("has_imu", C.c_int32), ("pad", C.c_int32),
        ("prm", FilterParams),
    ]


class BootParams(C.Structure):
    """lins_boot_params: the filter's parameters and INIT_BA / INIT_BW"""
    _fields_ = [("filter", FilterParams), ("init_ba", C.c_double * 3), ("init_bw", C.c_double * 3)]


class Preintegration(C.Structure):
    """lins_preintegration: the IMU pre-integration between a stream's first and second scan (delta_q: w x y z)"""
    _fields_ = [("sum_dt", C.c_double), ("delta_p", C.c_double * 3), ("delta_q", C.c_double * 4), ("delta_v", C.c_double * 3),
                ("acc_0", C.c_double * 3), ("gyr_0", C.c_double * 3)]

    def array(self):
        return np.frombuffer(bytes(self), np.float64).copy()


class Features(C.Structure):
    _fields_ = [
        ("corner_sharp", C.POINTER(Point)), ("n_corner_sharp", C.c_int32),
        ("corner_less_sharp", C.POINTER(Point)), ("n_corner_less_sharp", C.c_int32),
        ("surf_flat", C.POINTER(Point)), ("n_surf_flat", C.c_int32),
        ("surf_less_flat", C.POINTER(Point)), ("n_surf_less_flat", C.c_int32),
        ("n_segmented", C.c_int32), ("n_outlier", C.c_int32),
    ]


class SegmentedScanC(C.Structure):
    """lins_segmented_scan: segmented cloud + cloud_msgs/cloud_info (include/lins_host.h)."""
    _fields_ = [("cloud", C.POINTER(Point)), ("range", C.POINTER(C.c_float)), ("col", C.POINTER(C.c_uint32)),
                ("ground", C.POINTER(C.c_uint8)), ("n", C.c_int32), ("start_ring", C.c_int32 * 16),
                ("end_ring", C.c_int32 * 16), ("start_ori", C.c_float), ("end_ori", C.c_float),
                ("ori_diff", C.c_float), ("n_outlier", C.c_int32)]


class Segmented:
    """numpy-owned segmented scan; .c is the ctypes view (pointers into the arrays kept alive here)."""

    def __init__(self, cloud, rng, col, ground, c):
        self.cloud, self.range, self.col, self.ground, self.c = cloud, rng, col, ground, c

    @property
    def n(self):
        return self.c.n


def _features_buffers():
    cs, pcs = _buf(192)
    cls, pcls = _buf(1920)
    sf, psf = _buf(MAX_QUERY)
    slf, pslf = _buf(CLOUD_MAX)
    f = Features()
    f.corner_sharp, f.corner_less_sharp, f.surf_flat, f.surf_less_flat = pcs, pcls, psf, pslf
    return f, (cs, cls, sf, slf)


def _features_dict(f, bufs):
    cs, cls, sf, slf = bufs
    return dict(corner_sharp=cs[: f.n_corner_sharp].copy(), corner_less_sharp=cls[: f.n_corner_less_sharp].copy(),
                surf_flat=sf[: f.n_surf_flat].copy(), surf_less_flat=slf[: f.n_surf_less_flat].copy(),
                n_segmented=f.n_segmented, n_outlier=f.n_outlier)


def frontend_segment(raw):
    """image_projection_node on the host: raw cloud -> segmented scan (lins_frontend_segment)."""
    raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1, 4)
    cloud = np.zeros((CLOUD_MAX, 4), np.float32)
    rng = np.zeros(CLOUD_MAX, np.float32)
    col = np.zeros(CLOUD_MAX, np.uint32)
    ground = np.zeros(CLOUD_MAX, np.uint8)
    c = SegmentedScanC()
    L = lib()
    L.lins_frontend_segment.argtypes = [C.POINTER(Point), C.c_int, C.POINTER(Point), C.POINTER(C.c_float),
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(SegmentedScanC)]
    rc = L.lins_frontend_segment(raw.ctypes.data_as(C.POINTER(Point)), len(raw), cloud.ctypes.data_as(C.POINTER(Point)),
                                 rng.ctypes.data_as(C.POINTER(C.c_float)), col.ctypes.data_as(C.POINTER(C.c_uint32)),
                                 ground.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(c))
    if rc != 0:
        raise RuntimeError(f"lins_frontend_segment failed: {rc}")
    return Segmented(cloud, rng, col, ground, c)


def frontend_segment_outliers(raw):
    """image_projection_node's /outlier_cloud on the host (lins_frontend_segment_outliers): (n, 4) f32, raster order."""
    from ._ctypes_defs import OUTLIER_MAX

    raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1, 4)
    out = np.zeros((OUTLIER_MAX, 4), np.float32)
    L = lib()
    L.lins_frontend_segment_outliers.argtypes = [C.POINTER(Point), C.c_int, C.POINTER(Point)]
    L.lins_frontend_segment_outliers.restype = C.c_int
    rc = L.lins_frontend_segment_outliers(raw.ctypes.data_as(C.POINTER(Point)), len(raw), out.ctypes.data_as(C.POINTER(Point)))
    if rc < 0:
        raise RuntimeError(f"lins_frontend_segment_outliers failed: {rc}")
    return out[:rc].copy()


def segmented_from_arrays(cloud, rng, col, ground, n, start_ring, end_ring, orientation, n_outlier=0):
    """A Segmented (lins_segmented_scan view) over caller-provided arrays — e.g. another implementation's output."""
    cloud = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4)
    rng = np.ascontiguousarray(rng, dtype=np.float32)
    col = np.ascontiguousarray(col, dtype=np.uint32)
    ground = np.ascontiguousarray(ground, dtype=np.uint8)
    c = SegmentedScanC()
    c.cloud = cloud.ctypes.data_as(C.POINTER(Point))
    c.range = rng.ctypes.data_as(C.POINTER(C.c_float))
    c.col = col.ctypes.data_as(C.POINTER(C.c_uint32))
    c.ground = ground.ctypes.data_as(C.POINTER(C.c_uint8))
    c.n = int(n)
    for k in range(16):
        c.start_ring[k], c.end_ring[k] = int(start_ring[k]), int(end_ring[k])
    c.start_ori, c.end_ori, c.ori_diff = float(orientation[0]), float(orientation[1]), float(orientation[2])
    c.n_outlier = int(n_outlier)
    return Segmented(cloud, rng, col, ground, c)


def frontend_extract_segmented(seg, scan_period=0.1):
    """StateEstimator's feature stage on the host (the CPU restatement of the device front-end)."""
    f, bufs = _features_buffers()
    L = lib()
    L.lins_frontend_extract_segmented.argtypes = [C.POINTER(SegmentedScanC), C.c_double, C.POINTER(Features)]
    rc = L.lins_frontend_extract_segmented(C.byref(seg.c), scan_period, C.byref(f))
    if rc != 0:
        raise RuntimeError(f"lins_frontend_extract_segmented failed: {rc}")
    return _features_dict(f, bufs)


class SynthPairC(C.Structure):
    _fields_ = [
        ("surf_flat", C.POINTER(Point)), ("n_surf_flat", C.c_int32),
        ("corner_sharp", C.POINTER(Point)), ("n_corner_sharp", C.c_int32),
        ("surf_last", C.POINTER(Point)), ("n_surf_last", C.c_int32),
        ("corner_last", C.POINTER(Point)), ("n_corner_last", C.c_int32),
        ("state", C.c_double * STATE_DIM),
        ("cov", C.c_double * (ERR_DIM * ERR_DIM)),
        ("true_t", C.c_double * 3), ("true_q", C.c_double * 4),
        ("speed", C.c_double), ("yaw_rate", C.c_double),
        ("n_raw_last", C.c_int32), ("n_raw_new", C.c_int32),
    ]


def lib_path():
    return os.path.join(_HERE, "liblins_host.so")


def lib():
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise RuntimeError(f"{p} is missing — run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(p)
        L.lins_synth_generate.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(SynthPairC)]
        L.lins_synth_generate.restype = C.c_int
        L.lins_synth_raw_scan.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.POINTER(Point), C.c_int]
        L.lins_synth_raw_scan.restype = C.c_int
        L.lins_synth_generate_scene.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(SynthPairC)]
        L.lins_synth_generate_scene.restype = C.c_int
        L.lins_synth_raw_scan_scene.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(Point), C.c_int]
        L.lins_synth_raw_scan_scene.restype = C.c_int
        dp = C.POINTER(C.c_double)
        L.lins_synth_seq_raw_scan.argtypes = [C.c_uint32, C.c_int, C.POINTER(Point), C.c_int]
        L.lins_synth_seq_imu.argtypes = [C.c_uint32, C.c_int, dp, dp]
        L.lins_synth_seq_truth.argtypes = [C.c_uint32, C.c_double, dp, dp, dp]
        for f in (L.lins_synth_seq_raw_scan, L.lins_synth_seq_imu, L.lins_synth_seq_truth):
            f.restype = C.c_int
        L.lins_frontend_extract.argtypes = [C.POINTER(Point), C.c_int, C.c_double, C.POINTER(Features)]
        L.lins_frontend_extract.restype = C.c_int
        L.lins_transform_to_end.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                                            C.POINTER(Point), C.c_int, C.POINTER(Point)]
        L.lins_transform_to_end.restype = None
        L.lins_filter_default_params.argtypes = [C.POINTER(FilterParams)]
        L.lins_filter_init.argtypes = [C.POINTER(Filter), C.POINTER(FilterParams)] + [C.POINTER(C.c_double)] * 3
        L.lins_filter_predict.argtypes = [C.POINTER(Filter), C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.lins_filter_reset1.argtypes = [C.POINTER(Filter)]
        from ._ctypes_defs import ResultC

        L.lins_filter_finish.argtypes = [C.POINTER(Filter), C.POINTER(C.c_double), C.POINTER(ResultC), C.c_int]
        for f in (L.lins_filter_default_params, L.lins_filter_init, L.lins_filter_predict, L.lins_filter_reset1, L.lins_filter_finish):
            f.restype = None
        L.lins_boot_default_params.argtypes = [C.POINTER(BootParams)]
        L.lins_host_preintegrate.argtypes = [C.POINTER(Preintegration), C.c_int, dp, dp, dp]
        L.lins_host_boot_start.argtypes = [C.POINTER(Preintegration), dp, dp]
        L.lins_host_boot_first.argtypes = [C.POINTER(Filter), dp, dp, C.POINTER(Preintegration), dp, C.c_double, C.POINTER(BootParams)]
        L.lins_host_boot_second.argtypes = [C.POINTER(Filter), dp, dp, C.POINTER(Preintegration), dp, dp, dp, C.c_double,
                                            C.POINTER(BootParams)]
        for f in (L.lins_boot_default_params, L.lins_host_preintegrate, L.lins_host_boot_start, L.lins_host_boot_first, L.lins_host_boot_second):
            f.restype = None
        _LIB = L
    return _LIB


def filter_finish(filt, global_state, state, cov, used_prior_cov=False):
    """lins_filter_finish: filter_->update(state, cov) — the state only with used_prior_cov —, integrateTransformation,
    reset(1), correctRollPitch on `filt` (a Filter, changed in place).  Returns the new globalState_ (19,)."""
    from ._ctypes_defs import ResultC

    r = ResultC()
    r.state[:] = [float(v) for v in np.asarray(state, np.float64).reshape(19)]
    r.cov[:] = [float(v) for v in np.asarray(cov, np.float64).reshape(324)]
    g = np.array(global_state, dtype=np.float64).reshape(19).copy()
    lib().lins_filter_finish(C.byref(filt), g.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r), int(bool(used_prior_cov)))
    return g


# ---- the two-scan bootstrap (lins_host_preintegrate / lins_host_boot_*: csrc/host/boot.cpp) ----
def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def boot_default_params():
    p = BootParams()
    lib().lins_boot_default_params(C.byref(p))
    return p


def preintegrate(pre, rows, prm=None):
    """IntegrationBase::push_back of `rows` ((m, 7): dt, acc, gyr) onto `pre` (a Preintegration, changed in place)"""
    prm = prm or boot_default_params()
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 7)
    ba, bw = np.array(prm.init_ba[:]), np.array(prm.init_bw[:])
    lib().lins_host_preintegrate(C.byref(pre), len(rows), _dp(rows), _dp(ba), _dp(bw))
    return pre


def boot_start(pre):
    """-> (pl (3,), ql (4,) w x y z): the pose estimateTransform starts from (SE:392-396)"""
    t, q = np.zeros(3), np.zeros(4)
    lib().lins_host_boot_start(C.byref(pre), _dp(t), _dp(q))
    return t, q


def boot_first(imu_last, time, prm=None):
    """processFirstScan -> (Filter, linState_ (19,), Preintegration)"""
    prm = prm or boot_default_params()
    f, pre, lin, g = Filter(), Preintegration(), np.zeros(19), np.zeros(19)
    il = np.ascontiguousarray(imu_last, np.float64).reshape(6)
    lib().lins_host_boot_first(C.byref(f), _dp(g), _dp(lin), C.byref(pre), _dp(il), float(time), C.byref(prm))
    return f, lin, pre


def boot_second(pre, icp_t, icp_q, imu_last, time, prm=None):
    """processSecondScan behind estimateTransform -> (Filter, globalState_ (19,), linState_ (19,))"""
    prm = prm or boot_default_params()
    f, g, lin = Filter(), np.zeros(19), np.zeros(19)
    t, q = np.ascontiguousarray(icp_t, np.float64).reshape(3), np.ascontiguousarray(icp_q, np.float64).reshape(4)
    il = np.ascontiguousarray(imu_last, np.float64).reshape(6)
    lib().lins_host_boot_second(C.byref(f), _dp(g), _dp(lin), C.byref(pre), _dp(t), _dp(q), _dp(il), float(time), C.byref(prm))
    return f, g, lin


def local_map(frames, scan, window=50):
    """lins_host_local_map: the CPU restatement of lins_local_map_build for one entry.  frames: [(corner, surf, outlier,
    pose (x, y, z, roll, pitch, yaw))] oldest first (the last `window` are used); scan: (corner, surf, outlier) raw.
    Returns (the six clouds in LOCAL_* order, sizes dict)."""
    from ._ctypes_defs import KeyframeC, LocalMapSizesC, keyframe_c, local_scan_c

    L = lib()
    fr, keep = (KeyframeC * max(len(frames), 1))(), []
    for k, f in enumerate(frames):
        fr[k], kk = keyframe_c(*f)
        keep.append(kk)
    sc, skeep = local_scan_c(*scan)
    used = frames[max(0, len(frames) - window):]
    ncorner = sum(len(f[0]) for f in used)
    nsurf = sum(len(f[1]) + len(f[2]) for f in used)
    caps = [ncorner, nsurf, len(skeep[0]), len(skeep[1]), len(skeep[2]), len(skeep[1]) + len(skeep[2])]
    outs = [np.zeros((max(c, 1), 4), np.float32) for c in caps]
    ptrs = (C.POINTER(Point) * 6)(*[o.ctypes.data_as(C.POINTER(Point)) for o in outs])
    sizes = LocalMapSizesC()
    L.lins_host_local_map.argtypes = [C.POINTER(KeyframeC), C.c_int, C.c_int, C.POINTER(type(sc)), C.POINTER(C.POINTER(Point)),
                                      C.POINTER(LocalMapSizesC)]
    L.lins_host_local_map.restype = C.c_int
    rc = L.lins_host_local_map(fr, len(frames), int(window), C.byref(sc), ptrs, C.byref(sizes))
    if rc != 0:
        raise RuntimeError(f"lins_host_local_map: {rc}")
    d = sizes.as_dict()
    return [o[:n].copy() for o, n in zip(outs, d["n"])], d


def _key_poses(poses):
    from ._ctypes_defs import KeyPoseC, key_pose

    return (KeyPoseC * max(len(poses), 1))(*[key_pose(p) for p in poses])


def select_radius(poses, centre, radius, pose_leaf):
    """lins_host_select_radius: publishGlobalMap's choice of frames (LM:989-1007) among key poses (x, y, z, roll, pitch,
    yaw) by frame id -> the selected ids in the order the frames are visited"""
    from ._ctypes_defs import KeyPoseC

    L = lib()
    ids = np.zeros(max(len(poses), 1), np.int32)
    c = (C.c_float * 3)(*[float(v) for v in centre])
    L.lins_host_select_radius.argtypes = [C.POINTER(KeyPoseC), C.c_int, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_void_p, C.c_int]
    L.lins_host_select_radius.restype = C.c_int
    rc = L.lins_host_select_radius(_key_poses(poses), len(poses), c, float(radius), float(pose_leaf), ids.ctypes.data, len(poses))
    if rc < 0:
        raise RuntimeError(f"lins_host_select_radius: {rc}")
    return ids[:rc].copy()


def find_loop(poses, times, centre, radius, now, min_gap_s):
    """lins_host_find_loop: detectLoopClosure's candidate (LM:1050-1067) -> frame id or -1"""
    from ._ctypes_defs import KeyPoseC

    L = lib()
    t = np.ascontiguousarray(times, np.float64)
    c = (C.c_float * 3)(*[float(v) for v in centre])
    out = C.c_int32(-2)
    L.lins_host_find_loop.argtypes = [C.POINTER(KeyPoseC), C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_double, C.c_double,
                                      C.POINTER(C.c_int32)]
    L.lins_host_find_loop.restype = C.c_int
    rc = L.lins_host_find_loop(_key_poses(poses), t.ctypes.data, len(poses), c, float(radius), float(now), float(min_gap_s), C.byref(out))
    if rc != 0:
        raise RuntimeError(f"lins_host_find_loop: {rc}")
    return int(out.value)


def submap(frames, ids, clouds, leaf, flags=0):
    """lins_host_submap: the CPU restatement of one lins_archive_assemble spec.  frames: [(corner, surf, outlier, pose)]
    by frame id.  Returns (cloud (n, 4) f32, info dict)."""
    from ._ctypes_defs import KeyframeC, SubmapInfoC, keyframe_c

    L = lib()
    fr, keep = (KeyframeC * max(len(frames), 1))(), []
    for k, f in enumerate(frames):
        fr[k], kk = keyframe_c(*f)
        keep.append(kk)
    idv = np.ascontiguousarray(ids, np.int32)
    cap = sum(len(frames[i][q]) for i in idv if 0 <= i < len(frames) for q in range(3) if clouds & (1 << q) and clouds > 0)
    out = np.zeros((max(cap, 1), 4), np.float32)
    info = SubmapInfoC()
    L.lins_host_submap.argtypes = [C.POINTER(KeyframeC), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p,
                                   C.POINTER(SubmapInfoC)]
    L.lins_host_submap.restype = C.c_int
    rc = L.lins_host_submap(fr, len(frames), idv.ctypes.data, len(idv), int(clouds), float(leaf), int(flags), out.ctypes.data, C.byref(info))
    if rc != 0:
        raise RuntimeError(f"lins_host_submap: {rc}")
    d = info.as_dict()
    return out[:d["n"]].copy(), d


def surround_update(lst, ds, cap=None):
    """lins_host_surround_update: surroundingExistingKeyPosesID after one step with the loop closure off (LM:1261-1308)
    -> the new list; cap: the room of the caller's array (default: enough).  Raises MemoryError on LINS_E_CAPACITY."""
    L = lib()
    cap = len(lst) + len(ds) if cap is None else int(cap)
    buf = np.zeros(max(cap, len(lst), 1), np.int32)
    buf[:len(lst)] = lst
    dv = np.ascontiguousarray(ds, np.int32)
    L.lins_host_surround_update.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.lins_host_surround_update.restype = C.c_int
    rc = L.lins_host_surround_update(buf.ctypes.data, len(lst), cap, dv.ctypes.data, len(dv))
    if rc == -3:  # LINS_E_CAPACITY: the list is as it was
        assert buf[:len(lst)].tolist() == [int(v) for v in lst]
        raise MemoryError("lins_host_surround_update: LINS_E_CAPACITY")
    if rc < 0:
        raise RuntimeError(f"lins_host_surround_update: {rc}")
    return buf[:rc].tolist()


def surround_map(frames, lst, scan):
    """lins_host_surround_map: the CPU restatement of lins_local_map_build_surround for one entry.  frames: [(corner,
    surf, outlier, pose)] by frame id; lst: the listed ids; scan: (corner, surf, outlier) raw.  Returns (the six clouds in
    LOCAL_* order, sizes dict)."""
    from ._ctypes_defs import KeyframeC, LocalMapSizesC, keyframe_c, local_scan_c

    L = lib()
    fr, keep = (KeyframeC * max(len(frames), 1))(), []
    for k, f in enumerate(frames):
        fr[k], kk = keyframe_c(*f)
        keep.append(kk)
    sc, skeep = local_scan_c(*scan)
    idv = np.ascontiguousarray(lst, np.int32)
    used = [frames[i] for i in idv if 0 <= i < len(frames)]
    caps = [sum(len(f[0]) for f in used), sum(len(f[1]) + len(f[2]) for f in used), len(skeep[0]), len(skeep[1]), len(skeep[2]),
            len(skeep[1]) + len(skeep[2])]
    outs = [np.zeros((max(c, 1), 4), np.float32) for c in caps]
    ptrs = (C.POINTER(Point) * 6)(*[o.ctypes.data_as(C.POINTER(Point)) for o in outs])
    sizes = LocalMapSizesC()
    L.lins_host_surround_map.argtypes = [C.POINTER(KeyframeC), C.c_int, C.c_void_p, C.c_int, C.POINTER(type(sc)), C.POINTER(C.POINTER(Point)),
                                         C.POINTER(LocalMapSizesC)]
    L.lins_host_surround_map.restype = C.c_int
    rc = L.lins_host_surround_map(fr, len(frames), idv.ctypes.data, len(idv), C.byref(sc), ptrs, C.byref(sizes))
    if rc != 0:
        raise RuntimeError(f"lins_host_surround_map: {rc}")
    d = sizes.as_dict()
    return [o[:n].copy() for o, n in zip(outs, d["n"])], d


def loop_icp_params(**kw):
    """lins_loop_icp_default_params with fields overridden by keyword (max_iterations=3, ...)"""
    from ._ctypes_defs import loop_icp_params as f

    return f(lib(), **kw)


def _loop_clouds(source, target):
    from ._ctypes_defs import cloud

    s, t = cloud(source), cloud(target)
    return s, t, s.ctypes.data_as(C.POINTER(Point)), t.ctypes.data_as(C.POINTER(Point))


def loop_icp(source, target, params=None, max_rounds=0):
    """lins_host_loop_icp: the CPU restatement of one lins_loop_icp_batch problem (max_rounds: as
    lins_debug_loop_icp_rounds) -> result dict"""
    from ._ctypes_defs import LoopIcpParamsC, LoopIcpResultC

    L = lib()
    s, t, ps, pt = _loop_clouds(source, target)
    prm = params if params is not None else loop_icp_params()
    out = LoopIcpResultC()
    L.lins_host_loop_icp.argtypes = [C.POINTER(Point), C.c_int, C.POINTER(Point), C.c_int, C.POINTER(LoopIcpParamsC), C.c_int, C.POINTER(LoopIcpResultC)]
    L.lins_host_loop_icp.restype = C.c_int
    rc = L.lins_host_loop_icp(ps, len(s), pt, len(t), C.byref(prm), int(max_rounds), C.byref(out))
    if rc != 0:
        raise RuntimeError(f"lins_host_loop_icp: {rc}")
    return out.as_dict()


def loop_icp_from(source, target, T0, params=None, max_rounds=0):
    """lins_host_loop_icp_from: loop_icp started from T0 (4 x 4) -> result dict, or the C return code of a refusal"""
    from ._ctypes_defs import LoopIcpParamsC, LoopIcpResultC

    L = lib()
    s, t, ps, pt = _loop_clouds(source, target)
    prm = params if params is not None else loop_icp_params()
    out = LoopIcpResultC()
    T = np.ascontiguousarray(T0, np.float64).reshape(16)
    L.lins_host_loop_icp_from.argtypes = [C.POINTER(Point), C.c_int, C.POINTER(Point), C.c_int, C.c_void_p, C.POINTER(LoopIcpParamsC), C.c_int,
                                          C.POINTER(LoopIcpResultC)]
    L.lins_host_loop_icp_from.restype = C.c_int
    rc = L.lins_host_loop_icp_from(ps, len(s), pt, len(t), T.ctypes.data, C.byref(prm), int(max_rounds), C.byref(out))
    return out.as_dict() if rc == 0 else rc


# ---- place recognition (include/lins_host.h lins_host_place_*: the definition the device is held to) ----
def place_params(**kw):
    from ._ctypes_defs import place_params as f

    return f(lib(), **kw)


def place_descriptor(corner, surf, outlier, params=None):
    """lins_host_place_descriptor -> D[ring][sector], (20, 60) f32"""
    from ._ctypes_defs import KeyframeC, PlaceParamsC, keyframe_c

    L = lib()
    f, _keep = keyframe_c(corner, surf, outlier, (0, 0, 0, 0, 0, 0))
    prm = params if params is not None else place_params()
    out = np.zeros((20, 60), np.float32)
    L.lins_host_place_descriptor.argtypes = [C.POINTER(KeyframeC), C.POINTER(PlaceParamsC), C.c_void_p]
    L.lins_host_place_descriptor.restype = C.c_int
    rc = L.lins_host_place_descriptor(C.byref(f), C.byref(prm), out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"lins_host_place_descriptor: {rc}")
    return out


def place_distance(query, candidate):
    """lins_host_place_distance: one pair of descriptors -> d[shift], 60 f32"""
    L = lib()
    q, c = np.ascontiguousarray(query, np.float32).reshape(1200), np.ascontiguousarray(candidate, np.float32).reshape(1200)
    d = np.zeros(60, np.float32)
    L.lins_host_place_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lins_host_place_distance.restype = C.c_int
    rc = L.lins_host_place_distance(q.ctypes.data, c.ctypes.data, d.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"lins_host_place_distance: {rc}")
    return d


def place_search(query, descs, times, now, min_gap_s, skip_id=-1):
    """lins_host_place_search -> dict(id, shift, distance (np.float32), candidates), or the C return code of a refusal"""
    L = lib()
    q = np.ascontiguousarray(query, np.float32).reshape(1200)
    n = len(descs)
    D = np.ascontiguousarray(descs, np.float32).reshape(max(n, 1) if n else 0, 1200) if n else np.zeros((1, 1200), np.float32)
    t = np.ascontiguousarray(times, np.float64) if n else np.zeros(1)
    i, k, d, c = C.c_int32(-2), C.c_int32(-2), C.c_float(0), C.c_int32(0)
    L.lins_host_place_search.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    L.lins_host_place_search.restype = C.c_int
    rc = L.lins_host_place_search(q.ctypes.data, D.ctypes.data, t.ctypes.data, n, int(skip_id), float(now), float(min_gap_s), C.byref(i), C.byref(k),
                                  C.byref(d), C.byref(c))
    if rc != 0:
        return rc
    return dict(id=int(i.value), shift=int(k.value), distance=np.float32(d.value), candidates=int(c.value))


def place_topk(query, descs, times, now, min_gap_s, k, min_sep, skip_id=-1, raw=False):
    """lins_host_place_topk -> (the filled ranks' dicts (id, shift, distance (np.float32)), candidates), or the C return
    code (a negative int) of a refusal.  raw: all k ranks, the unfilled ones as the call leaves them."""
    L = lib()
    q = np.ascontiguousarray(query, np.float32).reshape(1200)
    n = len(descs)
    D = np.ascontiguousarray(descs, np.float32).reshape(n, 1200) if n else np.zeros((1, 1200), np.float32)
    t = np.ascontiguousarray(times, np.float64) if n else np.zeros(1)
    kk = max(int(k), 1)
    ids, sh, d, c = np.full(kk, -2, np.int32), np.full(kk, -2, np.int32), np.zeros(kk, np.float32), C.c_int32(0)
    L.lins_host_place_topk.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    L.lins_host_place_topk.restype = C.c_int
    rc = L.lins_host_place_topk(q.ctypes.data, D.ctypes.data, t.ctypes.data, n, int(skip_id), float(now), float(min_gap_s), int(k), int(min_sep),
                                ids.ctypes.data, sh.ctypes.data, d.ctypes.data, C.byref(c))
    if rc < 0:
        return rc
    return [dict(id=int(ids[j]), shift=int(sh[j]), distance=np.float32(d[j])) for j in range(kk if raw else rc)], int(c.value)


def loop_choose(converged, fitness, max_fitness=0.3):
    """lins_host_loop_choose: the rank of the smallest accepted fitness (the lower rank at a tie), -1: none accepted"""
    L = lib()
    cv, ft = np.ascontiguousarray(converged, np.int32), np.ascontiguousarray(fitness, np.float64)
    assert len(cv) == len(ft)
    L.lins_host_loop_choose.argtypes, L.lins_host_loop_choose.restype = [C.c_int, C.c_void_p, C.c_void_p, C.c_float], C.c_int
    return int(L.lins_host_loop_choose(len(cv), cv.ctypes.data if len(cv) else None, ft.ctypes.data if len(ft) else None, float(max_fitness)))


def rendezvous_consensus(hyps, n_hyp=None, **kw):
    """lins_host_rendezvous_consensus: the definition of the consensus rule of a rendezvous over a window.  hyps: a list of
    dicts (X 4 x 4 f64, p (3,), fitness, query, rank, target_slot, admissible) or a ConsensusHypC array (then n_hyp says how
    many count); kw: fields of lins_consensus_params (max_translation=, min_cos_rotation=).  Returns dict(winner, support,
    n_admissible, members (ascending indices)), or the C return code (a negative int) of a refusal."""
    from ._ctypes_defs import ConsensusHypC, ConsensusParamsC, ConsensusResultC, consensus_params, consensus_table

    L = lib()
    arr = consensus_table(hyps) if isinstance(hyps, (list, tuple)) else hyps
    n = len(hyps) if n_hyp is None else int(n_hyp)
    prm, out = consensus_params(L, **kw), ConsensusResultC()
    L.lins_host_rendezvous_consensus.argtypes = [C.POINTER(ConsensusHypC), C.c_int, C.POINTER(ConsensusParamsC), C.POINTER(ConsensusResultC)]
    L.lins_host_rendezvous_consensus.restype = C.c_int
    rc = L.lins_host_rendezvous_consensus(arr, n, C.byref(prm), C.byref(out))
    return out.as_dict() if rc == 0 else rc


def place_guess(pose_q, pose_c, shift, up_axis=1):
    """lins_host_place_guess -> T0 (4 x 4 f64), or the C return code of a refusal"""
    from ._ctypes_defs import KeyPoseC, key_pose

    L = lib()
    T = np.zeros(16, np.float64)
    pq, pc = key_pose(pose_q), key_pose(pose_c)
    L.lins_host_place_guess.argtypes = [C.POINTER(KeyPoseC), C.POINTER(KeyPoseC), C.c_int, C.c_int, C.c_void_p]
    L.lins_host_place_guess.restype = C.c_int
    rc = L.lins_host_place_guess(C.byref(pq), C.byref(pc), int(shift), int(up_axis), T.ctypes.data)
    return T.reshape(4, 4) if rc == 0 else rc


def loop_icp_trace(source, target, params=None):
    """lins_host_loop_icp_trace -> (rounds: list of dicts (T_in, n_corr, mse, delta, T_out, stop, reason), result dict)"""
    from ._ctypes_defs import LoopIcpParamsC, LoopIcpResultC, LoopIcpRoundC

    L = lib()
    s, t, ps, pt = _loop_clouds(source, target)
    prm = params if params is not None else loop_icp_params()
    cap = max(int(prm.max_iterations), 1)
    rounds, out = (LoopIcpRoundC * cap)(), LoopIcpResultC()
    L.lins_host_loop_icp_trace.argtypes = [C.POINTER(Point), C.c_int, C.POINTER(Point), C.c_int, C.POINTER(LoopIcpParamsC), C.POINTER(LoopIcpRoundC),
                                           C.c_int, C.POINTER(LoopIcpResultC)]
    L.lins_host_loop_icp_trace.restype = C.c_int
    n = L.lins_host_loop_icp_trace(ps, len(s), pt, len(t), C.byref(prm), rounds, cap, C.byref(out))
    if n < 0:
        raise RuntimeError(f"lins_host_loop_icp_trace: {n}")
    return [rounds[k].as_dict() for k in range(n)], out.as_dict()


def loop_icp_correspondences(source, target, T, cap=0.0):
    """lins_host_loop_icp_correspondences: the move + EXHAUSTIVE search at T -> (idx (-1: none), d)"""
    L = lib()
    s, t, ps, pt = _loop_clouds(source, target)
    idx, d = np.full(max(len(s), 1), -2, np.int32), np.zeros(max(len(s), 1), np.float32)
    Tm = np.ascontiguousarray(T, np.float64).reshape(16)
    L.lins_host_loop_icp_correspondences.argtypes = [C.POINTER(Point), C.c_int, C.POINTER(Point), C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    L.lins_host_loop_icp_correspondences.restype = C.c_int
    rc = L.lins_host_loop_icp_correspondences(ps, len(s), pt, len(t), Tm.ctypes.data, float(cap), idx.ctypes.data, d.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"lins_host_loop_icp_correspondences: {rc}")
    return idx[:len(s)].copy(), d[:len(s)].copy()


def loop_icp_step(sums, params=None, mode=0, state=None):
    """lins_host_loop_icp_step: steps 3-6 of one round (mode 0) or the fitness score (mode 1) from the 17 sums; state: a
    dict of lins_loop_icp_state fields over a fresh problem -> (state dict, delta (4, 4), stop (4))"""
    from ._ctypes_defs import LoopIcpParamsC, LoopIcpStateC, loop_icp_state

    L = lib()
    v = np.ascontiguousarray(sums, np.float64).reshape(17)
    prm = params if params is not None else loop_icp_params()
    st, D, q = loop_icp_state(state), np.full(16, np.nan), np.full(4, np.nan)
    L.lins_host_loop_icp_step.argtypes = [C.c_void_p, C.POINTER(LoopIcpParamsC), C.c_int, C.POINTER(LoopIcpStateC), C.c_void_p, C.c_void_p]
    L.lins_host_loop_icp_step.restype = C.c_int
    rc = L.lins_host_loop_icp_step(v.ctypes.data, C.byref(prm), int(mode), C.byref(st), D.ctypes.data, q.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"lins_host_loop_icp_step: {rc}")
    return st.as_dict(), D.reshape(4, 4), q


def loop_pose_from(T, wrong):
    """lins_host_loop_pose_from (LM:1156-1166, f32): the ICP's T and the latest key pose (x, y, z, roll, pitch, yaw) ->
    the corrected pose the factor graph's BetweenFactor starts from, same field order"""
    from ._ctypes_defs import KeyPoseC, key_pose

    L = lib()
    Tm = np.ascontiguousarray(T, np.float64).reshape(16)
    w, out = key_pose(wrong), KeyPoseC()
    L.lins_host_loop_pose_from.argtypes = [C.c_void_p, C.POINTER(KeyPoseC), C.POINTER(KeyPoseC)]
    L.lins_host_loop_pose_from.restype = C.c_int
    rc = L.lins_host_loop_pose_from(Tm.ctypes.data, C.byref(w), C.byref(out))
    if rc != 0:
        raise RuntimeError(f"lins_host_loop_pose_from: {rc}")
    return np.array([out.x, out.y, out.z, out.roll, out.pitch, out.yaw], np.float32)


def loop_window(latest, closest, search_num):
    """lins_host_loop_window (LM:1087-1098): the ids closest - search_num .. closest + search_num clipped to [0, latest]"""
    L = lib()
    cap = max(int(latest) + 1, 1)
    ids = np.zeros(cap, np.int32)
    L.lins_host_loop_window.argtypes, L.lins_host_loop_window.restype = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int], C.c_int
    n = L.lins_host_loop_window(int(latest), int(closest), int(search_num), ids.ctypes.data, cap)
    if n < 0:
        raise RuntimeError(f"lins_host_loop_window: {n}")
    return ids[:n].tolist()


def loop_candidate(latest, closest, last_latest=-1, last_closest=-1):
    """lins_host_loop_candidate: LOOP_NONE (no candidate, or the latest frame itself), LOOP_REPEAT (the pair of the slot's
    most recent loop factor), or -1: the pair is aligned"""
    L = lib()
    L.lins_host_loop_candidate.argtypes, L.lins_host_loop_candidate.restype = [C.c_int] * 4, C.c_int
    return int(L.lins_host_loop_candidate(int(latest), int(closest), int(last_latest), int(last_closest)))


def loop_accept(converged, fitness, max_fitness=0.3):
    """lins_host_loop_accept (LM:1140-1141): converged && !(fitness > (double)(float)max_fitness)"""
    L = lib()
    L.lins_host_loop_accept.argtypes, L.lins_host_loop_accept.restype = [C.c_int, C.c_double, C.c_float], C.c_int
    return bool(L.lins_host_loop_accept(int(converged), float(fitness), float(max_fitness)))


def loop_variance(fitness):
    """lins_host_loop_variance (LM:1171-1175) -> (usable, (double)(float)fitness)"""
    L, v = lib(), C.c_double(0)
    L.lins_host_loop_variance.argtypes, L.lins_host_loop_variance.restype = [C.c_double, C.POINTER(C.c_double)], C.c_int
    ok = L.lins_host_loop_variance(float(fitness), C.byref(v))
    return bool(ok), float(v.value)


def arena_reclaim_plan(blocks, chunk):
    """lins_host_arena_reclaim_plan (csrc/host/arena_reclaim.h): the compaction of an arena whose blocks are the tuples
    (offset, points, keep) in ascending offset order, in passes of at most `chunk` points.  Returns the passes, each a
    dict(direct=bool, segments=[(src, dst, n), ...]) with its segments in arena order."""
    from ._ctypes_defs import ArenaBlockC, ArenaSegmentC

    L = lib()
    n = len(blocks)
    arr = (ArenaBlockC * max(n, 1))(*[ArenaBlockC(int(o), int(c), int(bool(k)), 0) for o, c, k in blocks])
    L.lins_host_arena_reclaim_plan.argtypes = [C.c_int, C.POINTER(ArenaBlockC), C.c_longlong, C.POINTER(ArenaSegmentC), C.c_longlong,
                                               C.POINTER(C.c_int32)]
    L.lins_host_arena_reclaim_plan.restype = C.c_longlong
    np_ = C.c_int32(0)
    cnt = L.lins_host_arena_reclaim_plan(n, arr, int(chunk), None, 0, C.byref(np_))
    if cnt < 0:
        raise RuntimeError(f"lins_host_arena_reclaim_plan: {cnt}")
    segs = (ArenaSegmentC * max(cnt, 1))()
    got = L.lins_host_arena_reclaim_plan(n, arr, int(chunk), segs, cnt, C.byref(np_))
    assert got == cnt
    passes = [dict(direct=None, segments=[]) for _ in range(np_.value)]
    for i in range(cnt):
        g = segs[i]
        p = passes[g.pass_]
        assert p["direct"] in (None, bool(g.direct))  # (one flag per pass)
        p["direct"] = bool(g.direct)
        p["segments"].append((int(g.src), int(g.dst), int(g.n)))
    return passes


def snapshot_info(blob):
    """lins_host_snapshot_info (csrc/host/snapshot_format.h): the header of a stream snapshot's blob (bytes) as a dict
    after the whole format check — no device needed; RuntimeError with the code when the blob is refused"""
    from ._ctypes_defs import SnapshotInfoC

    L = lib()
    buf = np.frombuffer(blob, np.uint8)
    out = SnapshotInfoC()
    L.lins_host_snapshot_info.argtypes, L.lins_host_snapshot_info.restype = [C.c_void_p, C.c_uint64, C.POINTER(SnapshotInfoC)], C.c_int
    rc = L.lins_host_snapshot_info(buf.ctypes.data if len(buf) else None, len(buf), C.byref(out))
    if rc != 0:
        raise RuntimeError(f"lins_host_snapshot_info: {rc}")
    return out.as_dict()


def _buf(n):
    a = np.zeros((n, 4), dtype=np.float32)
    return a, a.ctypes.data_as(C.POINTER(Point))


def synth_pair(index, seed=SYNTH_SEED, scene=0):
    """Seeded synthetic scan pair `index` as a ScanPair.  scene: 0 = the room, 1 = the open scene family
    (trunks, far wall segments, lost returns, a moving box: csrc/host/synth.cpp)."""
    sf, psf = _buf(MAX_QUERY)
    cs, pcs = _buf(MAX_QUERY)
    sl, psl = _buf(CLOUD_MAX)
    cl, pcl = _buf(1920)
    sp = SynthPairC()
    sp.surf_flat, sp.corner_sharp, sp.surf_last, sp.corner_last = psf, pcs, psl, pcl
    rc = lib().lins_synth_generate_scene(scene, seed, index, C.byref(sp))
    if rc != 0:
        raise RuntimeError(f"lins_synth_generate_scene({scene}) failed: {rc}")
    meta = dict(true_t=np.array(sp.true_t[:]), true_q=np.array(sp.true_q[:]), speed=sp.speed,
                yaw_rate=sp.yaw_rate, n_raw=(sp.n_raw_last, sp.n_raw_new), index=index, seed=seed, scene=scene)
    return ScanPair(sf[: sp.n_surf_flat].copy(), cs[: sp.n_corner_sharp].copy(), sl[: sp.n_surf_last].copy(),
                    cl[: sp.n_corner_last].copy(), np.array(sp.state[:]), np.array(sp.cov[:]), meta)


def synth_batch(n, start=0, seed=SYNTH_SEED, scene=0):
    return [synth_pair(start + i, seed, scene) for i in range(n)]


def synth_raw_scan(index, k, seed=SYNTH_SEED, scene=0):
    a, p = _buf(CLOUD_MAX)
    n = lib().lins_synth_raw_scan_scene(scene, seed, index, k, p, CLOUD_MAX)
    if n < 0:
        raise RuntimeError(f"lins_synth_raw_scan failed: {n}")
    return a[:n].copy()


def synth_seq_raw_scan(seq, k):
    """Raw cloud (firing order) of sweep k of the seeded scan SEQUENCE `seq` (one trajectory: lins_synth_seq_raw_scan)."""
    a, p = _buf(CLOUD_MAX)
    n = lib().lins_synth_seq_raw_scan(seq, k, p, CLOUD_MAX)
    if n < 0:
        raise RuntimeError(f"lins_synth_seq_raw_scan failed: {n}")
    return a[:n].copy()


def synth_seq_imu(seq, k):
    """(acc, gyr): the 40 IMU samples (400 Hz) of sweep k of sequence `seq`, each 40 x 3."""
    acc, gyr = np.zeros((40, 3)), np.zeros((40, 3))
    dp = C.POINTER(C.c_double)
    n = lib().lins_synth_seq_imu(seq, k, acc.ctypes.data_as(dp), gyr.ctypes.data_as(dp))
    if n != 40:
        raise RuntimeError(f"lins_synth_seq_imu failed: {n}")
    return acc, gyr


def synth_seq_truth(seq, tau):
    """(x, y, yaw, speed, yaw_rate) of the sensor at time tau [s] since the start of sweep 0."""
    xyy, v, w = np.zeros(3), C.c_double(0), C.c_double(0)
    rc = lib().lins_synth_seq_truth(seq, tau, xyy.ctypes.data_as(C.POINTER(C.c_double)), C.byref(v), C.byref(w))
    if rc != 0:
        raise RuntimeError(f"lins_synth_seq_truth failed: {rc}")
    return xyy[0], xyy[1], xyy[2], v.value, w.value


def frontend_extract(raw, scan_period=0.1):
    raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1, 4)
    cs, pcs = _buf(192)
    cls, pcls = _buf(1920)
    sf, psf = _buf(MAX_QUERY)
    slf, pslf = _buf(CLOUD_MAX)
    f = Features()
    f.corner_sharp, f.corner_less_sharp, f.surf_flat, f.surf_less_flat = pcs, pcls, psf, pslf
    rc = lib().lins_frontend_extract(raw.ctypes.data_as(C.POINTER(Point)), len(raw), scan_period, C.byref(f))
    if rc != 0:
        raise RuntimeError(f"lins_frontend_extract failed: {rc}")
    return dict(corner_sharp=cs[: f.n_corner_sharp].copy(), corner_less_sharp=cls[: f.n_corner_less_sharp].copy(),
                surf_flat=sf[: f.n_surf_flat].copy(), surf_less_flat=slf[: f.n_surf_less_flat].copy(),
                n_segmented=f.n_segmented, n_outlier=f.n_outlier)


def transform_to_end(t, q, pts, scan_period=0.1):
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 4)
    out = np.empty_like(pts)
    t = (C.c_double * 3)(*t)
    q = (C.c_double * 4)(*q)
    lib().lins_transform_to_end(t, q, scan_period, pts.ctypes.data_as(C.POINTER(Point)), len(pts),
                                out.ctypes.data_as(C.POINTER(Point)))
    return out


# ---- the pose graph on the CPU (include/lins_host.h lins_host_pose_graph_*) ----------------------
def pose_graph_params(**kw):
    """lins_pose_graph_default_params with fields overridden by keyword (max_iterations=3, ...)"""
    from ._ctypes_defs import pose_graph_params as f

    return f(lib(), **kw)


def pose_from6(p):
    """six floats (pitch, yaw, roll, y, z, x) -> pose (12 doubles: R row-major, t)"""
    from ._ctypes_defs import six_floats

    L, T = lib(), np.zeros(12)
    L.lins_host_pose_from6.argtypes, L.lins_host_pose_from6.restype = [C.POINTER(C.c_float), C.c_void_p], None
    L.lins_host_pose_from6(six_floats(p), T.ctypes.data)
    return T


def pose_to6(T):
    """pose (12 doubles) -> six floats, rounded once"""
    L, Tm, out = lib(), np.ascontiguousarray(T, dtype=np.float64).reshape(12), np.zeros(6, np.float32)
    L.lins_host_pose_to6.argtypes, L.lins_host_pose_to6.restype = [C.c_void_p, C.c_void_p], None
    L.lins_host_pose_to6(Tm.ctypes.data, out.ctypes.data)
    return out


class PoseGraph:
    """lins_host_pose_graph: the CPU restatement of one slot's pose graph.  Calls return the C return code where it can be
    an error the tests look at (push, add_loop); the others raise."""

    def __init__(self, max_frames, max_loops):
        L = lib()
        L.lins_host_pose_graph_create.argtypes, L.lins_host_pose_graph_create.restype = [C.c_int, C.c_int], C.c_void_p
        self._h = L.lins_host_pose_graph_create(int(max_frames), int(max_loops))
        if not self._h:
            raise RuntimeError("lins_host_pose_graph_create")

    def close(self):
        if self._h:
            L = lib()
            L.lins_host_pose_graph_destroy.argtypes, L.lins_host_pose_graph_destroy.restype = [C.c_void_p], None
            L.lins_host_pose_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def push(self, last6, aft6):
        """returns the frame id (>= 0) or the error code"""
        from ._ctypes_defs import six_floats

        L = lib()
        L.lins_host_pose_graph_push.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.lins_host_pose_graph_push.restype = C.c_int
        return L.lins_host_pose_graph_push(self._h, six_floats(last6) if last6 is not None else None, six_floats(aft6))

    def add_loop(self, latest_id, closest_id, pose_from, fitness):
        """pose_from: (x, y, z, roll, pitch, yaw) as loop_pose_from returns it; returns the C return code"""
        from ._ctypes_defs import KeyPoseC, key_pose

        L = lib()
        L.lins_host_pose_graph_add_loop.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(KeyPoseC), C.c_double]
        L.lins_host_pose_graph_add_loop.restype = C.c_int
        p = key_pose(pose_from)
        return L.lins_host_pose_graph_add_loop(self._h, int(latest_id), int(closest_id), C.byref(p), float(fitness))

    def count(self):
        """(frames, loops)"""
        L, nl = lib(), C.c_int32(0)
        L.lins_host_pose_graph_count.argtypes, L.lins_host_pose_graph_count.restype = [C.c_void_p, C.POINTER(C.c_int32)], C.c_int
        n = L.lins_host_pose_graph_count(self._h, C.byref(nl))
        return n, int(nl.value)

    def rebase(self, X):
        """lins_host_pose_graph_rebase: the history moves into the frame X (4 x 4 f64, the archive's axes) -> the C return code"""
        L = lib()
        x = np.ascontiguousarray(X, np.float64).reshape(16)
        L.lins_host_pose_graph_rebase.argtypes, L.lins_host_pose_graph_rebase.restype = [C.c_void_p, C.c_void_p], C.c_int
        return L.lins_host_pose_graph_rebase(self._h, x.ctypes.data)

    def solve(self, params=None):
        from ._ctypes_defs import PoseGraphParamsC, PoseGraphResultC

        L, out = lib(), PoseGraphResultC()
        prm = params if params is not None else pose_graph_params()
        L.lins_host_pose_graph_solve.argtypes = [C.c_void_p, C.POINTER(PoseGraphParamsC), C.POINTER(PoseGraphResultC)]
        L.lins_host_pose_graph_solve.restype = C.c_int
        rc = L.lins_host_pose_graph_solve(self._h, C.byref(prm), C.byref(out))
        if rc:
            raise RuntimeError(f"lins_host_pose_graph_solve: {rc}")
        return out.as_dict()

    def poses(self, first_id=0, n=None):
        """(n, 6) f32: x, y, z, roll, pitch, yaw (PointTypePose)"""
        from ._ctypes_defs import KeyPoseC

        L = lib()
        n = self.count()[0] - first_id if n is None else n
        out = np.zeros((max(n, 1), 6), np.float32)
        L.lins_host_pose_graph_poses.argtypes, L.lins_host_pose_graph_poses.restype = [C.c_void_p, C.c_int, C.c_int, C.c_void_p], C.c_int
        rc = L.lins_host_pose_graph_poses(self._h, int(first_id), int(n), out.ctypes.data)
        if rc:
            raise RuntimeError(f"lins_host_pose_graph_poses: {rc}")
        return out[:n]

    def poses_f64(self, first_id=0, n=None):
        """(n, 12) f64: R row-major, t"""
        L = lib()
        n = self.count()[0] - first_id if n is None else n
        out = np.zeros((max(n, 1), 12))
        L.lins_host_pose_graph_poses_f64.argtypes, L.lins_host_pose_graph_poses_f64.restype = [C.c_void_p, C.c_int, C.c_int, C.c_void_p], C.c_int
        rc = L.lins_host_pose_graph_poses_f64(self._h, int(first_id), int(n), out.ctypes.data)
        if rc:
            raise RuntimeError(f"lins_host_pose_graph_poses_f64: {rc}")
        return out[:n]

    def loop_z(self, loop):
        L, z = lib(), np.zeros(12)
        L.lins_host_pose_graph_loop_z.argtypes, L.lins_host_pose_graph_loop_z.restype = [C.c_void_p, C.c_int, C.c_void_p], C.c_int
        rc = L.lins_host_pose_graph_loop_z(self._h, int(loop), z.ctypes.data)
        if rc:
            raise RuntimeError(f"lins_host_pose_graph_loop_z: {rc}")
        return z

    def linearize(self, poses=None):
        """the linearisation at absolute poses (N, 12) (None: the estimate) -> dict r_odo (N-1, 6), D (N-1, 6, 6), g (N-1, 6),
        r_loop (L, 6), M (L, 6, 6)"""
        L = lib()
        n, nl = self.count()
        T = None if poses is None else np.ascontiguousarray(poses, dtype=np.float64).reshape(n, 12)
        m = max(n - 1, 1)
        r, D, g, rl, M = np.zeros((m, 6)), np.zeros((m, 6, 6)), np.zeros((m, 6)), np.zeros((max(nl, 1), 6)), np.zeros((max(nl, 1), 6, 6))
        L.lins_host_pose_graph_linearize.argtypes = [C.c_void_p] * 7
        L.lins_host_pose_graph_linearize.restype = C.c_int
        rc = L.lins_host_pose_graph_linearize(self._h, T.ctypes.data if T is not None else None, r.ctypes.data, D.ctypes.data, g.ctypes.data,
                                              rl.ctypes.data, M.ctypes.data)
        if rc:
            raise RuntimeError(f"lins_host_pose_graph_linearize: {rc}")
        return dict(r_odo=r[:n - 1], D=D[:n - 1], g=g[:n - 1], r_loop=rl[:nl], M=M[:nl])


# ---- the team graph on the CPU (include/lins_host.h lins_host_team_*) ----------------------------
TEAM_ROOT_VARIANCE = (1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6)  # the odometry factor's, rotation first


def team_factor(Tb, Ta, X=None, fitness=1.0):
    """lins_host_team_factor: Z = (X Tb)^-1 Ta of two poses (12 doubles each; X: 4 x 4 f64 in the archive's axes, None: the
    identity) -> a TeamFactorC with zero slots and ids, or the C return code of a refused call"""
    from ._ctypes_defs import TeamFactorC

    L, out = lib(), TeamFactorC()
    b, a = np.ascontiguousarray(Tb, np.float64).reshape(12), np.ascontiguousarray(Ta, np.float64).reshape(12)
    x = None if X is None else np.ascontiguousarray(X, np.float64).reshape(16)
    L.lins_host_team_factor.argtypes, L.lins_host_team_factor.restype = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(TeamFactorC)], C.c_int
    rc = L.lins_host_team_factor(b.ctypes.data, a.ctypes.data, x.ctypes.data if x is not None else None, float(fitness), C.byref(out))
    return rc if rc else out


def _team_args(graphs, factors, root_variance):
    from ._ctypes_defs import TeamFactorC, team_factor as rec

    n = len(graphs)
    hs = (C.c_void_p * max(n, 1))(*[g._h for g in graphs])
    rv = np.ascontiguousarray(np.broadcast_to(np.asarray(TEAM_ROOT_VARIANCE if root_variance is None else root_variance, np.float64), (max(n, 1), 6)))
    fac = [rec(f) for f in factors]
    farr = (TeamFactorC * max(len(fac), 1))(*fac)
    return n, hs, rv, len(fac), farr


def team_graph_solve(graphs, factors=(), params=None, root_variance=None):
    """lins_host_team_graph_solve of ONE group: graphs[0] (PoseGraph objects) is the anchor; a factor's slots are member
    indices; root_variance: six variances, or (members, 6).  Returns the result dict, or the C return code of a refused call."""
    from ._ctypes_defs import PoseGraphParamsC, TeamFactorC, TeamGraphResultC

    L, out = lib(), TeamGraphResultC()
    prm = params if params is not None else pose_graph_params()
    n, hs, rv, nf, farr = _team_args(graphs, factors, root_variance)
    L.lins_host_team_graph_solve.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(TeamFactorC), C.POINTER(PoseGraphParamsC),
                                             C.POINTER(TeamGraphResultC)]
    L.lins_host_team_graph_solve.restype = C.c_int
    rc = L.lins_host_team_graph_solve(n, hs, rv.ctypes.data, nf, farr, C.byref(prm), C.byref(out))
    return rc if rc else out.as_dict()


def team_graph_linearize(graphs, factors=(), poses=None, root_variance=None):
    """lins_host_team_graph_linearize at the absolute poses of all members back to back (sum N, 12) (None: the estimates) ->
    dict r_factor (F, 6), M (F, 6, 6), r_root (members - 1, 6), H_root (members - 1, 6, 6), g_root (members - 1, 6)"""
    from ._ctypes_defs import TeamFactorC

    L = lib()
    n, hs, rv, nf, farr = _team_args(graphs, factors, root_variance)
    T = None if poses is None else np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
    assert T is None or len(T) == sum(g.count()[0] for g in graphs)
    k = max(n - 1, 1)
    rf, M, rr, H, g = np.zeros((max(nf, 1), 6)), np.zeros((max(nf, 1), 6, 6)), np.zeros((k, 6)), np.zeros((k, 6, 6)), np.zeros((k, 6))
    L.lins_host_team_graph_linearize.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(TeamFactorC)] + [C.c_void_p] * 6
    L.lins_host_team_graph_linearize.restype = C.c_int
    rc = L.lins_host_team_graph_linearize(n, hs, rv.ctypes.data, nf, farr, T.ctypes.data if T is not None else None, rf.ctypes.data,
                                          M.ctypes.data, rr.ctypes.data, H.ctypes.data, g.ctypes.data)
    if rc:
        raise RuntimeError(f"lins_host_team_graph_linearize: {rc}")
    return dict(r_factor=rf[:nf], M=M[:nf], r_root=rr[:n - 1], H_root=H[:n - 1], g_root=g[:n - 1])


# ---- pairwise-consistent team factors on the CPU (include/lins_host.h lins_host_team_factors_consistent) ----------
def team_pcm_params(**kw):
    from ._ctypes_defs import team_pcm_params as rec

    return rec(lib(), **kw)


def team_factors_consistent(factors, Tb, Ta, n_factors=None, out=None, **kw):
    """lins_host_team_factors_consistent of ONE group: factors whose slots are member indices (TeamFactorC records, dicts or
    tuples), Tb / Ta (n, 12): the f64 estimates of every factor's two frames.  kw: fields of lins_team_pcm_params over the
    defaults.  n_factors: the count to pass instead of len(factors); out: a TeamPcmResultC to write into (for the
    refusals).  Returns dict(n_factors, n_kept, n_pairs, n_pairs_kept, exact, nodes_max, kept: the kept factors' indices),
    or the C return code (a negative int) of a refused call."""
    from ._ctypes_defs import TeamFactorC, TeamPcmParamsC, TeamPcmResultC, team_factor as rec

    L = lib()
    fac = [rec(f) for f in factors]
    n = len(fac) if n_factors is None else int(n_factors)
    farr = (TeamFactorC * max(len(fac), 1))(*fac)
    b = np.ascontiguousarray(Tb, np.float64).reshape(-1, 12) if len(fac) else np.zeros((1, 12))
    a = np.ascontiguousarray(Ta, np.float64).reshape(-1, 12) if len(fac) else np.zeros((1, 12))
    assert len(a) >= len(fac) and len(b) >= len(fac)
    prm = team_pcm_params(**kw)
    res = out if out is not None else TeamPcmResultC()
    L.lins_host_team_factors_consistent.argtypes = [C.c_int, C.POINTER(TeamFactorC), C.c_void_p, C.c_void_p, C.POINTER(TeamPcmParamsC),
                                                    C.POINTER(TeamPcmResultC)]
    L.lins_host_team_factors_consistent.restype = C.c_int
    rc = L.lins_host_team_factors_consistent(n, farr, b.ctypes.data, a.ctypes.data, C.byref(prm), C.byref(res))
    return rc if rc else res.as_dict()


def team_factors_consistent_graphs(graphs, factors, **kw):
    """team_factors_consistent with the poses taken from PoseGraph objects: graphs[m] is member m"""
    from ._ctypes_defs import team_factor as rec

    fac = [rec(f) for f in factors]
    T = [g.poses_f64() for g in graphs]
    Tb = np.array([T[f.slot_b][f.id_b] for f in fac]).reshape(-1, 12)
    Ta = np.array([T[f.slot_a][f.id_a] for f in fac]).reshape(-1, 12)
    return team_factors_consistent(fac, Tb, Ta, **kw)


def team_pcm_clique(adj, pair=None, out=None, **kw):
    """lins_host_team_pcm_clique: the search and the winners alone.  adj: n 64-bit rows (bit b of row a: a and b are
    consistent); pair: n keys (default: one pair) -> the result dict, or the C return code of a refused call"""
    from ._ctypes_defs import TeamPcmParamsC, TeamPcmResultC

    L = lib()
    rows = np.ascontiguousarray(adj, np.uint64)
    n = len(rows)
    keys = np.ascontiguousarray(pair if pair is not None else np.zeros(n), np.int32)
    assert len(keys) == n
    prm = team_pcm_params(**kw)
    res = out if out is not None else TeamPcmResultC()
    L.lins_host_team_pcm_clique.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(TeamPcmParamsC), C.POINTER(TeamPcmResultC)]
    L.lins_host_team_pcm_clique.restype = C.c_int
    rc = L.lins_host_team_pcm_clique(n, rows.ctypes.data if n else None, keys.ctypes.data if n else None, C.byref(prm), C.byref(res))
    return rc if rc else res.as_dict()
