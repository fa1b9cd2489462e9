"""ctypes mirrors of the PODs in include/lins_ieskf.h and include/lins_host.h.

Shared by the product bindings (ieskf.py, host.py) and by the oracle's test
binding (oracle/oracle.py) — it describes the C ABI only, no behaviour.
"""
import ctypes as C

import numpy as np

STATE_DIM = 19
ERR_DIM = 18
MAX_QUERY = 1024
CLOUD_MAX = 16 * 1800
OUTLIER_MAX = (16 - 6) * (1800 // 5)  # LINS_OUTLIER_MAX: rows above groundScanInd, every fifth column
# `path` of lins_debug_cov_update(ctx, path, n, P, sums, r2, diverged, out) by index (csrc/lins_capi_debug.hip): the
# covariance epilogue of the three LDS kernel families, then the any-size path's stand-alone kernel
COV_PATHS = ("lds", "lds1", "mr", "joseph")

LINS_OK = 0
STREAMS_IMU_MAX = 64  # LINS_STREAMS_IMU_MAX: IMU rows per stream and call of the streams' device filter
STREAMS_GATED = 1     # LINS_STREAMS_GATED: Result.reserved[0] of a scan the reference's feature gate (SE:436-440) stopped
# the streams' state machine (include/lins_streams_filter.h): status_ values (SE:177-183) and Result.reserved[0] of an
# accepted first / second scan
STREAM_INIT, STREAM_FIRST_SCAN, STREAM_RUNNING = 0, 1, 3
STREAMS_FIRST, STREAMS_BOOTED = 2, 3
E_STATE, E_UNSUPPORTED = -6, -7


class Point(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("intensity", C.c_float)]


class Params(C.Structure):
    _fields_ = [
        ("num_iter", C.c_int32),
        ("icp_freq", C.c_int32),
        ("fixed_iters", C.c_int32),
        ("reserved", C.c_int32),
        ("lidar_std", C.c_double),
        ("lidar_scale", C.c_double),
        ("nearest_sq_dist", C.c_double),
        ("scan_period", C.c_double),
    ]


def default_params(num_iter=30, fixed_iters=0, icp_freq=1):
    """exp_port.yaml:11-20 values."""
    return Params(num_iter, icp_freq, fixed_iters, 0, 0.01, 1.0, 25.0, 0.1)


class ScanPairC(C.Structure):
    _fields_ = [
        ("surf_flat", C.POINTER(Point)),
        ("corner_sharp", C.POINTER(Point)),
        ("surf_less_flat_last", C.POINTER(Point)),
        ("corner_less_sharp_last", C.POINTER(Point)),
        ("n_surf_flat", C.c_int32),
        ("n_corner_sharp", C.c_int32),
        ("n_surf_last", C.c_int32),
        ("n_corner_last", C.c_int32),
        ("point_stride_bytes", C.c_int32),  # 0 / 16: packed points; 32: pcl::PointXYZI arrays
        ("reserved", C.c_int32),
        ("state", C.c_double * STATE_DIM),
        ("cov", C.c_double * (ERR_DIM * ERR_DIM)),
    ]


class ResultC(C.Structure):
    _fields_ = [
        ("state", C.c_double * STATE_DIM),
        ("cov", C.c_double * (ERR_DIM * ERR_DIM)),
        ("residual_norm", C.c_double),
        ("update_norm", C.c_double),
        ("iters", C.c_int32),
        ("converged", C.c_int32),
        ("diverged", C.c_int32),
        ("m_surf", C.c_int32),
        ("m_corner", C.c_int32),
        ("reserved", C.c_int32 * 3),
    ]


class PoseRecordC(C.Structure):
    _fields_ = [
        ("state", C.c_double * STATE_DIM),
        ("residual_norm", C.c_double),
        ("iters", C.c_int32),
        ("converged", C.c_int32),
        ("diverged", C.c_int32),
        ("m_surf", C.c_int32),
        ("m_corner", C.c_int32),
        ("scan_id", C.c_int32),
        ("pad", C.c_int32 * 2),
    ]


assert C.sizeof(PoseRecordC) == 192

CORR_DTYPE = np.dtype(
    [("ind1", "<i4"), ("ind2", "<i4"), ("ind3", "<i4"), ("accepted", "<i4"), ("coeff", "<f4", (4,)), ("sel", "<f4", (4,))]
)
assert CORR_DTYPE.itemsize == 48

POSE_DTYPE = np.dtype(
    [
        ("state", "<f8", (STATE_DIM,)),
        ("residual_norm", "<f8"),
        ("iters", "<i4"),
        ("converged", "<i4"),
        ("diverged", "<i4"),
        ("m_surf", "<i4"),
        ("m_corner", "<i4"),
        ("scan_id", "<i4"),
        ("pad", "<i4", (2,)),
    ]
)
assert POSE_DTYPE.itemsize == 192


def _pts(a):
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4)
    return a


class ScanPair:
    """One IESKF problem: queries, targets, prior state + covariance."""

    def __init__(self, surf_flat, corner_sharp, surf_last, corner_last, state, cov, meta=None):
        self.surf_flat = _pts(surf_flat)
        self.corner_sharp = _pts(corner_sharp)
        self.surf_last = _pts(surf_last)
        self.corner_last = _pts(corner_last)
        self.state = np.ascontiguousarray(state, dtype=np.float64).reshape(STATE_DIM)
        self.cov = np.ascontiguousarray(cov, dtype=np.float64).reshape(ERR_DIM, ERR_DIM)
        self.meta = meta or {}

    def sizes(self):
        return (len(self.corner_sharp), len(self.surf_flat), len(self.corner_last), len(self.surf_last))

    def bytes_per_iter(self):
        """Algorithmic bytes of one iteration."""
        return 16 * sum(self.sizes()) + 8 * 19 + 8 * 28

    def as_c(self):
        c = ScanPairC()
        self.fill_c(c)
        return c

    def fill_c(self, c):
        c.surf_flat = self.surf_flat.ctypes.data_as(C.POINTER(Point))
        c.corner_sharp = self.corner_sharp.ctypes.data_as(C.POINTER(Point))
        c.surf_less_flat_last = self.surf_last.ctypes.data_as(C.POINTER(Point))
        c.corner_less_sharp_last = self.corner_last.ctypes.data_as(C.POINTER(Point))
        c.n_surf_flat = len(self.surf_flat)
        c.n_corner_sharp = len(self.corner_sharp)
        c.n_surf_last = len(self.surf_last)
        c.n_corner_last = len(self.corner_last)
        C.memmove(c.state, self.state.ctypes.data, 8 * STATE_DIM)
        C.memmove(c.cov, self.cov.ctypes.data, 8 * ERR_DIM * ERR_DIM)


def pairs_to_c(pairs):
    arr = (ScanPairC * len(pairs))()
    for i, p in enumerate(pairs):
        p.fill_c(arr[i])
    return arr


def pairs_strided(pairs):
    """The same pairs with their clouds as pcl::PointXYZI lays them out (32 bytes a point: x, y, z, pad, intensity, 3 pads;
    parameters.h:52) and point_stride_bytes = 32: what a lins_fusion_node passes without repacking.  Returns the ScanPairC
    array and the arrays that own the memory (keep them alive)."""
    arr = pairs_to_c(pairs)
    keep = []
    for i, p in enumerate(pairs):
        for name, src in (("surf_flat", p.surf_flat), ("corner_sharp", p.corner_sharp), ("surf_less_flat_last", p.surf_last),
                          ("corner_less_sharp_last", p.corner_last)):
            wide = np.full((len(src), 8), np.float32(-77.0))  # (pads hold a value no cloud has: read by mistake, it shows)
            wide[:, 0:3], wide[:, 4] = src[:, 0:3], src[:, 3]
            keep.append(wide)
            setattr(arr[i], name, wide.ctypes.data_as(C.POINTER(Point)))
        arr[i].point_stride_bytes = 32
    return arr, keep


class Result:
    def __init__(self, rc):
        self.state = np.array(rc.state[:], dtype=np.float64)
        self.cov = np.array(rc.cov[:], dtype=np.float64).reshape(ERR_DIM, ERR_DIM)
        self.residual_norm = rc.residual_norm
        self.update_norm = rc.update_norm
        self.iters = rc.iters
        self.converged = rc.converged
        self.diverged = rc.diverged
        self.m_surf = rc.m_surf
        self.m_corner = rc.m_corner
        self.reserved = tuple(rc.reserved[:])  # debug counters of the kernels (certificate / exhaustive-search statistics)

    def __repr__(self):
        return (
            f"Result(iters={self.iters}, conv={self.converged}, div={self.diverged}, "
            f"m=({self.m_surf},{self.m_corner}), p={self.state[:3]}, |r|={self.residual_norm:.4g})"
        )


# ---- scan-to-map row (include/lins_map.h) -------------------------------------------------
LINS_MAP_REUSE, LINS_MAP_LOCAL = 1, 2


class MapProblemC(C.Structure):
    _fields_ = [("map_corner", C.POINTER(Point)), ("map_surf", C.POINTER(Point)), ("scan_corner", C.POINTER(Point)),
                ("scan_surf", C.POINTER(Point)), ("n_map_corner", C.c_int32), ("n_map_surf", C.c_int32),
                ("n_scan_corner", C.c_int32), ("n_scan_surf", C.c_int32), ("transform", C.c_float * 6),
                ("reserved", C.c_int32 * 2)]


class MapResultC(C.Structure):
    _fields_ = [("transform", C.c_float * 6), ("iters", C.c_int32), ("converged", C.c_int32),
                ("degenerate", C.c_int32), ("n_sel", C.c_int32)]


MAP_CORR_DTYPE = np.dtype([("ind", np.int32, 5), ("accepted", np.int32), ("coeff", np.float32, 4),
                           ("sel", np.float32, 3), ("sq5", np.float32)])


class MapProblem:
    """numpy-owned scan-to-map problem; as_c() gives the ctypes view."""

    def __init__(self, map_corner, map_surf, scan_corner, scan_surf, transform):
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4)
        self.map_corner, self.map_surf, self.scan_corner, self.scan_surf = f(map_corner), f(map_surf), f(scan_corner), f(scan_surf)
        self.transform = np.asarray(transform, dtype=np.float32).copy()
        self.reuse_resident_map = False  # LINS_MAP_REUSE: the maps are the previous call's (lins_map.h)
        self.use_local_map = False  # LINS_MAP_LOCAL: maps and queries are entry k of the last local-map build

    @classmethod
    def local(cls, transform):
        """problem k of a LINS_MAP_LOCAL batch: the clouds are those of entry k of the last lins_local_map_build"""
        e = np.zeros((0, 4), np.float32)
        p = cls(e, e, e, e, transform)
        p.use_local_map = True
        return p

    def as_c(self):
        c = MapProblemC()
        c.reserved[0] = (LINS_MAP_REUSE if self.reuse_resident_map else 0) | (LINS_MAP_LOCAL if self.use_local_map else 0)
        pp = lambda a: a.ctypes.data_as(C.POINTER(Point))
        c.map_corner, c.map_surf, c.scan_corner, c.scan_surf = pp(self.map_corner), pp(self.map_surf), pp(self.scan_corner), pp(self.scan_surf)
        c.n_map_corner, c.n_map_surf = len(self.map_corner), len(self.map_surf)
        c.n_scan_corner, c.n_scan_surf = len(self.scan_corner), len(self.scan_surf)
        c.transform[:] = [float(v) for v in self.transform]
        return c


# ---- the mapping node's local map (include/lins_map.h lins_local_map_*) -------------------
LOCAL_MAP_CORNER, LOCAL_MAP_SURF, LOCAL_SCAN_CORNER, LOCAL_SCAN_SURF, LOCAL_SCAN_OUTLIER, LOCAL_SCAN_TOTAL = range(6)


class KeyPoseC(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("roll", C.c_float), ("pitch", C.c_float), ("yaw", C.c_float)]


def key_pose(p):
    """(x, y, z, roll, pitch, yaw) -> lins_key_pose"""
    return KeyPoseC(*[float(v) for v in np.asarray(p, dtype=np.float32)])


class KeyframeC(C.Structure):
    _fields_ = [("corner", C.POINTER(Point)), ("surf", C.POINTER(Point)), ("outlier", C.POINTER(Point)),
                ("n_corner", C.c_int32), ("n_surf", C.c_int32), ("n_outlier", C.c_int32), ("reserved", C.c_int32),
                ("pose", KeyPoseC)]


class LocalScanC(C.Structure):
    _fields_ = [("corner", C.POINTER(Point)), ("surf", C.POINTER(Point)), ("outlier", C.POINTER(Point)),
                ("n_corner", C.c_int32), ("n_surf", C.c_int32), ("n_outlier", C.c_int32), ("reserved", C.c_int32)]


class LocalMapSizesC(C.Structure):
    _fields_ = [("n", C.c_int32 * 6), ("box_min", (C.c_int32 * 3) * 2), ("box_dim", (C.c_int32 * 3) * 2),
                ("frames", C.c_int32), ("status", C.c_int32)]

    def as_dict(self):
        return dict(n=[int(v) for v in self.n], box_min=[list(r) for r in self.box_min], box_dim=[list(r) for r in self.box_dim],
                    frames=int(self.frames), status=int(self.status))


def cloud(a):
    """an (n, 4) f32 C-contiguous array (x, y, z, intensity)"""
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4)


def keyframe_c(corner, surf, outlier, pose):
    """lins_keyframe over numpy clouds; returns (struct, the arrays it points into)"""
    keep = [cloud(corner), cloud(surf), cloud(outlier)]
    pp = lambda a: a.ctypes.data_as(C.POINTER(Point))
    f = KeyframeC(pp(keep[0]), pp(keep[1]), pp(keep[2]), len(keep[0]), len(keep[1]), len(keep[2]), 0, key_pose(pose))
    return f, keep


def local_scan_c(corner, surf, outlier):
    keep = [cloud(corner), cloud(surf), cloud(outlier)]
    pp = lambda a: a.ctypes.data_as(C.POINTER(Point))
    return LocalScanC(pp(keep[0]), pp(keep[1]), pp(keep[2]), len(keep[0]), len(keep[1]), len(keep[2]), 0), keep


# ---- the key-frame archive (include/lins_map.h lins_archive_*) ------------------------------
SUBMAP_CORNER, SUBMAP_SURF, SUBMAP_OUTLIER = 1, 2, 4
SUBMAP_DROP_NEGATIVE = 1


class SubmapSpecC(C.Structure):
    _fields_ = [("ids", C.POINTER(C.c_int32)), ("n_ids", C.c_int32), ("slot", C.c_int32), ("clouds", C.c_int32),
                ("flags", C.c_int32), ("leaf", C.c_float), ("reserved", C.c_int32)]


class SubmapInfoC(C.Structure):
    _fields_ = [("n", C.c_int32), ("frames", C.c_int32), ("points_in", C.c_uint64), ("box_min", C.c_int32 * 3),
                ("box_dim", C.c_int32 * 3), ("status", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return dict(n=int(self.n), frames=int(self.frames), points_in=int(self.points_in), box_min=list(self.box_min),
                    box_dim=list(self.box_dim), status=int(self.status))


# ---- key-pose selection on the device (include/lins_map.h lins_keyposes_*) ------------------
KEYPOSES_HOST, KEYPOSES_DEVICE = 0, 1


class KeyposesQueryC(C.Structure):
    _fields_ = [("slot", C.c_int32), ("centre", C.c_float * 3), ("radius", C.c_float), ("pose_leaf", C.c_float)]


class KeyposesLoopQueryC(C.Structure):
    _fields_ = [("q", KeyposesQueryC), ("now", C.c_double), ("min_gap_s", C.c_double)]


class KeyposesResultC(C.Structure):
    _fields_ = [("n", C.c_int32), ("hits", C.c_int32), ("status", C.c_int32), ("host", C.c_int32)]

    def as_dict(self):
        return dict(n=int(self.n), hits=int(self.hits), status=int(self.status), host=int(self.host))


def keyposes_query(slot, centre, radius, pose_leaf=1.0):
    return KeyposesQueryC(int(slot), (C.c_float * 3)(*[float(v) for v in centre]), float(radius), float(pose_leaf))


# ---- the team selection (include/lins_map.h lins_keyposes_team_select_batch) -----------------
KEYPOSES_TEAM_CELLS = 4096


class KeyposesTeamQueryC(C.Structure):
    _fields_ = [("centre", C.c_float * 3), ("radius", C.c_float), ("pose_leaf", C.c_float), ("n_targets", C.c_int32),
                ("first_target", C.c_int32), ("reserved", C.c_int32)]


def keyposes_team_query(centre, radius, pose_leaf, n_targets, first_target):
    return KeyposesTeamQueryC((C.c_float * 3)(*[float(v) for v in centre]), float(radius), float(pose_leaf), int(n_targets), int(first_target), 0)


# ---- the loop-closure ICP (include/lins_map.h lins_loop_icp_*, include/lins_host.h lins_host_loop_icp*) --------
ICP_NONE, ICP_ITERATIONS, ICP_TRANSFORM, ICP_ABS_MSE, ICP_REL_MSE, ICP_NO_CORRESPONDENCES = range(6)


class LoopIcpParamsC(C.Structure):
    _fields_ = [("transformation_epsilon", C.c_double), ("fitness_epsilon", C.c_double), ("rel_mse", C.c_double),
                ("rotation_threshold", C.c_double), ("max_corr_dist", C.c_float), ("max_iterations", C.c_int32),
                ("min_correspondences", C.c_int32), ("reserved", C.c_int32)]


class LoopIcpProblemC(C.Structure):
    _fields_ = [("source_entry", C.c_int32), ("target_entry", C.c_int32), ("source", C.POINTER(Point)), ("target", C.POINTER(Point)),
                ("n_source", C.c_int32), ("n_target", C.c_int32)]


class LoopIcpResultC(C.Structure):
    _fields_ = [("transform", C.c_double * 16), ("fitness", C.c_double), ("mse", C.c_double), ("iterations", C.c_int32),
                ("converged", C.c_int32), ("reason", C.c_int32), ("n_corr", C.c_int32), ("n_fitness", C.c_int32),
                ("far_searches", C.c_uint32), ("status", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return dict(transform=np.array(self.transform[:], np.float64).reshape(4, 4), fitness=float(self.fitness), mse=float(self.mse),
                    iterations=int(self.iterations), converged=int(self.converged), reason=int(self.reason), n_corr=int(self.n_corr),
                    n_fitness=int(self.n_fitness), far_searches=int(self.far_searches), status=int(self.status))


class LoopIcpRoundC(C.Structure):
    _fields_ = [("T_in", C.c_double * 16), ("delta", C.c_double * 16), ("T_out", C.c_double * 16), ("mse", C.c_double),
                ("stop", C.c_double * 4), ("n_corr", C.c_int32), ("reason", C.c_int32)]

    def as_dict(self):
        m = lambda a: np.array(a[:], np.float64).reshape(4, 4)
        return dict(T_in=m(self.T_in), delta=m(self.delta), T_out=m(self.T_out), mse=float(self.mse),
                    stop=np.array(self.stop[:], np.float64), n_corr=int(self.n_corr), reason=int(self.reason))


class LoopIcpStateC(C.Structure):
    _fields_ = [("T", C.c_double * 16), ("mse_prev", C.c_double), ("mse", C.c_double), ("fitness", C.c_double), ("move", C.c_float * 12),
                ("iterations", C.c_int32), ("converged", C.c_int32), ("reason", C.c_int32), ("n_corr", C.c_int32), ("n_fitness", C.c_int32),
                ("active", C.c_int32)]
    COUNTS = ("iterations", "converged", "reason", "n_corr", "n_fitness", "active")

    def as_dict(self):
        d = dict(T=np.array(self.T[:], np.float64).reshape(4, 4), mse_prev=float(self.mse_prev), mse=float(self.mse), fitness=float(self.fitness),
                 move=np.array(self.move[:], np.float32).reshape(3, 4))
        d.update((k, int(getattr(self, k))) for k in self.COUNTS)
        return d


def loop_icp_state(state=None):
    """lins_loop_icp_state: a fresh problem (T = I, mse_prev = fitness = DBL_MAX, active = 1) with the fields of the dict
    `state` (as as_dict gives them; `move` is out only) put over it"""
    s = LoopIcpStateC()
    d = dict(T=np.eye(4), mse_prev=np.finfo(np.float64).max, mse=0.0, fitness=np.finfo(np.float64).max, active=1)
    d.update(state or {})
    for k, v in d.items():
        if k == "T":
            s.T[:] = [float(x) for x in np.asarray(v, np.float64).reshape(16)]
        elif k != "move":
            if not hasattr(s, k):
                raise TypeError(k)
            setattr(s, k, v)
    return s


def loop_icp_params(lib, **kw):
    """lins_loop_icp_default_params of `lib` (both libraries export it) with fields overridden by keyword"""
    p = LoopIcpParamsC()
    lib.lins_loop_icp_default_params.argtypes = [C.POINTER(LoopIcpParamsC)]
    lib.lins_loop_icp_default_params.restype = None
    lib.lins_loop_icp_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(k)
        setattr(p, k, v)
    return p


def loop_icp_problem_c(source, target):
    """lins_loop_icp_problem: each cloud an int (entry of the last archive assembly) or an (n, 4) array; returns
    (struct, the arrays it points into)"""
    c, keep = LoopIcpProblemC(), []
    c.source_entry = c.target_entry = -1
    for name, v in (("source", source), ("target", target)):
        if isinstance(v, (int, np.integer)):
            setattr(c, name + "_entry", int(v))
        else:
            a = cloud(v)
            keep.append(a)
            setattr(c, name, a.ctypes.data_as(C.POINTER(Point)))
            setattr(c, "n_" + name, len(a))
    return c, keep


# ---- the pose graph (include/lins_map.h lins_pose_graph_*, include/lins_host.h lins_host_pose_graph_*) --------
PG_NONE, PG_ITERATIONS, PG_INCREMENT, PG_REL_COST = range(4)


class PoseGraphParamsC(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("reserved", C.c_int32), ("rel_cost_decrease", C.c_double), ("max_increment", C.c_double),
                ("lambda_initial", C.c_double), ("lambda_up", C.c_double), ("lambda_down", C.c_double)]


class PoseGraphResultC(C.Structure):
    _fields_ = [("cost_before", C.c_double), ("cost_after", C.c_double), ("max_increment", C.c_double), ("iterations", C.c_int32),
                ("reason", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return dict(cost_before=float(self.cost_before), cost_after=float(self.cost_after), max_increment=float(self.max_increment),
                    iterations=int(self.iterations), reason=int(self.reason), status=int(self.status))


def pose_graph_params(lib, **kw):
    """lins_pose_graph_default_params of `lib` (both libraries export it) with fields overridden by keyword"""
    p = PoseGraphParamsC()
    lib.lins_pose_graph_default_params.argtypes = [C.POINTER(PoseGraphParamsC)]
    lib.lins_pose_graph_default_params.restype = None
    lib.lins_pose_graph_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"lins_pose_graph_params has no field {k}")
        setattr(p, k, v)
    return p


# ---- the team graph (include/lins_team.h lins_team_graph_*, include/lins_host.h lins_host_team_graph_*) --------
class TeamFactorC(C.Structure):
    _fields_ = [("slot_b", C.c_int32), ("id_b", C.c_int32), ("slot_a", C.c_int32), ("id_a", C.c_int32), ("Z", C.c_double * 12),
                ("var", C.c_double)]

    def as_dict(self):
        return dict(slot_b=int(self.slot_b), id_b=int(self.id_b), slot_a=int(self.slot_a), id_a=int(self.id_a),
                    Z=np.array(self.Z[:], np.float64), var=float(self.var))


class TeamMemberC(C.Structure):
    _fields_ = [("slot", C.c_int32), ("reserved", C.c_int32), ("root_variance", C.c_double * 6)]


class TeamGraphResultC(C.Structure):
    _fields_ = [("solve", PoseGraphResultC), ("n_frames", C.c_int32), ("n_loops", C.c_int32), ("n_factors", C.c_int32),
                ("reserved", C.c_int32)]

    def as_dict(self):
        return dict(self.solve.as_dict(), n_frames=int(self.n_frames), n_loops=int(self.n_loops), n_factors=int(self.n_factors))


def team_factor(f):
    """a TeamFactorC from a TeamFactorC, a dict of its fields, or a tuple (slot_b, id_b, slot_a, id_a, Z, var)"""
    if isinstance(f, TeamFactorC):
        return f
    if isinstance(f, dict):
        f = (f["slot_b"], f["id_b"], f["slot_a"], f["id_a"], f["Z"], f["var"])
    c = TeamFactorC(int(f[0]), int(f[1]), int(f[2]), int(f[3]))
    c.Z[:] = [float(x) for x in np.asarray(f[4], np.float64).reshape(12)]
    c.var = float(f[5])
    return c


# ---- pairwise-consistent team factors (include/lins_host.h lins_team_pcm_*) ------------------------------------
TEAM_PCM_MAX_FACTORS = 64


class TeamPcmParamsC(C.Structure):
    _fields_ = [("max_translation", C.c_double), ("min_cos_rotation", C.c_double), ("translation_per_frame", C.c_double),
                ("min_support", C.c_int32), ("max_nodes", C.c_int32)]


class TeamPcmResultC(C.Structure):
    _fields_ = [("n_factors", C.c_int32), ("n_kept", C.c_int32), ("n_pairs", C.c_int32), ("n_pairs_kept", C.c_int32), ("exact", C.c_int32),
                ("nodes_max", C.c_uint32), ("kept", C.c_uint32 * 2)]

    def as_dict(self):
        return dict(n_factors=int(self.n_factors), n_kept=int(self.n_kept), n_pairs=int(self.n_pairs), n_pairs_kept=int(self.n_pairs_kept),
                    exact=int(self.exact), nodes_max=int(self.nodes_max),
                    kept=[f for f in range(TEAM_PCM_MAX_FACTORS) if (int(self.kept[f >> 5]) >> (f & 31)) & 1])


def team_pcm_params(lib, **kw):
    """lins_team_pcm_default_params of library `lib` (max_translation 1.0, min_cos_rotation cos 5 degrees,
    translation_per_frame 0, min_support 3, max_nodes 65536) with fields overridden by keyword"""
    p = TeamPcmParamsC()
    lib.lins_team_pcm_default_params.argtypes = [C.POINTER(TeamPcmParamsC)]
    lib.lins_team_pcm_default_params.restype = None
    lib.lins_team_pcm_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"lins_team_pcm_params has no field {k}")
        setattr(p, k, v)
    return p


# ---- the loop thread's step (include/lins_map.h lins_loop_step) ------------------------------------------------
LOOP_NONE, LOOP_REPEAT, LOOP_REJECTED, LOOP_CLOSED = range(4)
LOOP_CENTRE_STREAM = 1


class LoopStepParamsC(C.Structure):
    _fields_ = [("search_radius", C.c_float), ("max_fitness", C.c_float), ("history_leaf", C.c_float), ("search_num", C.c_int32),
                ("min_gap_s", C.c_double), ("icp", LoopIcpParamsC), ("graph", PoseGraphParamsC)]


class LoopStepEntryC(C.Structure):
    _fields_ = [("slot", C.c_int32), ("stream", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32), ("centre", C.c_float * 3),
                ("pad", C.c_float), ("now", C.c_double)]


class LoopStepResultC(C.Structure):
    _fields_ = [("outcome", C.c_int32), ("status", C.c_int32), ("latest_id", C.c_int32), ("closest_id", C.c_int32), ("latest", SubmapInfoC),
                ("history", SubmapInfoC), ("icp", LoopIcpResultC), ("pose_from", KeyPoseC), ("graph", PoseGraphResultC)]

    def as_dict(self):
        pf = self.pose_from
        return dict(outcome=int(self.outcome), status=int(self.status), latest_id=int(self.latest_id), closest_id=int(self.closest_id),
                    latest=self.latest.as_dict(), history=self.history.as_dict(), icp=self.icp.as_dict(),
                    pose_from=np.array([pf.x, pf.y, pf.z, pf.roll, pf.pitch, pf.yaw], np.float32), graph=self.graph.as_dict())


def loop_step_params(lib, **kw):
    """lins_loop_step_default_params with fields overridden by keyword; icp / graph: dicts of fields of the nested structs"""
    p = LoopStepParamsC()
    lib.lins_loop_step_default_params.argtypes = [C.POINTER(LoopStepParamsC)]
    lib.lins_loop_step_default_params.restype = None
    lib.lins_loop_step_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"lins_loop_step_params has no field {k}")
        if k in ("icp", "graph"):
            for kk, vv in v.items():
                if not hasattr(getattr(p, k), kk):
                    raise TypeError(f"{k} has no field {kk}")
                setattr(getattr(p, k), kk, vv)
        else:
            setattr(p, k, v)
    return p


def loop_step_entry(slot, centre=None, now=0.0, stream=-1):
    """lins_loop_step_entry; centre None: LINS_LOOP_CENTRE_STREAM (currentRobotPosPoint of `stream`)"""
    e = LoopStepEntryC()
    e.slot, e.stream, e.flags, e.now = int(slot), int(stream), LOOP_CENTRE_STREAM if centre is None else 0, float(now)
    if centre is not None:
        e.centre[:] = [float(v) for v in np.asarray(centre, np.float32)[:3]]
    return e


def six_floats(p):
    """six floats (pitch, yaw, roll, y, z, x) as a C array"""
    return (C.c_float * 6)(*[float(v) for v in np.asarray(p, dtype=np.float32)])


# ---- the mapping node's step for streams (include/lins_streams_map.h lins_streams_map_*, lins_map_associate_batch) ----
MAP_STEP_SKIPPED = 1


class MapPoseStateC(C.Structure):
    _fields_ = [("bef", C.c_float * 6), ("aft", C.c_float * 6), ("tobe", C.c_float * 6), ("last", C.c_float * 6), ("prev", C.c_float * 3),
                ("n_frames", C.c_int32), ("last_time", C.c_double)]
    VECTORS = ("bef", "aft", "tobe", "last", "prev")

    def as_dict(self):
        d = {k: np.array(getattr(self, k)[:], np.float32) for k in self.VECTORS}
        d.update(n_frames=int(self.n_frames), last_time=float(self.last_time))
        return d


def map_pose_state(state=None):
    """lins_map_pose_state as lins_streams_map_init leaves it (zero, last_time = -1) with the fields of `state` over it"""
    s = MapPoseStateC()
    s.last_time = -1.0
    for k, v in (state or {}).items():
        if k in MapPoseStateC.VECTORS:
            getattr(s, k)[:] = [float(x) for x in np.asarray(v, np.float32)]
        elif k in ("n_frames", "last_time"):
            setattr(s, k, v)
        else:
            raise TypeError(k)
    return s


class MapOdomC(C.Structure):
    _fields_ = [("transform_sum", C.c_float * 6), ("imu_roll", C.c_float), ("imu_pitch", C.c_float), ("has_imu", C.c_int32),
                ("reserved", C.c_int32), ("time", C.c_double)]


class MapStepResultC(C.Structure):
    _fields_ = [("tobe_start", C.c_float * 6), ("transform", C.c_float * 6), ("key_pose", C.c_float * 6), ("iters", C.c_int32),
                ("converged", C.c_int32), ("degenerate", C.c_int32), ("n_sel", C.c_int32), ("status", C.c_int32), ("key_frame", C.c_int32),
                ("ring_age", C.c_int32), ("archive_id", C.c_int32)]
    COUNTS = ("iters", "converged", "degenerate", "n_sel", "status", "key_frame", "ring_age", "archive_id")

    def as_dict(self):
        d = {k: np.array(getattr(self, k)[:], np.float32) for k in ("tobe_start", "transform", "key_pose")}
        d.update((k, int(getattr(self, k))) for k in self.COUNTS)
        return d


# ---- streams end to end (include/lins_streams_slam.h; lins_stream_odom / lins_fused_pose: include/lins_host.h) ----
class StreamOdomC(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("orientation", C.c_double * 4), ("transform_sum", C.c_float * 6), ("valid", C.c_int32),
                ("reserved", C.c_int32)]

    def as_dict(self):
        return dict(position=np.array(self.position[:], np.float64), orientation=np.array(self.orientation[:], np.float64),
                    transform_sum=np.array(self.transform_sum[:], np.float32), valid=int(self.valid))


class FusedPoseC(C.Structure):
    _fields_ = [("transform_mapped", C.c_float * 6), ("orientation", C.c_double * 4)]

    def as_dict(self):
        return dict(transform_mapped=np.array(self.transform_mapped[:], np.float32), orientation=np.array(self.orientation[:], np.float64))


class SlamImuC(C.Structure):
    _fields_ = [("roll", C.c_float), ("pitch", C.c_float), ("has_imu", C.c_int32), ("reserved", C.c_int32)]


# ---- stream lifecycle (include/lins_lifecycle.h): the records of the compaction plan ----
class ArenaBlockC(C.Structure):
    _fields_ = [("off", C.c_longlong), ("n", C.c_longlong), ("keep", C.c_int32), ("reserved", C.c_int32)]


class ArenaSegmentC(C.Structure):
    _fields_ = [("src", C.c_longlong), ("dst", C.c_longlong), ("n", C.c_longlong), ("pass_", C.c_int32), ("direct", C.c_int32)]


# ---- place recognition (include/lins_place.h, include/lins_host.h lins_host_place_*) ----
PLACE_RINGS, PLACE_SECTORS, PLACE_CELLS = 20, 60, 1200


class PlaceParamsC(C.Structure):
    _fields_ = [("r_max", C.c_float), ("lift", C.c_float), ("up_axis", C.c_int32), ("clouds", C.c_int32)]


class PlaceQueryC(C.Structure):
    _fields_ = [("query_slot", C.c_int32), ("query_id", C.c_int32), ("target_slot", C.c_int32), ("reserved", C.c_int32),
                ("now", C.c_double), ("min_gap_s", C.c_double)]


class PlaceResultC(C.Structure):
    _fields_ = [("id", C.c_int32), ("shift", C.c_int32), ("distance", C.c_float), ("candidates", C.c_int32), ("status", C.c_int32),
                ("reserved", C.c_int32)]

    def as_dict(self):
        return dict(id=int(self.id), shift=int(self.shift), distance=np.float32(self.distance), candidates=int(self.candidates),
                    status=int(self.status))


def place_params(L, **kw):
    """lins_place_default_params of library L with fields overridden by keyword (up_axis=2, ...)"""
    p = PlaceParamsC()
    L.lins_place_default_params.argtypes = [C.POINTER(PlaceParamsC)]
    L.lins_place_default_params.restype = None
    L.lins_place_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def place_query(query_slot, query_id, target_slot, now, min_gap_s):
    return PlaceQueryC(int(query_slot), int(query_id), int(target_slot), 0, float(now), float(min_gap_s))


# ---- the loop thread's step by appearance (include/lins_place.h lins_loop_step_place) ----
PLACE_MAX_K = 8
LOOP_DETECT_PLACE, LOOP_DETECT_POSE_THEN_PLACE = 0, 1


class LoopPlaceParamsC(C.Structure):
    _fields_ = [("mode", C.c_int32), ("k", C.c_int32), ("min_sep", C.c_int32), ("reserved", C.c_int32), ("max_distance", C.c_float),
                ("pad", C.c_float)]


class LoopPlaceResultC(C.Structure):
    _fields_ = [("step", LoopStepResultC), ("detect", C.c_int32), ("n_candidates", C.c_int32), ("chosen", C.c_int32), ("reserved", C.c_int32),
                ("cand", PlaceResultC * PLACE_MAX_K), ("icp", LoopIcpResultC * PLACE_MAX_K)]

    def as_dict(self):
        n = int(self.n_candidates)
        return dict(step=self.step.as_dict(), detect=int(self.detect), n_candidates=n, chosen=int(self.chosen),
                    cand=[self.cand[j].as_dict() for j in range(n)], icp=[self.icp[j].as_dict() for j in range(n)])


def loop_place_params(lib, **kw):
    """lins_loop_place_default_params with fields overridden by keyword (mode=, k=, min_sep=, max_distance=)"""
    p = LoopPlaceParamsC()
    lib.lins_loop_place_default_params.argtypes = [C.POINTER(LoopPlaceParamsC)]
    lib.lins_loop_place_default_params.restype = None
    lib.lins_loop_place_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"lins_loop_place_params has no field {k}")
        setattr(p, k, v)
    return p


# ---- team search (include/lins_team.h, include/lins_host.h lins_host_place_team_topk) ----
PLACE_MAX_SHORTLIST, PLACE_MAX_TEAM_SLOTS = 64, 65536


class PlaceTeamParamsC(C.Structure):
    _fields_ = [("shortlist", C.c_int32), ("k", C.c_int32), ("min_sep", C.c_int32), ("reserved", C.c_int32)]


class PlaceTeamQueryC(C.Structure):
    _fields_ = [("query_slot", C.c_int32), ("query_id", C.c_int32), ("now", C.c_double), ("min_gap_s", C.c_double)]


class PlaceTeamResultC(C.Structure):
    _fields_ = [("slot", C.c_int32), ("id", C.c_int32), ("shift", C.c_int32), ("distance", C.c_float), ("dk", C.c_int32),
                ("candidates", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return dict(slot=int(self.slot), id=int(self.id), shift=int(self.shift), distance=np.float32(self.distance), dk=int(self.dk),
                    candidates=int(self.candidates), status=int(self.status))


def place_team_params(lib, **kw):
    """lins_place_team_default_params of library `lib` with fields overridden by keyword (shortlist=, k=, min_sep=)"""
    p = PlaceTeamParamsC()
    lib.lins_place_team_default_params.argtypes = [C.POINTER(PlaceTeamParamsC)]
    lib.lins_place_team_default_params.restype = None
    lib.lins_place_team_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"lins_place_team_params has no field {k}")
        setattr(p, k, v)
    return p


RENDEZVOUS_NONE, RENDEZVOUS_REJECTED, RENDEZVOUS_FOUND = 0, 1, 2


class RendezvousEntryC(C.Structure):
    _fields_ = [("slot", C.c_int32), ("reserved", C.c_int32), ("now", C.c_double)]


class RendezvousParamsC(C.Structure):
    _fields_ = [("team", PlaceTeamParamsC), ("max_distance", C.c_float), ("pad", C.c_float)]


class RendezvousResultC(C.Structure):
    _fields_ = [("outcome", C.c_int32), ("status", C.c_int32), ("latest_id", C.c_int32), ("n_candidates", C.c_int32), ("chosen", C.c_int32),
                ("target_slot", C.c_int32), ("target_id", C.c_int32), ("reserved", C.c_int32), ("latest", SubmapInfoC),
                ("cand", PlaceTeamResultC * PLACE_MAX_K), ("target", SubmapInfoC * PLACE_MAX_K), ("icp", LoopIcpResultC * PLACE_MAX_K),
                ("X", C.c_double * 16)]

    def as_dict(self):
        n = int(self.n_candidates)
        return dict(outcome=int(self.outcome), status=int(self.status), latest_id=int(self.latest_id), n_candidates=n, chosen=int(self.chosen),
                    target_slot=int(self.target_slot), target_id=int(self.target_id), latest=self.latest.as_dict(),
                    cand=[self.cand[j].as_dict() for j in range(n)], target=[self.target[j].as_dict() for j in range(n)],
                    icp=[self.icp[j].as_dict() for j in range(n)], X=np.array(self.X[:], np.float64).reshape(4, 4))


def rendezvous_params(lib, **kw):
    """lins_rendezvous_default_params with fields overridden by keyword: shortlist=, k=, min_sep= (of .team), max_distance="""
    p = RendezvousParamsC()
    lib.lins_rendezvous_default_params.argtypes = [C.POINTER(RendezvousParamsC)]
    lib.lins_rendezvous_default_params.restype = None
    lib.lins_rendezvous_default_params(C.byref(p))
    for k, v in kw.items():
        if k == "max_distance":
            p.max_distance = v
        elif hasattr(p.team, k):
            setattr(p.team, k, v)
        else:
            raise TypeError(f"lins_rendezvous_params has no field {k}")
    return p


# ---- rendezvous over a window (include/lins_team.h; the consensus records are include/lins_host.h's) ----
RENDEZVOUS_UNCONFIRMED = 3
RENDEZVOUS_MAX_WINDOW, RENDEZVOUS_MAX_HYP = 16, 128


class ConsensusHypC(C.Structure):
    _fields_ = [("X", C.c_double * 16), ("p", C.c_double * 3), ("fitness", C.c_double), ("query", C.c_int32), ("rank", C.c_int32),
                ("target_slot", C.c_int32), ("admissible", C.c_int32)]


class ConsensusParamsC(C.Structure):
    _fields_ = [("window", C.c_int32), ("stride", C.c_int32), ("min_support", C.c_int32), ("reserved", C.c_int32),
                ("max_translation", C.c_double), ("min_cos_rotation", C.c_double)]


class ConsensusResultC(C.Structure):
    _fields_ = [("winner", C.c_int32), ("support", C.c_int32), ("n_admissible", C.c_int32), ("reserved", C.c_int32), ("members", C.c_uint32 * 4)]

    def as_dict(self):
        return dict(winner=int(self.winner), support=int(self.support), n_admissible=int(self.n_admissible), members=members_of(self.members))


def members_of(words):
    """the set bits of a 128-bit member mask, ascending"""
    return [h for h in range(RENDEZVOUS_MAX_HYP) if (int(words[h >> 5]) >> (h & 31)) & 1]


class RendezvousHypothesisC(C.Structure):
    _fields_ = [("query", C.c_int32), ("rank", C.c_int32), ("admissible", C.c_int32), ("member", C.c_int32), ("cand", PlaceTeamResultC),
                ("target", SubmapInfoC), ("icp", LoopIcpResultC)]

    def as_dict(self):
        return dict(query=int(self.query), rank=int(self.rank), admissible=int(self.admissible), member=int(self.member), cand=self.cand.as_dict(),
                    target=self.target.as_dict(), icp=self.icp.as_dict())


class RendezvousWindowResultC(C.Structure):
    _fields_ = [("outcome", C.c_int32), ("status", C.c_int32), ("n_queries", C.c_int32), ("n_hypotheses", C.c_int32), ("winner", C.c_int32),
                ("support", C.c_int32), ("n_admissible", C.c_int32), ("target_slot", C.c_int32), ("target_id", C.c_int32), ("reserved", C.c_int32),
                ("members", C.c_uint32 * 4), ("query_id", C.c_int32 * RENDEZVOUS_MAX_WINDOW), ("n_ranks", C.c_int32 * RENDEZVOUS_MAX_WINDOW),
                ("source", SubmapInfoC * RENDEZVOUS_MAX_WINDOW), ("X", C.c_double * 16)]

    def as_dict(self):
        nq = int(self.n_queries)
        return dict(outcome=int(self.outcome), status=int(self.status), n_queries=nq, n_hypotheses=int(self.n_hypotheses), winner=int(self.winner),
                    support=int(self.support), n_admissible=int(self.n_admissible), target_slot=int(self.target_slot), target_id=int(self.target_id),
                    members=members_of(self.members), query_id=[int(self.query_id[j]) for j in range(nq)],
                    n_ranks=[int(self.n_ranks[j]) for j in range(nq)], source=[self.source[j].as_dict() for j in range(nq)],
                    X=np.array(self.X[:], np.float64).reshape(4, 4))


def consensus_params(lib, **kw):
    """lins_rendezvous_consensus_default_params of library `lib` (window 5, stride 1, min_support 3, max_translation 1.0,
    min_cos_rotation cos 5 degrees) with fields overridden by keyword"""
    p = ConsensusParamsC()
    lib.lins_rendezvous_consensus_default_params.argtypes = [C.POINTER(ConsensusParamsC)]
    lib.lins_rendezvous_consensus_default_params.restype = None
    lib.lins_rendezvous_consensus_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"lins_consensus_params has no field {k}")
        setattr(p, k, v)
    return p


def consensus_table(hyps):
    """[dict(X, p, fitness, query, rank, target_slot, admissible)] -> a ConsensusHypC array (at least one element)"""
    arr = (ConsensusHypC * max(len(hyps), 1))()
    for i, h in enumerate(hyps):
        arr[i].X[:] = [float(v) for v in np.asarray(h["X"], np.float64).reshape(16)]
        arr[i].p[:] = [float(v) for v in np.asarray(h["p"], np.float64).reshape(3)]
        arr[i].fitness = float(h["fitness"])
        arr[i].query, arr[i].rank, arr[i].target_slot, arr[i].admissible = int(h["query"]), int(h["rank"]), int(h["target_slot"]), int(h["admissible"])
    return arr


# ---- stream snapshots (include/lins_snapshot.h): the blob's header and records, the plan's records ----
SNAPSHOT_MAGIC, SNAPSHOT_VERSION = 0x3150414E534E494C, 1
SNAP_STREAM, SNAP_FILTER, SNAP_BOOT, SNAP_ODOM, SNAP_MAP_POSE, SNAP_RING, SNAP_ARCHIVE, SNAP_GRAPH = (1 << k for k in range(8))
SNAP_SECTIONS, SNAP_FIRST_DEVICE_SEC, SNAP_FIRST_UNIT8_SEC = 14, 5, 9
SNAP_SEC_NAMES = ("stream_rec", "surround", "ring_meta", "ar_meta", "pg_host", "scan_pts", "outl_pts", "ring_pts", "ar_pts", "filter_rows",
                  "boot_pre", "odom", "map_pose", "pg_d")
SNAP_BUFFERS, SNAP_FIRST_UNIT8_BUF = 13, 4


class _FilterParamsC(C.Structure):  # lins_filter_params (host.FilterParams has the same layout)
    _fields_ = [("acc_n", C.c_double), ("gyr_n", C.c_double), ("acc_w", C.c_double), ("gyr_w", C.c_double), ("init_pos_std", C.c_double * 3),
                ("init_vel_std", C.c_double * 3), ("init_att_std", C.c_double * 3), ("init_acc_std", C.c_double * 3), ("init_gyr_std", C.c_double * 3)]


class _BootParamsC(C.Structure):
    _fields_ = [("filter", _FilterParamsC), ("init_ba", C.c_double * 3), ("init_bw", C.c_double * 3)]


class SnapshotCountsC(C.Structure):
    _fields_ = [("has_scan", C.c_int32), ("less_sharp", C.c_int32), ("less_flat", C.c_int32), ("outliers", C.c_int32), ("ring_frames", C.c_int32),
                ("archive_frames", C.c_int32), ("ring_points", C.c_int64), ("archive_points", C.c_int64), ("graph_frames", C.c_int32),
                ("graph_loops", C.c_int32), ("graph_up_frames", C.c_int32), ("surround", C.c_int32)]


class SnapshotFactsC(C.Structure):
    _fields_ = [("params", Params), ("boot", _BootParamsC), ("machine", C.c_int32), ("loop", C.c_int32), ("surround", C.c_int32),
                ("ring_window", C.c_int32), ("map_interval", C.c_double), ("surround_radius", C.c_float), ("surround_pose_leaf", C.c_float)]


class SnapshotInfoC(C.Structure):
    _fields_ = [("magic", C.c_uint64), ("version", C.c_uint32), ("header_bytes", C.c_uint32), ("total_bytes", C.c_uint64), ("checksum", C.c_uint64),
                ("modules", C.c_uint32), ("n_sections", C.c_uint32), ("counts", SnapshotCountsC), ("facts", SnapshotFactsC),
                ("header_checksum", C.c_uint64)]

    def as_dict(self):
        c, f = self.counts, self.facts
        return dict(version=int(self.version), total_bytes=int(self.total_bytes), modules=int(self.modules),
                    counts={n: int(getattr(c, n)) for n, _ in SnapshotCountsC._fields_},
                    facts=dict(num_iter=int(f.params.num_iter), machine=int(f.machine), loop=int(f.loop), surround=int(f.surround),
                               ring_window=int(f.ring_window), map_interval=float(f.map_interval), surround_radius=float(f.surround_radius),
                               surround_pose_leaf=float(f.surround_pose_leaf)))


class SnapshotDirentC(C.Structure):
    _fields_ = [("id", C.c_uint32), ("unit", C.c_uint32), ("offset", C.c_uint64), ("bytes", C.c_uint64)]


class SnapshotStreamRecC(C.Structure):
    _fields_ = [("outl_put", C.c_int32), ("filter_set", C.c_int32), ("status", C.c_int32), ("imu_seen", C.c_int32), ("filter_prm", _FilterParamsC),
                ("imu_last", C.c_double * 6), ("map_last_time", C.c_double), ("centre", C.c_float * 3), ("stepped", C.c_int32),
                ("last6", C.c_float * 6), ("reserved", C.c_int64)]


class SnapshotFrameC(C.Structure):
    _fields_ = [("n", C.c_int32 * 3), ("reserved", C.c_int32), ("pose", C.c_float * 6), ("t", C.c_float * 9), ("reserved2", C.c_float),
                ("time", C.c_double)]


class SnapshotLoopC(C.Structure):
    _fields_ = [("Z", C.c_double * 12), ("var", C.c_double), ("latest", C.c_int32), ("closest", C.c_int32)]


class SnapshotLimitsC(C.Structure):
    _fields_ = [("modules", C.c_uint32), ("less_sharp_max", C.c_int32), ("less_flat_max", C.c_int32), ("outlier_max", C.c_int32),
                ("ring_window", C.c_int32), ("ring_max_pts", C.c_int32), ("archive_frames", C.c_int32), ("graph_frames", C.c_int32),
                ("graph_loops", C.c_int32), ("surround_max", C.c_int32), ("archive_points", C.c_int64)]


class SnapshotPlaceC(C.Structure):
    _fields_ = [("row", C.c_int64), ("scan_off", C.c_int64 * 2), ("outl_off", C.c_int64), ("graph_off", C.c_int64), ("ring_off", C.c_void_p),
                ("ar_off", C.c_void_p), ("ring_n", C.c_void_p), ("ar_n", C.c_void_p)]


class SnapshotSegmentC(C.Structure):
    _fields_ = [("buffer", C.c_int32), ("unit", C.c_int32), ("buf_off", C.c_int64), ("stg_off", C.c_int64), ("units", C.c_int64)]
