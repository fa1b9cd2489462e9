"""Binding of liblins_ieskf.so — the HIP IESKF update path behind the C ABI of
include/lins_ieskf.h.  Host-side mirror of the reference's call surface for this
path (StateEstimator::performIESKF and the two correspondence functions).

There is NO CPU fallback here: a missing library or a missing GPU raises.
"""
import ctypes as C
import os

import numpy as np

from ._ctypes_defs import (CORR_DTYPE, POSE_DTYPE, Params, Point, PoseRecordC, Result, ResultC, ScanPairC, default_params,
                           pairs_to_c)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

EXPORTS = [
    "lins_create", "lins_destroy", "lins_strerror", "lins_last_hip_error", "lins_set_search",
    "lins_ieskf_update", "lins_ieskf_update_batch", "lins_batch_upload", "lins_batch_run", "lins_sync",
    "lins_batch_download", "lins_last_kernel_ms", "lins_batch_bytes_per_iter", "lins_batch_total_iters",
    "lins_correspondences", "lins_reduce_pass", "lins_host_perform_ieskf", "lins_transform_to_end_batch",
    "lins_last_reproject_stats", "lins_icp_update_batch", "lins_extract_features_batch", "lins_last_frontend_stats",
    "lins_streams_init", "lins_streams_step", "lins_streams_stats", "lins_streams_peek", "lins_segment_batch",
    "lins_last_segment_ms", "lins_streams_step_raw", "lins_map_correspondences", "lins_scan2map_batch",
    "lins_last_map_stats", "lins_last_search", "lins_kernel_ms_history", "lins_set_pipelined", "lins_set_launch_queues", "lins_runs_span_ms", "lins_launch_ms_history",
    "lins_rccl_unique_id", "lins_rccl_init", "lins_pose_allgather", "lins_rccl_destroy", "lins_last_index_ms", "lins_last_cut",
    "lins_batch_map", "lins_local_map_init", "lins_local_map_push", "lins_local_map_build", "lins_local_map_push_scans",
    "lins_local_map_set_pose", "lins_local_map_download", "lins_last_local_map_stats",
    "lins_archive_init", "lins_archive_push", "lins_archive_push_scans", "lins_archive_set_poses", "lins_archive_count",
    "lins_archive_select_radius", "lins_archive_find_loop", "lins_archive_assemble", "lins_archive_download",
    "lins_last_archive_stats", "lins_archive_set_scan_chunk",
    "lins_streams_filter_set", "lins_streams_filter_get", "lins_streams_filter_predict", "lins_streams_step_imu",
    "lins_streams_step_imu_raw", "lins_streams_filter_stats",
    "lins_boot_default_params", "lins_streams_machine_init", "lins_streams_process", "lins_streams_process_raw",
    "lins_streams_status", "lins_streams_preintegration_get", "lins_streams_lin_state", "lins_streams_boot_stats",
    "lins_loop_icp_default_params", "lins_loop_icp_batch", "lins_loop_icp_correspondences", "lins_last_loop_icp_stats",
    "lins_segment_batch_outliers", "lins_streams_put_outliers", "lins_streams_map_cloud", "lins_local_map_build_streams",
    "lins_last_local_map_stage_ms",
    "lins_map_associate_batch", "lins_streams_map_init", "lins_streams_map_get_pose", "lins_streams_map_set_pose",
    "lins_streams_map_step", "lins_last_streams_map_ms",
    "lins_streams_odometry", "lins_streams_map_step_resident", "lins_streams_fuse", "lins_streams_slam_step",
    "lins_pose_graph_default_params", "lins_pose_graph_init", "lins_pose_graph_push", "lins_pose_graph_add_loop",
    "lins_pose_graph_solve", "lins_pose_graph_poses", "lins_pose_graph_apply", "lins_pose_graph_count",
    "lins_last_pose_graph_stats", "lins_pose_graph_apply_batch",
    "lins_loop_step_default_params", "lins_loop_step", "lins_loop_closed_cloud", "lins_last_loop_step_stats", "lins_streams_map_loop",
    "lins_local_map_build_surround", "lins_local_map_build_surround_streams", "lins_streams_map_surround", "lins_streams_map_surround_list",
    "lins_keyposes_select_batch", "lins_keyposes_find_loop_batch", "lins_keyposes_surround_batch", "lins_keyposes_set_mode",
    "lins_keyposes_mode", "lins_last_keyposes_stats",
    "lins_rendezvous_consensus_default_params", "lins_rendezvous_consensus_batch", "lins_last_rendezvous_consensus_stats",
    "lins_rendezvous_window_step", "lins_last_rendezvous_window_stats",
]
# the calls of include/lins_lifecycle.h, a list of their own (tests/test_abi_archive.py counts the lins_archive_* calls of
# include/lins_map.h in EXPORTS); lib() resolves every one of them, so a library without them does not load
LIFECYCLE_EXPORTS = [
    "lins_archive_usage", "lins_archive_release_slots", "lins_archive_set_reclaim_chunk", "lins_pose_graph_release_slot",
    "lins_local_map_release_slot", "lins_streams_release", "lins_streams_map_release", "lins_streams_retire", "lins_last_reclaim_stats",
]
# the calls of include/lins_snapshot.h, for the same reason a list of their own; lib() resolves every one of them
SNAPSHOT_EXPORTS = [
    "lins_streams_snapshot_size", "lins_streams_snapshot", "lins_streams_restore", "lins_streams_migrate", "lins_snapshot_info_get",
    "lins_last_snapshot_stats",
]
# the calls of include/lins_place.h, for the same reason a list of their own; lib() resolves every one of them
PLACE_EXPORTS = [
    "lins_place_default_params", "lins_place_init", "lins_place_sync", "lins_place_search_batch", "lins_place_descriptor",
    "lins_place_distances", "lins_place_set_chunk", "lins_last_place_stats", "lins_loop_icp_batch_from",
    "lins_place_topk_batch", "lins_last_place_select_ms", "lins_loop_place_default_params", "lins_loop_step_place",
]
# the calls of include/lins_team.h (team.py wraps them); lib() resolves every one of them
TEAM_EXPORTS = [
    "lins_place_team_default_params", "lins_place_team_topk_batch", "lins_place_team_key", "lins_place_team_set_chunk",
    "lins_last_place_team_stats", "lins_rendezvous_default_params", "lins_rendezvous_step",
    "lins_pose_graph_rebase_batch", "lins_team_rebase",
]
# the team graph's calls (include/lins_team.h lins_team_graph_*; team.py wraps them); lib() resolves every one of them
TEAM_GRAPH_EXPORTS = ["lins_team_factor_from_alignment", "lins_team_graph_solve", "lins_last_team_graph_stats"]
# the pairwise-consistent team factors (include/lins_team.h; team.py wraps them); lib() resolves every one of them
TEAM_PCM_EXPORTS = ["lins_team_pcm_default_params", "lins_team_factors_consistent_batch", "lins_last_team_pcm_stats"]
# the team map's calls (include/lins_map.h; team.py wraps them); lib() resolves every one of them
TEAM_MAP_EXPORTS = [
    "lins_keyposes_team_select_batch", "lins_last_keyposes_team_stats", "lins_local_map_build_team",
    "lins_local_map_build_team_streams", "lins_streams_map_team", "lins_streams_map_team_groups", "lins_streams_map_team_group",
    "lins_streams_map_team_list",
]


class LinsError(RuntimeError):
    pass


class ReprojectJob(C.Structure):
    _fields_ = [("inp", C.c_void_p), ("out_xyz", C.c_void_p), ("out_yzx", C.c_void_p), ("n", C.c_int32),
                ("reserved", C.c_int32), ("t", C.c_double * 3), ("q", C.c_double * 4)]


def lib_path():
    # (LINS_IESKF_LIB: A/B timing of two builds of the library in one GPU call, tools/ab_timing.py)
    return os.environ.get("LINS_IESKF_LIB") or os.path.join(_HERE, "liblins_ieskf.so")


def lib():
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise LinsError(f"{p} is missing: the HIP extension was not built (run __graft_entry__.build()); "
                            "there is no CPU fallback for this path")
        L = C.CDLL(p)
        vp, dp = C.c_void_p, C.POINTER(C.c_double)
        L.lins_create.argtypes = [C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.lins_destroy.argtypes = [vp]
        L.lins_destroy.restype = None
        L.lins_strerror.argtypes = [C.c_int]
        L.lins_strerror.restype = C.c_char_p
        L.lins_last_hip_error.argtypes = [vp]
        L.lins_last_hip_error.restype = C.c_char_p
        L.lins_set_search.argtypes = [vp, C.c_char_p]
        L.lins_ieskf_update.argtypes = [vp, C.POINTER(ScanPairC), C.POINTER(ResultC)]
        L.lins_ieskf_update_batch.argtypes = [vp, C.c_int, C.POINTER(ScanPairC), C.POINTER(ResultC)]
        L.lins_batch_upload.argtypes = [vp, C.c_int, C.POINTER(ScanPairC)]
        L.lins_batch_run.argtypes = [vp, vp, C.c_int32]
        L.lins_sync.argtypes = [vp]
        L.lins_batch_download.argtypes = [vp, C.c_int, C.POINTER(ResultC)]
        L.lins_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.lins_kernel_ms_history.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
        L.lins_last_index_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.lins_set_pipelined.argtypes = [vp, C.c_int]
        L.lins_set_launch_queues.argtypes = [vp, C.c_int]
        L.lins_runs_span_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
        L.lins_launch_ms_history.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
        L.lins_rccl_unique_id.argtypes = [vp, C.c_void_p]
        L.lins_rccl_init.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
        L.lins_pose_allgather.argtypes = [vp, vp, C.c_int, vp]
        L.lins_rccl_destroy.argtypes = [vp]
        L.lins_batch_bytes_per_iter.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.lins_batch_total_iters.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.lins_correspondences.argtypes = [vp, C.POINTER(ScanPairC), dp, C.c_int, vp, vp]
        L.lins_reduce_pass.argtypes = [vp, C.POINTER(ScanPairC), dp, C.c_int, dp, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32)]
        L.lins_host_perform_ieskf.argtypes = [vp, C.POINTER(Params), C.POINTER(ScanPairC), C.POINTER(ResultC),
                                              C.POINTER(C.c_int32)]
        L.lins_icp_update_batch.argtypes = [vp, C.c_int, C.POINTER(ScanPairC), C.POINTER(ResultC)]
        L.lins_transform_to_end_batch.argtypes = [vp, C.c_int, C.POINTER(ReprojectJob)]
        L.lins_last_reproject_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        for name in EXPORTS:
            if name not in ("lins_destroy", "lins_strerror", "lins_last_hip_error", "lins_last_search", "lins_loop_icp_default_params",
                            "lins_boot_default_params", "lins_pose_graph_default_params", "lins_loop_step_default_params",
                            "lins_rendezvous_consensus_default_params"):
                if os.environ.get("LINS_IESKF_LIB") and not hasattr(L, name):
                    continue  # (an older build under A/B timing)
                getattr(L, name).restype = C.c_int
        for name in LIFECYCLE_EXPORTS + SNAPSHOT_EXPORTS + PLACE_EXPORTS + TEAM_EXPORTS + TEAM_MAP_EXPORTS + TEAM_GRAPH_EXPORTS + TEAM_PCM_EXPORTS:
            if os.environ.get("LINS_IESKF_LIB") and not hasattr(L, name):
                continue  # (an older build under A/B timing)
            getattr(L, name).restype = None if name.endswith("_default_params") else C.c_int
        _LIB = L
    return _LIB


class IeskfContext:
    """lins_ctx wrapper: one HIP stream + device arena on one GPU."""

    def __init__(self, params=None, device=0, max_batch=1, max_targets=16384, search="auto"):
        self.params = params if params is not None else default_params()
        self._h = C.c_void_p()
        self._check(lib().lins_create(C.byref(self.params), device, max_batch, max_targets, C.byref(self._h)))
        self.max_batch = max_batch
        self.set_search(search)
        self._n = 0

    def _check(self, rc):
        if rc != 0:
            msg = lib().lins_strerror(rc).decode()
            if rc == -2 and self._h:
                msg += ": " + lib().lins_last_hip_error(self._h).decode()
            raise LinsError(f"liblins_ieskf error {rc}: {msg}")

    def close(self):
        if self._h:
            lib().lins_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_search(self, mode):
        self._check(lib().lins_set_search(self._h, mode.encode()))
        self.search = mode

    # -- StateEstimator::performIESKF ------------------------------------------------
    def update(self, pair):
        c = pair.as_c()
        r = ResultC()
        self._check(lib().lins_ieskf_update(self._h, C.byref(c), C.byref(r)))
        return Result(r)

    def update_batch(self, pairs, arr=None):
        """lins_ieskf_update_batch; `arr`: a prepared ScanPairC array for these pairs (pairs_strided / map_batch)."""
        arr = pairs_to_c(pairs) if arr is None else arr
        res = (ResultC * len(pairs))()
        self._check(lib().lins_ieskf_update_batch(self._h, len(pairs), arr, res))
        return [Result(r) for r in res]

    def map_batch(self, pairs):
        """lins_batch_map for the cloud sizes of `pairs`, then the clouds written into the context's pinned staging arena
        where the library wants them — standing in for a caller whose feature extraction writes there in the first place.
        Returns the ScanPairC array that points at them: passed to upload / update_batch, the library's staging copy is
        skipped."""
        n = len(pairs)
        counts = np.array([[len(p.surf_flat), len(p.corner_sharp), len(p.surf_last), len(p.corner_last)] for p in pairs], dtype=np.int32)
        clouds = (C.POINTER(Point) * (4 * n))()
        self._check(lib().lins_batch_map(self._h, n, counts.ctypes.data_as(C.POINTER(C.c_int32)), clouds))
        arr = pairs_to_c(pairs)
        for i, p in enumerate(pairs):
            for c, (name, src) in enumerate((("surf_flat", p.surf_flat), ("corner_sharp", p.corner_sharp),
                                             ("surf_less_flat_last", p.surf_last), ("corner_less_sharp_last", p.corner_last))):
                if len(src):
                    C.memmove(clouds[4 * i + c], src.ctypes.data, src.nbytes)
                setattr(arr[i], name, clouds[4 * i + c])
        return arr

    def perform_ieskf(self, pair):
        """performIESKF as the node sees it: GPU loop + ICP fallback on divergence."""
        c = pair.as_c()
        r = ResultC()
        used = C.c_int32(0)
        self._check(lib().lins_host_perform_ieskf(self._h, C.byref(self.params), C.byref(c), C.byref(r), C.byref(used)))
        return Result(r), bool(used.value)

    # -- scan-to-map row (include/lins_map.h) -----------------------------------------------------
    def map_correspondences(self, problem):
        from ._ctypes_defs import MAP_CORR_DTYPE, MapProblemC

        c = problem.as_c()
        corner = np.zeros(len(problem.scan_corner), dtype=MAP_CORR_DTYPE)
        surf = np.zeros(len(problem.scan_surf), dtype=MAP_CORR_DTYPE)
        L = lib()
        L.lins_map_correspondences.argtypes = [C.c_void_p, C.POINTER(MapProblemC), C.c_void_p, C.c_void_p]
        self._check(L.lins_map_correspondences(self._h, C.byref(c), corner.ctypes.data, surf.ctypes.data))
        return corner, surf

    def scan2map_batch(self, problems):
        from ._ctypes_defs import MapProblemC, MapResultC

        n = len(problems)
        arr = (MapProblemC * n)(*[p.as_c() for p in problems])
        res = (MapResultC * n)()
        L = lib()
        L.lins_scan2map_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(MapProblemC), C.POINTER(MapResultC)]
        self._check(L.lins_scan2map_batch(self._h, n, arr, res))
        return [dict(transform=np.array(r.transform[:], dtype=np.float32), iters=r.iters, converged=r.converged,
                     degenerate=r.degenerate, n_sel=r.n_sel) for r in res]

    def debug_map_rounds(self, rounds):
        """test aid (lins_debug_map_rounds): scan2map_batch of this context stops after `rounds` rounds (10: as shipped)"""
        L = lib()
        L.lins_debug_map_rounds.argtypes = [C.c_void_p, C.c_int]
        L.lins_debug_map_rounds.restype = C.c_int
        self._check(L.lins_debug_map_rounds(self._h, int(rounds)))

    def map_stats(self):
        ms, q = C.c_float(0), C.c_uint64(0)
        L = lib()
        L.lins_last_map_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        self._check(L.lins_last_map_stats(self._h, C.byref(ms), C.byref(q)))
        return ms.value, q.value

    # -- the mapping node's local map on the device (include/lins_map.h lins_local_map_*) ------------
    def local_map_init(self, n_slots, window=50, max_points_per_frame=16384):
        self._check(lib().lins_local_map_init(self._h, int(n_slots), int(window), int(max_points_per_frame)))

    def local_map_push(self, slot, corner, surf, outlier, pose):
        """one key frame (sensor-frame clouds, pose (x, y, z, roll, pitch, yaw)) onto the ring of `slot`"""
        from ._ctypes_defs import KeyframeC, keyframe_c

        f, _keep = keyframe_c(corner, surf, outlier, pose)
        L = lib()
        L.lins_local_map_push.argtypes = [C.c_void_p, C.c_int, C.POINTER(KeyframeC)]
        self._check(L.lins_local_map_push(self._h, int(slot), C.byref(f)))

    def local_map_build(self, slots, scans):
        """extractSurroundingKeyFrames + downsampleCurrentScan for len(slots) entries; scans: (corner, surf, outlier)
        raw clouds per entry.  Returns the per-entry sizes dicts (n, box_min, box_dim, frames, status)."""
        from ._ctypes_defs import LocalMapSizesC, LocalScanC, local_scan_c

        n = len(slots)
        keep, arr = [], (LocalScanC * max(n, 1))()
        for k, sc in enumerate(scans):
            arr[k], kk = local_scan_c(*sc)
            keep.append(kk)
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        out = (LocalMapSizesC * max(n, 1))()
        L = lib()
        L.lins_local_map_build.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(LocalScanC), C.POINTER(LocalMapSizesC)]
        self._local_sizes = []
        self._check(L.lins_local_map_build(self._h, n, sl.ctypes.data, arr, out))
        self._local_sizes = [out[k].as_dict() for k in range(n)]
        return self._local_sizes

    def local_map_build_streams(self, slots, streams):
        """local_map_build with entry k's scan clouds taken from stream streams[k] where they lie on the device
        (lins_local_map_build_streams).  Returns the per-entry sizes dicts."""
        from ._ctypes_defs import LocalMapSizesC

        n = len(slots)
        assert len(streams) == n
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        stv = np.ascontiguousarray(streams, dtype=np.int32)
        out = (LocalMapSizesC * max(n, 1))()
        L = lib()
        L.lins_local_map_build_streams.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(LocalMapSizesC)]
        self._local_sizes = []
        self._check(L.lins_local_map_build_streams(self._h, n, sl.ctypes.data, stv.ctypes.data, out))
        self._local_sizes = [out[k].as_dict() for k in range(n)]
        return self._local_sizes

    def _surround_build(self, fn, slots, ids, tail_types, tail, per=1):
        """per: ints per list entry (1: ids of the entry's slot; 2: (slot, id) pairs)"""
        from ._ctypes_defs import LocalMapSizesC

        n = len(slots)
        assert len(ids) == n
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        keep = [np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in ids]
        idp = (C.c_void_p * max(n, 1))(*[v.ctypes.data for v in keep])
        idn = np.ascontiguousarray([len(v) // per for v in keep] or [0], dtype=np.int32)
        out = (LocalMapSizesC * max(n, 1))()
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + tail_types + [C.POINTER(LocalMapSizesC)]
        self._local_sizes = []
        self._check(fn(self._h, n, sl.ctypes.data, idp, idn.ctypes.data, *tail, out))
        self._local_sizes = [out[k].as_dict() for k in range(n)]
        return self._local_sizes

    def local_map_build_surround(self, slots, ids, scans):
        """lins_local_map_build_surround: local_map_build with entry k's map side read from the frames ids[k] (in that
        order) of the key-frame archive's slot slots[k] instead of the ring.  Returns the per-entry sizes dicts."""
        from ._ctypes_defs import LocalScanC, local_scan_c

        keep, arr = [], (LocalScanC * max(len(slots), 1))()
        for k, sc in enumerate(scans):
            arr[k], kk = local_scan_c(*sc)
            keep.append(kk)
        return self._surround_build(lib().lins_local_map_build_surround, slots, ids, [C.POINTER(LocalScanC)], [arr])

    def local_map_build_surround_streams(self, slots, ids, streams):
        """lins_local_map_build_surround_streams: the same with the scan clouds taken from streams[k] where they lie"""
        assert len(streams) == len(slots)
        stv = np.ascontiguousarray(streams, dtype=np.int32)
        return self._surround_build(lib().lins_local_map_build_surround_streams, slots, ids, [C.c_void_p], [stv.ctypes.data])

    def local_map_build_team(self, slots, pairs, scans):
        """lins_local_map_build_team: local_map_build_surround with each list entry naming its own archive slot — pairs[k]:
        the (slot, id) pairs of entry k, in list order.  Returns the per-entry sizes dicts."""
        from ._ctypes_defs import LocalScanC, local_scan_c

        keep, arr = [], (LocalScanC * max(len(slots), 1))()
        for k, sc in enumerate(scans):
            arr[k], kk = local_scan_c(*sc)
            keep.append(kk)
        return self._surround_build(lib().lins_local_map_build_team, slots, pairs, [C.POINTER(LocalScanC)], [arr], per=2)

    def local_map_build_team_streams(self, slots, pairs, streams):
        """lins_local_map_build_team_streams: the same with the scan clouds taken from streams[k] where they lie"""
        assert len(streams) == len(slots)
        stv = np.ascontiguousarray(streams, dtype=np.int32)
        return self._surround_build(lib().lins_local_map_build_team_streams, slots, pairs, [C.c_void_p], [stv.ctypes.data], per=2)

    def local_map_stage_ms(self):
        """HIP-event time (ms) of the staging kernel of the last local_map_build_streams"""
        ms = C.c_float(0)
        L = lib()
        L.lins_last_local_map_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(L.lins_last_local_map_stage_ms(self._h, C.byref(ms)))
        return ms.value

    def local_map_push_scans(self, entries, poses):
        """the cornerDS / surfDS / outlierDS of the chosen entries of the last build become key frames of their slots"""
        from ._ctypes_defs import KeyPoseC, key_pose

        n = len(entries)
        e = np.ascontiguousarray(entries, dtype=np.int32)
        ps = (KeyPoseC * max(n, 1))(*[key_pose(p) for p in poses])
        L = lib()
        L.lins_local_map_push_scans.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(KeyPoseC)]
        self._check(L.lins_local_map_push_scans(self._h, n, e.ctypes.data, ps))

    def local_map_set_pose(self, slot, age, pose):
        from ._ctypes_defs import KeyPoseC, key_pose

        p = key_pose(pose)
        L = lib()
        L.lins_local_map_set_pose.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(KeyPoseC)]
        self._check(L.lins_local_map_set_pose(self._h, int(slot), int(age), C.byref(p)))

    def local_map_download(self, entry, which):
        """cloud `which` (LOCAL_*) of entry `entry` of the last build, (n, 4) f32"""
        sizes = getattr(self, "_local_sizes", [])
        cap = sizes[entry]["n"][which] if 0 <= entry < len(sizes) and 0 <= which < 6 else 0
        out = np.zeros((max(cap, 1), 4), np.float32)
        L = lib()
        L.lins_local_map_download.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        rc = L.lins_local_map_download(self._h, int(entry), int(which), out.ctypes.data, int(cap))
        if rc < 0:
            self._check(rc)
        return out[:rc].copy()

    def local_map_stats(self):
        ms, pts = C.c_float(0), C.c_uint64(0)
        L = lib()
        L.lins_last_local_map_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        self._check(L.lins_last_local_map_stats(self._h, C.byref(ms), C.byref(pts)))
        return ms.value, pts.value

    # -- the key-frame archive on the device (include/lins_map.h lins_archive_*) --------------------
    def _rc(self, rc):
        """a call that returns a count / id (>= 0) or an error"""
        if rc < 0:
            self._check(rc)
        return rc

    def archive_init(self, n_slots, max_frames_per_slot, max_points_total):
        L = lib()
        L.lins_archive_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong]
        self._check(L.lins_archive_init(self._h, int(n_slots), int(max_frames_per_slot), int(max_points_total)))

    def archive_push(self, slot, corner, surf, outlier, pose, time=0.0):
        """one key frame behind the frames of `slot`; returns its id"""
        from ._ctypes_defs import KeyframeC, keyframe_c

        f, _keep = keyframe_c(corner, surf, outlier, pose)
        L = lib()
        L.lins_archive_push.argtypes = [C.c_void_p, C.c_int, C.POINTER(KeyframeC), C.c_double]
        return self._rc(L.lins_archive_push(self._h, int(slot), C.byref(f), float(time)))

    def archive_push_scans(self, entries, poses, times):
        """cornerDS / surfDS / outlierDS of entries of the last local_map_build become frames of their slots; returns the ids"""
        from ._ctypes_defs import KeyPoseC, key_pose

        n = len(entries)
        e = np.ascontiguousarray(entries, dtype=np.int32)
        t = np.ascontiguousarray(times, dtype=np.float64)
        ps = (KeyPoseC * max(n, 1))(*[key_pose(p) for p in poses])
        ids = np.full(max(n, 1), -1, np.int32)
        L = lib()
        L.lins_archive_push_scans.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(KeyPoseC), C.c_void_p, C.c_void_p]
        self._check(L.lins_archive_push_scans(self._h, n, e.ctypes.data, ps, t.ctypes.data, ids.ctypes.data))
        return ids[:n].tolist()

    def archive_set_poses(self, slot, first_id, poses):
        """correctPoses: the poses of frames first_id .. first_id + len(poses) - 1 of `slot`"""
        from ._ctypes_defs import KeyPoseC, key_pose

        ps = (KeyPoseC * max(len(poses), 1))(*[key_pose(p) for p in poses])
        L = lib()
        L.lins_archive_set_poses.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(KeyPoseC)]
        self._check(L.lins_archive_set_poses(self._h, int(slot), int(first_id), len(poses), ps))

    def archive_count(self, slot):
        L = lib()
        L.lins_archive_count.argtypes = [C.c_void_p, C.c_int]
        return self._rc(L.lins_archive_count(self._h, int(slot)))

    def archive_select_radius(self, slot, centre, radius, pose_leaf):
        """publishGlobalMap's choice of frames (LM:989-1007): ids in the order the frames are visited"""
        L = lib()
        cap = max(self.archive_count(slot), 1)
        ids = np.zeros(cap, np.int32)
        c = (C.c_float * 3)(*[float(v) for v in centre])
        L.lins_archive_select_radius.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_void_p, C.c_int]
        n = self._rc(L.lins_archive_select_radius(self._h, int(slot), c, float(radius), float(pose_leaf), ids.ctypes.data, cap))
        return ids[:n].copy()

    def archive_find_loop(self, slot, centre, radius, now, min_gap_s):
        """detectLoopClosure's candidate (LM:1050-1067): frame id or -1"""
        L = lib()
        c = (C.c_float * 3)(*[float(v) for v in centre])
        out = C.c_int32(-2)
        L.lins_archive_find_loop.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_double, C.c_double, C.POINTER(C.c_int32)]
        self._check(L.lins_archive_find_loop(self._h, int(slot), c, float(radius), float(now), float(min_gap_s), C.byref(out)))
        return int(out.value)

    def archive_assemble(self, specs):
        """specs: dicts / tuples (slot, ids, clouds, leaf, flags).  Returns the per-spec info dicts (n, frames, points_in,
        box_min, box_dim, status); the clouds stay on the device (archive_download)."""
        from ._ctypes_defs import SubmapInfoC, SubmapSpecC

        n = len(specs)
        arr, keep = (SubmapSpecC * max(n, 1))(), []
        for k, sp in enumerate(specs):
            slot, ids, clouds, leaf, flags = (sp["slot"], sp["ids"], sp["clouds"], sp["leaf"], sp.get("flags", 0)) if isinstance(sp, dict) else sp
            idv = np.ascontiguousarray(ids, dtype=np.int32)
            keep.append(idv)
            arr[k] = SubmapSpecC(idv.ctypes.data_as(C.POINTER(C.c_int32)), len(idv), int(slot), int(clouds), int(flags), float(leaf), 0)
        out = (SubmapInfoC * max(n, 1))()
        L = lib()
        L.lins_archive_assemble.argtypes = [C.c_void_p, C.c_int, C.POINTER(SubmapSpecC), C.POINTER(SubmapInfoC)]
        self._archive_info = []
        self._check(L.lins_archive_assemble(self._h, n, arr, out))
        self._archive_info = [out[k].as_dict() for k in range(n)]
        return self._archive_info

    def archive_download(self, entry):
        """the cloud of entry `entry` of the last assembly, (n, 4) f32"""
        info = getattr(self, "_archive_info", [])
        cap = info[entry]["n"] if 0 <= entry < len(info) else 0
        out = np.zeros((max(cap, 1), 4), np.float32)
        L = lib()
        L.lins_archive_download.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        n = self._rc(L.lins_archive_download(self._h, int(entry), out.ctypes.data, int(cap)))
        return out[:n].copy()

    def archive_stats(self):
        ms, pts = C.c_float(0), C.c_uint64(0)
        L = lib()
        L.lins_last_archive_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        self._check(L.lins_last_archive_stats(self._h, C.byref(ms), C.byref(pts)))
        return ms.value, pts.value

    def archive_set_scan_chunk(self, chunk_tiles):
        """test hook: jobs above chunk_tiles tiles have their scans split over workgroups (0: default, 2**31 - 1: never)"""
        L = lib()
        L.lins_archive_set_scan_chunk.argtypes = [C.c_void_p, C.c_int]
        self._check(L.lins_archive_set_scan_chunk(self._h, int(chunk_tiles)))

    # -- key-pose selection on the device (include/lins_map.h lins_keyposes_*) -----------------------
    def keyposes_select_batch(self, queries, stride=None):
        """lins_archive_select_radius for a batch.  queries: tuples (slot, centre, radius, pose_leaf); stride: ids an entry
        may return (default: the most frames a named slot holds).  Returns (ids, results): per entry its ids (int32 array,
        None with a status) and dict(n, hits, status, host)."""
        from ._ctypes_defs import KeyposesQueryC, KeyposesResultC, keyposes_query

        n = len(queries)
        arr = (KeyposesQueryC * max(n, 1))(*[keyposes_query(*q) for q in queries])
        if stride is None:
            stride = max([self.archive_count(q[0]) for q in queries] + [1])
        ids = np.full((max(n, 1), max(int(stride), 1)), -1, np.int32)
        out = (KeyposesResultC * max(n, 1))()
        L = lib()
        L.lins_keyposes_select_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(KeyposesQueryC), C.c_void_p, C.c_int, C.POINTER(KeyposesResultC)]
        self._check(L.lins_keyposes_select_batch(self._h, n, arr, ids.ctypes.data, int(stride), out))
        res = [out[k].as_dict() for k in range(n)]
        return [None if r["status"] else ids[k, :r["n"]].copy() for k, r in enumerate(res)], res

    def keyposes_find_loop_batch(self, queries):
        """lins_archive_find_loop for a batch.  queries: tuples (slot, centre, radius, now, min_gap_s); returns the ids (-1: none)"""
        from ._ctypes_defs import KeyposesLoopQueryC, keyposes_query

        n = len(queries)
        arr = (KeyposesLoopQueryC * max(n, 1))(*[KeyposesLoopQueryC(keyposes_query(s, c, r, 0.0), float(now), float(gap)) for s, c, r, now, gap in queries])
        out = np.full(max(n, 1), -2, np.int32)
        L = lib()
        L.lins_keyposes_find_loop_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(KeyposesLoopQueryC), C.c_void_p]
        self._check(L.lins_keyposes_find_loop_batch(self._h, n, arr, out.ctypes.data))
        return out[:n].tolist()

    def keyposes_surround_batch(self, queries, lists, stride=None):
        """the selection and the surround list rule in one call.  queries as keyposes_select_batch, lists: per entry the
        list of ids before; stride default: list + frames of the slot.  Returns (lists afterwards — the list before for an
        entry with a status —, results)."""
        from ._ctypes_defs import KeyposesQueryC, KeyposesResultC, keyposes_query

        n = len(queries)
        arr = (KeyposesQueryC * max(n, 1))(*[keyposes_query(*q) for q in queries])
        if stride is None:
            stride = max([self.archive_count(q[0]) + len(l) for q, l in zip(queries, lists)] + [1])
        buf = np.zeros((max(n, 1), max(int(stride), 1)), np.int32)
        cnt = np.zeros(max(n, 1), np.int32)
        for k, l in enumerate(lists):
            buf[k, :len(l)] = np.asarray(l, np.int32)
            cnt[k] = len(l)
        out = (KeyposesResultC * max(n, 1))()
        L = lib()
        L.lins_keyposes_surround_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(KeyposesQueryC), C.c_void_p, C.c_int, C.c_void_p, C.POINTER(KeyposesResultC)]
        self._check(L.lins_keyposes_surround_batch(self._h, n, arr, buf.ctypes.data, int(stride), cnt.ctypes.data, out))
        return [buf[k, :cnt[k]].tolist() for k in range(n)], [out[k].as_dict() for k in range(n)]

    def keyposes_set_mode(self, mode):
        """who selects for the surround step and the loop step: KEYPOSES_HOST (default) or KEYPOSES_DEVICE"""
        L = lib()
        L.lins_keyposes_set_mode.argtypes = [C.c_void_p, C.c_int]
        self._check(L.lins_keyposes_set_mode(self._h, int(mode)))

    def keyposes_mode(self):
        L = lib()
        L.lins_keyposes_mode.argtypes = [C.c_void_p]
        return self._rc(L.lins_keyposes_mode(self._h))

    def keyposes_stats(self):
        """dict(device_ms, host_entries, hits) of the last batched selection"""
        ms, host, hits = C.c_float(0), C.c_int32(0), C.c_uint64(0)
        L = lib()
        L.lins_last_keyposes_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
        self._check(L.lins_last_keyposes_stats(self._h, C.byref(ms), C.byref(host), C.byref(hits)))
        return dict(device_ms=ms.value, host_entries=host.value, hits=hits.value)

    # -- the loop-closure ICP on the device (include/lins_map.h lins_loop_icp_*) ---------------------
    def loop_icp(self, problems, params=None):
        """performLoopClosure's alignment for a batch.  problems: (source, target) pairs, each cloud an int — that entry
        of the last archive_assemble, read on the device where it lies — or an (n, 4) array, uploaded.  params: a
        LoopIcpParamsC (default: lins_loop_icp_default_params).  Returns the per-problem result dicts."""
        from ._ctypes_defs import LoopIcpParamsC, LoopIcpProblemC, LoopIcpResultC, loop_icp_params, loop_icp_problem_c

        L = lib()
        prm = params if params is not None else loop_icp_params(L)
        n = len(problems)
        arr, keep = (LoopIcpProblemC * max(n, 1))(), []
        for k, (s, t) in enumerate(problems):
            arr[k], kk = loop_icp_problem_c(s, t)
            keep.append(kk)
        out = (LoopIcpResultC * max(n, 1))()
        L.lins_loop_icp_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(LoopIcpProblemC), C.POINTER(LoopIcpParamsC), C.POINTER(LoopIcpResultC)]
        self._check(L.lins_loop_icp_batch(self._h, n, arr, C.byref(prm), out))
        return [out[k].as_dict() for k in range(n)]

    def loop_icp_from(self, problems, T0, params=None):
        """lins_loop_icp_batch_from: loop_icp with problem k started from T0[k] (4 x 4, e.g. host.place_guess) instead of
        the identity; returns the C return code as a negative int for a refusal, else the result dicts"""
        from ._ctypes_defs import LoopIcpParamsC, LoopIcpProblemC, LoopIcpResultC, loop_icp_params, loop_icp_problem_c

        L = lib()
        prm = params if params is not None else loop_icp_params(L)
        n = len(problems)
        arr, keep = (LoopIcpProblemC * max(n, 1))(), []
        for k, (s, t) in enumerate(problems):
            arr[k], kk = loop_icp_problem_c(s, t)
            keep.append(kk)
        T = np.ascontiguousarray(T0, np.float64).reshape(n, 16) if n else np.zeros((1, 16))
        out = (LoopIcpResultC * max(n, 1))()
        L.lins_loop_icp_batch_from.argtypes = [C.c_void_p, C.c_int, C.POINTER(LoopIcpProblemC), C.c_void_p, C.POINTER(LoopIcpParamsC),
                                               C.POINTER(LoopIcpResultC)]
        rc = L.lins_loop_icp_batch_from(self._h, n, arr, T.ctypes.data, C.byref(prm), out)
        if rc in (-1, -4):
            return rc
        self._check(rc)
        return [out[k].as_dict() for k in range(n)]

    # -- place recognition over the archive (include/lins_place.h) -----------------------------------
    def place_init(self, **kw):
        """lins_place_init with lins_place_default_params overridden by keyword (up_axis=2, clouds=2, ...); returns the C return code"""
        from ._ctypes_defs import PlaceParamsC, place_params

        L = lib()
        prm = place_params(L, **kw)
        L.lins_place_init.argtypes = [C.c_void_p, C.POINTER(PlaceParamsC)]
        return L.lins_place_init(self._h, C.byref(prm))

    def place_sync(self, slots):
        s = np.ascontiguousarray(slots, np.int32)
        L = lib()
        L.lins_place_sync.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        return L.lins_place_sync(self._h, len(s), s.ctypes.data)

    def place_search(self, queries):
        """queries: tuples (query_slot, query_id, target_slot, now, min_gap_s).  Returns the result dicts (id, shift,
        distance (np.float32), candidates, status), or the C return code (a negative int) of a refused call."""
        from ._ctypes_defs import PlaceQueryC, PlaceResultC, place_query

        n = len(queries)
        arr = (PlaceQueryC * max(n, 1))(*[place_query(*q) for q in queries])
        out = (PlaceResultC * max(n, 1))()
        L = lib()
        L.lins_place_search_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(PlaceQueryC), C.POINTER(PlaceResultC)]
        rc = L.lins_place_search_batch(self._h, n, arr, out)
        if rc in (-1, -4, -6):
            return rc
        self._check(rc)
        return [out[k].as_dict() for k in range(n)]

    def place_topk(self, queries, k, min_sep):
        """lins_place_topk_batch: per query the list of its filled ranks' result dicts (at most k, more than min_sep ids
        apart); an entry without a rank gives [].  `candidates` of the entry is in each of its dicts — and in
        self.place_topk_candidates per entry.  Returns the C return code (a negative int) of a refused call."""
        from ._ctypes_defs import PlaceQueryC, PlaceResultC, place_query

        n = len(queries)
        arr = (PlaceQueryC * max(n, 1))(*[place_query(*q) for q in queries])
        out = (PlaceResultC * max(n * max(int(k), 1), 1))()
        counts = np.zeros(max(n, 1), np.int32)
        L = lib()
        L.lins_place_topk_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(PlaceQueryC), C.c_int, C.c_int, C.POINTER(PlaceResultC), C.c_void_p]
        rc = L.lins_place_topk_batch(self._h, n, arr, int(k), int(min_sep), out, counts.ctypes.data)
        if rc in (-1, -4, -6):
            return rc
        self._check(rc)
        self.place_topk_candidates = [int(out[e * k].candidates) for e in range(n)]
        self.place_topk_raw = [[out[e * k + j].as_dict() for j in range(k)] for e in range(n)]  # (the unfilled ranks too)
        return [[out[e * k + j].as_dict() for j in range(int(counts[e]))] for e in range(n)]

    def place_select_ms(self):
        """HIP-event ms of the select launch of the last place_topk"""
        ms = C.c_float(0)
        L = lib()
        L.lins_last_place_select_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(L.lins_last_place_select_ms(self._h, C.byref(ms)))
        return ms.value

    def place_descriptor(self, slot, id):
        """D[ring][sector] of one frame, (20, 60) f32"""
        out = np.zeros((20, 60), np.float32)
        L = lib()
        L.lins_place_descriptor.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        self._check(L.lins_place_descriptor(self._h, int(slot), int(id), out.ctypes.data))
        return out

    def place_distances(self, query):
        """test aid: one entry's row -> (d, shift) per frame of the target slot (-1, -1: inadmissible)"""
        from ._ctypes_defs import PlaceQueryC, place_query

        q = place_query(*query)
        cap = max(self.archive_count(q.target_slot), 1)
        d, sh = np.zeros(cap, np.float32), np.zeros(cap, np.int32)
        L = lib()
        L.lins_place_distances.argtypes = [C.c_void_p, C.POINTER(PlaceQueryC), C.c_void_p, C.c_void_p, C.c_int]
        n = self._rc(L.lins_place_distances(self._h, C.byref(q), d.ctypes.data, sh.ctypes.data, cap))
        return d[:n].copy(), sh[:n].copy()

    def place_set_chunk(self, chunk):
        """test hook: candidates per workgroup of the search (0: default)"""
        L = lib()
        L.lins_place_set_chunk.argtypes = [C.c_void_p, C.c_int]
        return L.lins_place_set_chunk(self._h, int(chunk))

    def place_stats(self):
        """dict(build_ms, search_ms, pairs, frames_built) of the last place call"""
        b, s, p, f = C.c_float(0), C.c_float(0), C.c_uint64(0), C.c_int32(0)
        L = lib()
        L.lins_last_place_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
        self._check(L.lins_last_place_stats(self._h, C.byref(b), C.byref(s), C.byref(p), C.byref(f)))
        return dict(build_ms=b.value, search_ms=s.value, pairs=p.value, frames_built=f.value)

    def loop_icp_correspondences(self, source, target, T, cap=0.0):
        """one pass of the move + search at T (4 x 4): (idx (-1: none), d) per source point; cap <= 0: no distance cap"""
        from ._ctypes_defs import LoopIcpProblemC, loop_icp_problem_c

        L = lib()
        c, _keep = loop_icp_problem_c(source, target)
        if c.source_entry >= 0:
            info = getattr(self, "_archive_info", [])
            ns = info[c.source_entry]["n"] if c.source_entry < len(info) else 0
        else:
            ns = c.n_source
        idx, d = np.full(max(ns, 1), -2, np.int32), np.zeros(max(ns, 1), np.float32)
        Tm = np.ascontiguousarray(T, np.float64).reshape(16)
        L.lins_loop_icp_correspondences.argtypes = [C.c_void_p, C.POINTER(LoopIcpProblemC), C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        self._check(L.lins_loop_icp_correspondences(self._h, C.byref(c), Tm.ctypes.data, float(cap), idx.ctypes.data, d.ctypes.data))
        return idx[:ns].copy(), d[:ns].copy()

    def loop_icp_stats(self):
        """(HIP-event ms of the last loop_icp / loop_icp_correspondences, query evaluations it did)"""
        ms, q = C.c_float(0), C.c_uint64(0)
        L = lib()
        L.lins_last_loop_icp_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        self._check(L.lins_last_loop_icp_stats(self._h, C.byref(ms), C.byref(q)))
        return ms.value, q.value

    # -- the pose graph on the device (include/lins_map.h lins_pose_graph_*) -------------------------
    def pose_graph_init(self, n_slots, max_frames_per_slot, max_loops_per_slot):
        L = lib()
        L.lins_pose_graph_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        self._check(L.lins_pose_graph_init(self._h, int(n_slots), int(max_frames_per_slot), int(max_loops_per_slot)))

    def pose_graph_push(self, slot, last6, aft6):
        """saveKeyFramesAndFactor's factor: six floats (pitch, yaw, roll, y, z, x) each; returns the frame id"""
        from ._ctypes_defs import six_floats

        L = lib()
        L.lins_pose_graph_push.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        return self._rc(L.lins_pose_graph_push(self._h, int(slot), six_floats(last6) if last6 is not None else None, six_floats(aft6)))

    def pose_graph_add_loop(self, slot, latest_id, closest_id, pose_from, fitness):
        """performLoopClosure's factor: pose_from (x, y, z, roll, pitch, yaw) as host.loop_pose_from returns it"""
        from ._ctypes_defs import KeyPoseC, key_pose

        L, p = lib(), key_pose(pose_from)
        L.lins_pose_graph_add_loop.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(KeyPoseC), C.c_double]
        self._check(L.lins_pose_graph_add_loop(self._h, int(slot), int(latest_id), int(closest_id), C.byref(p), float(fitness)))

    def pose_graph_solve(self, slots, params=None):
        """the batched Levenberg-Marquardt solve of the graphs of `slots`; params: a PoseGraphParamsC (default:
        lins_pose_graph_default_params).  Returns the per-slot result dicts."""
        from ._ctypes_defs import PoseGraphParamsC, PoseGraphResultC, pose_graph_params

        L = lib()
        prm = params if params is not None else pose_graph_params(L)
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        n = len(sl)
        out = (PoseGraphResultC * max(n, 1))()
        L.lins_pose_graph_solve.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(PoseGraphParamsC), C.POINTER(PoseGraphResultC)]
        self._check(L.lins_pose_graph_solve(self._h, n, sl.ctypes.data, C.byref(prm), out))
        return [out[k].as_dict() for k in range(n)]

    def pose_graph_count(self, slot):
        """(frames, loops) of `slot`"""
        L, nl = lib(), C.c_int32(0)
        L.lins_pose_graph_count.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
        n = self._rc(L.lins_pose_graph_count(self._h, int(slot), C.byref(nl)))
        return n, int(nl.value)

    def pose_graph_poses(self, slot, first_id=0, n=None):
        """(n, 6) f32: x, y, z, roll, pitch, yaw (PointTypePose) of frames first_id .. first_id + n - 1"""
        L = lib()
        n = self.pose_graph_count(slot)[0] - first_id if n is None else n
        out = np.zeros((max(n, 1), 6), np.float32)
        L.lins_pose_graph_poses.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        self._check(L.lins_pose_graph_poses(self._h, int(slot), int(first_id), int(n), out.ctypes.data))
        return out[:n]

    def pose_graph_apply(self, slot, stream=-1):
        """correctPoses + LM:1737-1749: the solved poses go to the archive, the local map's ring and (stream >= 0) the
        stream's map pose"""
        L = lib()
        L.lins_pose_graph_apply.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._check(L.lins_pose_graph_apply(self._h, int(slot), int(stream)))

    def pose_graph_apply_batch(self, slots, streams=None):
        """pose_graph_apply for every (slot, stream) pair in one call: every refusal first, the streams' records by one
        kernel behind one upload; streams None: no streams (-1)"""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        st = np.full(len(sl), -1, np.int32) if streams is None else np.ascontiguousarray(streams, dtype=np.int32)
        assert len(sl) == len(st)
        L = lib()
        L.lins_pose_graph_apply_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self._check(L.lins_pose_graph_apply_batch(self._h, len(sl), sl.ctypes.data, st.ctypes.data))

    # -- stream lifecycle (include/lins_lifecycle.h) ----------------------------------------------------
    def _release_list(self, fn, ids):
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self._check(fn(self._h, len(a), a.ctypes.data))

    def archive_usage(self):
        """(points in use, points of capacity) of the archive's arena"""
        L, used, cap = lib(), C.c_longlong(0), C.c_longlong(0)
        L.lins_archive_usage.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        self._check(L.lins_archive_usage(self._h, C.byref(used), C.byref(cap)))
        return int(used.value), int(cap.value)

    def archive_release_slots(self, slots):
        """drop every frame of `slots`, compact the arena on the device; returns the points freed"""
        L, freed = lib(), C.c_longlong(0)
        a = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        L.lins_archive_release_slots.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_longlong)]
        self._check(L.lins_archive_release_slots(self._h, len(a), a.ctypes.data, C.byref(freed)))
        return int(freed.value)

    def archive_set_reclaim_chunk(self, chunk_points):
        """test hook: points moved per compaction pass (0: the default); the results do not depend on it"""
        L = lib()
        L.lins_archive_set_reclaim_chunk.argtypes = [C.c_void_p, C.c_longlong]
        self._check(L.lins_archive_set_reclaim_chunk(self._h, int(chunk_points)))

    def reclaim_stats(self):
        """dict(ms, points_moved, staged_passes, direct_passes) of the last compaction"""
        L = lib()
        ms, moved, st, di = C.c_float(0), C.c_uint64(0), C.c_int32(0), C.c_int32(0)
        L.lins_last_reclaim_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        self._check(L.lins_last_reclaim_stats(self._h, C.byref(ms), C.byref(moved), C.byref(st), C.byref(di)))
        return dict(ms=ms.value, points_moved=int(moved.value), staged_passes=int(st.value), direct_passes=int(di.value))

    def pose_graph_release_slot(self, slot):
        L = lib()
        L.lins_pose_graph_release_slot.argtypes = [C.c_void_p, C.c_int]
        self._check(L.lins_pose_graph_release_slot(self._h, int(slot)))

    def local_map_release_slot(self, slot):
        L = lib()
        L.lins_local_map_release_slot.argtypes = [C.c_void_p, C.c_int]
        self._check(L.lins_local_map_release_slot(self._h, int(slot)))

    def streams_release(self, streams):
        """the filter side of `streams` as lins_streams_init (+ lins_streams_machine_init) leave it"""
        self._release_list(lib().lins_streams_release, streams)

    def streams_map_release(self, streams):
        """the mapping side of `streams` as lins_streams_map_init leaves it"""
        self._release_list(lib().lins_streams_map_release, streams)

    def streams_retire(self, streams):
        """every initialised module's release for stream == slot, one call: the slots are what a fresh init leaves"""
        self._release_list(lib().lins_streams_retire, streams)

    # -- stream snapshots (include/lins_snapshot.h) ------------------------------------------------------
    def streams_snapshot_size(self, streams):
        """bytes the blob of each of `streams` takes now"""
        L = lib()
        a = np.ascontiguousarray(streams, dtype=np.int32).reshape(-1)
        out = np.zeros(max(len(a), 1), np.uint64)
        L.lins_streams_snapshot_size.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self._check(L.lins_streams_snapshot_size(self._h, len(a), a.ctypes.data, out.ctypes.data))
        return [int(x) for x in out[:len(a)]]

    def streams_snapshot(self, streams, caps=None):
        """the blobs of `streams` as a list of bytes objects: plain host memory, the same bytes for the same stream state
        wherever it lives.  caps (a test hook): the capacities offered instead of the sizes asked for."""
        L = lib()
        a = np.ascontiguousarray(streams, dtype=np.int32).reshape(-1)
        n = len(a)
        sizes = self.streams_snapshot_size(a) if caps is None else [int(c) for c in caps]
        bufs = [np.zeros(max(s, 1), np.uint8) for s in sizes]
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
        cap = np.array(sizes + [0] * (1 - min(n, 1)), np.uint64)
        got = np.zeros(max(n, 1), np.uint64)
        L.lins_streams_snapshot.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = L.lins_streams_snapshot(self._h, n, a.ctypes.data, ptrs, cap.ctypes.data, got.ctypes.data)
        self._snapshot_bytes = [int(x) for x in got[:n]]  # (set on LINS_E_CAPACITY too)
        self._check(rc)
        return [bufs[k][:int(got[k])].tobytes() for k in range(n)]

    def streams_restore(self, streams, blobs):
        """blobs[k] (bytes) continues as stream streams[k] of this context; the slot must be what init / release leave"""
        L = lib()
        a = np.ascontiguousarray(streams, dtype=np.int32).reshape(-1)
        n = len(a)
        assert n == len(blobs)
        keep = [np.frombuffer(b, np.uint8) for b in blobs]
        ptrs = (C.c_void_p * max(n, 1))(*[k.ctypes.data if len(k) else None for k in keep])
        sizes = np.array([len(b) for b in blobs] + [0] * (1 - min(n, 1)), np.uint64)
        L.lins_streams_restore.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(L.lins_streams_restore(self._h, n, a.ctypes.data, ptrs, sizes.ctypes.data))

    def streams_migrate(self, stream, dst, dst_stream):
        """snapshot of `stream`, restore into dst_stream of the context dst, retire of `stream` here — dst is asked first"""
        L = lib()
        L.lins_streams_migrate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        self._check(L.lins_streams_migrate(self._h, int(stream), dst._h, int(dst_stream)))

    def snapshot_stats(self):
        """dict(pack_ms, unpack_ms, bytes, segments) of the last snapshot / restore of this context"""
        L = lib()
        p, u, b, s = C.c_float(0), C.c_float(0), C.c_uint64(0), C.c_int32(0)
        L.lins_last_snapshot_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
        self._check(L.lins_last_snapshot_stats(self._h, C.byref(p), C.byref(u), C.byref(b), C.byref(s)))
        return dict(pack_ms=p.value, unpack_ms=u.value, bytes=int(b.value), segments=int(s.value))

    # -- the loop thread's step (include/lins_map.h lins_loop_step) ------------------------------------
    def loop_step(self, entries, params=None):
        """performLoopClosure + correctPoses for the slots named.  entries: LoopStepEntryC (loop_step_entry) or tuples
        (slot, centre, now[, stream]); params: a LoopStepParamsC (default: lins_loop_step_default_params).  Returns the
        per-entry result dicts."""
        from ._ctypes_defs import LoopStepEntryC, LoopStepParamsC, LoopStepResultC, loop_step_entry, loop_step_params

        L = lib()
        prm = params if params is not None else loop_step_params(L)
        n = len(entries)
        arr = (LoopStepEntryC * max(n, 1))(*[e if isinstance(e, LoopStepEntryC) else loop_step_entry(*e) for e in entries])
        out = (LoopStepResultC * max(n, 1))()
        L.lins_loop_step.argtypes = [C.c_void_p, C.c_int, C.POINTER(LoopStepEntryC), C.POINTER(LoopStepParamsC), C.POINTER(LoopStepResultC)]
        self._loop_step_sizes = []
        self._check(L.lins_loop_step(self._h, n, arr, C.byref(prm), out))
        res = [out[k].as_dict() for k in range(n)]
        self._loop_step_sizes = [r["latest"]["n"] for r in res]
        # the step's assembly is the archive's last one: two clouds per entry that had a candidate, in entry order
        self._archive_info = [r[k] for r in res if r["latest"]["frames"] for k in ("latest", "history")]
        return res

    def loop_step_place(self, entries, params=None, place=None):
        """lins_loop_step_place: loop_step with the candidates found by appearance.  place: a LoopPlaceParamsC (default:
        lins_loop_place_default_params).  Returns the per-entry result dicts (step, detect, n_candidates, chosen, cand,
        icp), or the C return code (a negative int) of a refused call."""
        from ._ctypes_defs import (LoopPlaceParamsC, LoopPlaceResultC, LoopStepEntryC, LoopStepParamsC, loop_place_params, loop_step_entry,
                                   loop_step_params)

        L = lib()
        prm = params if params is not None else loop_step_params(L)
        pl = place if place is not None else loop_place_params(L)
        n = len(entries)
        arr = (LoopStepEntryC * max(n, 1))(*[e if isinstance(e, LoopStepEntryC) else loop_step_entry(*e) for e in entries])
        out = (LoopPlaceResultC * max(n, 1))()
        L.lins_loop_step_place.argtypes = [C.c_void_p, C.c_int, C.POINTER(LoopStepEntryC), C.POINTER(LoopStepParamsC), C.POINTER(LoopPlaceParamsC),
                                           C.POINTER(LoopPlaceResultC)]
        self._loop_step_sizes = []
        rc = L.lins_loop_step_place(self._h, n, arr, C.byref(prm), C.byref(pl), out)
        if rc in (-1, -3, -4, -6):
            return rc
        self._check(rc)
        res = [out[k].as_dict() for k in range(n)]
        self._loop_step_sizes = [r["step"]["latest"]["n"] for r in res]
        return res

    def loop_closed_cloud(self, entry):
        """closed_cloud (LM:1143-1154) of an aligned entry of the last loop_step, (n, 4) f32"""
        sizes = getattr(self, "_loop_step_sizes", [])
        cap = sizes[entry] if 0 <= entry < len(sizes) else 0
        out = np.zeros((max(cap, 1), 4), np.float32)
        L = lib()
        L.lins_loop_closed_cloud.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        n = self._rc(L.lins_loop_closed_cloud(self._h, int(entry), out.ctypes.data, int(cap)))
        return out[:n].copy()

    def loop_step_stats(self):
        """dict(assemble_ms, icp_ms, solve_ms, candidates, aligned, closed) of the last loop_step"""
        L = lib()
        ms = [C.c_float(0) for _ in range(3)]
        cnt = [C.c_int32(0) for _ in range(3)]
        L.lins_last_loop_step_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_float)] * 3 + [C.POINTER(C.c_int32)] * 3
        self._check(L.lins_last_loop_step_stats(self._h, *[C.byref(v) for v in ms + cnt]))
        return dict(assemble_ms=ms[0].value, icp_ms=ms[1].value, solve_ms=ms[2].value, candidates=cnt[0].value, aligned=cnt[1].value,
                    closed=cnt[2].value)

    def pose_graph_stats(self):
        """(HIP-event ms of the last pose_graph_solve, trials it ran over all problems)"""
        L = lib()
        ms, it = C.c_float(0), C.c_uint64(0)
        L.lins_last_pose_graph_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        self._check(L.lins_last_pose_graph_stats(self._h, C.byref(ms), C.byref(it)))
        return ms.value, it.value

    def debug_pose_graph_poses_f64(self, slot, first_id=0, n=None):
        """test aid: the estimate in f64, (n, 12): R row-major, t"""
        L = lib()
        n = self.pose_graph_count(slot)[0] - first_id if n is None else n
        out = np.zeros((max(n, 1), 12))
        L.lins_debug_pose_graph_poses_f64.argtypes, L.lins_debug_pose_graph_poses_f64.restype = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p], C.c_int
        self._check(L.lins_debug_pose_graph_poses_f64(self._h, int(slot), int(first_id), int(n), out.ctypes.data))
        return out[:n]

    def debug_pose_graph_loop_z(self, slot, loop):
        L, z = lib(), np.zeros(12)
        L.lins_debug_pose_graph_loop_z.argtypes, L.lins_debug_pose_graph_loop_z.restype = [C.c_void_p, C.c_int, C.c_int, C.c_void_p], C.c_int
        self._check(L.lins_debug_pose_graph_loop_z(self._h, int(slot), int(loop), z.ctypes.data))
        return z

    def _debug_loop_icp(self, name, value):
        f = getattr(lib(), name)
        f.argtypes, f.restype = [C.c_void_p, C.c_int], C.c_int
        self._check(f(self._h, int(value)))

    def debug_loop_icp_rounds(self, rounds):
        """test aid: loop_icp of this context stops every problem after `rounds` rounds (0: off)"""
        self._debug_loop_icp("lins_debug_loop_icp_rounds", rounds)

    def debug_loop_icp_shells(self, shells):
        """test aid: shells a query scans before it is finished by the whole-target scan (0: every query goes that
        way; None: the default).  Same result bits for every value."""
        self._debug_loop_icp("lins_debug_loop_icp_shells", -1 if shells is None else shells)

    def debug_loop_icp_group(self, group):
        """measurement aid: rounds queued between two reads of the "still running" word (0: the default)"""
        self._debug_loop_icp("lins_debug_loop_icp_group", group)

    def debug_loop_icp_last_far(self):
        """queries the last loop_icp / loop_icp_correspondences finished by the whole-target scan"""
        v = C.c_uint32(0)
        L = lib()
        L.lins_debug_loop_icp_last_far.argtypes, L.lins_debug_loop_icp_last_far.restype = [C.c_void_p, C.POINTER(C.c_uint32)], C.c_int
        self._check(L.lins_debug_loop_icp_last_far(self._h, C.byref(v)))
        return int(v.value)

    def debug_loop_icp_step(self, partials, params=None, mode=0, states=None, n_tiles=None, status=None):
        """test aid (lins_debug_loop_icp_step): the device's step kernel on handed-over sums.  partials: (K, tiles, 17)
        f64; n_tiles: per problem, the tiles the kernel adds (default: all); status: per problem, != 0 is not run; states:
        per problem a dict of lins_loop_icp_state fields over a fresh problem.  -> (state dicts, problems still running)"""
        from ._ctypes_defs import LoopIcpParamsC, LoopIcpStateC, loop_icp_params, loop_icp_state

        L = lib()
        p = np.ascontiguousarray(partials, np.float64)
        if p.ndim != 3 or p.shape[2] != 17:
            raise ValueError("partials: (K, tiles, 17)")
        n, bpp = p.shape[:2]
        nt = np.full(n, bpp, np.int32) if n_tiles is None else np.ascontiguousarray(n_tiles, np.int32)
        stt = np.zeros(n, np.int32) if status is None else np.ascontiguousarray(status, np.int32)
        if nt.shape != (n,) or stt.shape != (n,) or (states is not None and len(states) != n):
            raise ValueError("one entry per problem")
        prm = params if params is not None else loop_icp_params(L)
        arr = (LoopIcpStateC * max(n, 1))(*[loop_icp_state(states[k] if states is not None else None) for k in range(n)])
        running = C.c_int32(-1)
        f = L.lins_debug_loop_icp_step
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(LoopIcpParamsC), C.c_int, C.POINTER(LoopIcpStateC),
                      C.POINTER(C.c_int32)]
        f.restype = C.c_int
        self._check(f(self._h, n, bpp, nt.ctypes.data, stt.ctypes.data, p.ctypes.data, C.byref(prm), int(mode), arr, C.byref(running)))
        return [arr[k].as_dict() for k in range(n)], int(running.value)

    def debug_cov_update(self, path, P, sums, r2, diverged=None):
        """test aid (lins_debug_cov_update): the covariance update alone by the program of one update path — path: one of
        _ctypes_defs.COV_PATHS ("lds", "lds1", "mr": that kernel family's joseph_epilogue; "joseph": ieskf_joseph_kernel).
        P: (n, 18, 18) priors, sums: (n, 21) upper triangle of H^T H row by row, r2 = sigma^2, diverged: per case, != 0
        passes the prior through.  One launch, one workgroup per case -> (n, 18, 18)"""
        from ._ctypes_defs import COV_PATHS

        P = np.ascontiguousarray(P, np.float64)
        s = np.ascontiguousarray(sums, np.float64)
        if P.ndim != 3 or P.shape[1:] != (18, 18) or s.shape != (len(P), 21) or len(P) < 1:
            raise ValueError("P: (n, 18, 18), sums: (n, 21)")
        n = len(P)
        div = np.zeros(n, np.int32) if diverged is None else np.ascontiguousarray(diverged, np.int32)
        if div.shape != (n,):
            raise ValueError("one diverged flag per case")
        out = np.zeros((n, 18, 18), np.float64)
        f = lib().lins_debug_cov_update
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        f.restype = C.c_int
        self._check(f(self._h, COV_PATHS.index(path), n, P.ctypes.data, s.ctypes.data, float(r2), div.ctypes.data, out.ctypes.data))
        return out

    # -- image_projection_node on the device: raw clouds -> segmented scans --------------------
    def segment_batch_outliers(self, raws):
        """segment_batch plus the outlier clouds: (list of host.Segmented, list of (n_outlier, 4) f32)."""
        return self.segment_batch(raws, outliers=True)

    def segment_batch(self, raws, outliers=False):
        """raws: list of (n,4) f32 raw clouds in firing order.  Returns a list of host.Segmented."""
        import importlib

        host = importlib.import_module(__package__ + ".host")
        n = len(raws)
        raws = [np.ascontiguousarray(r, dtype=np.float32).reshape(-1, 4) for r in raws]
        ptrs = (C.POINTER(host.Point) * n)(*[r.ctypes.data_as(C.POINTER(host.Point)) for r in raws])
        counts = (C.c_int32 * n)(*[len(r) for r in raws])
        out = (host.SegmentedScanC * n)()
        keep = []
        for k in range(n):
            cloud = np.zeros((host.CLOUD_MAX, 4), np.float32)
            rng = np.zeros(host.CLOUD_MAX, np.float32)
            col = np.zeros(host.CLOUD_MAX, np.uint32)
            ground = np.zeros(host.CLOUD_MAX, np.uint8)
            out[k].cloud = cloud.ctypes.data_as(C.POINTER(host.Point))
            out[k].range = rng.ctypes.data_as(C.POINTER(C.c_float))
            out[k].col = col.ctypes.data_as(C.POINTER(C.c_uint32))
            out[k].ground = ground.ctypes.data_as(C.POINTER(C.c_uint8))
            keep.append((cloud, rng, col, ground))
        L = lib()
        if outliers:
            from ._ctypes_defs import OUTLIER_MAX

            obufs = [np.zeros((OUTLIER_MAX, 4), np.float32) for _ in range(n)]
            optrs = (C.POINTER(host.Point) * n)(*[b.ctypes.data_as(C.POINTER(host.Point)) for b in obufs])
            L.lins_segment_batch_outliers.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(host.Point)), C.POINTER(C.c_int32),
                                                      C.POINTER(host.SegmentedScanC), C.POINTER(C.POINTER(host.Point))]
            self._check(L.lins_segment_batch_outliers(self._h, n, ptrs, counts, out, optrs))
        else:
            L.lins_segment_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(host.Point)), C.POINTER(C.c_int32),
                                             C.POINTER(host.SegmentedScanC)]
            self._check(L.lins_segment_batch(self._h, n, ptrs, counts, out))
        res = []
        for k in range(n):
            c = host.SegmentedScanC()
            C.memmove(C.byref(c), C.byref(out[k]), C.sizeof(c))
            res.append(host.Segmented(*keep[k], c))
        if outliers:
            return res, [obufs[k][: res[k].c.n_outlier].copy() for k in range(n)]
        return res

    def segment_ms(self):
        ms = C.c_float(0)
        L = lib()
        L.lins_last_segment_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(L.lins_last_segment_ms(self._h, C.byref(ms)))
        return ms.value

    # -- StateEstimator's feature front-end on the device (undistortPcl .. extractFeatures) ----
    def extract_features_batch(self, segs, scan_period=0.1):
        """segs: list of host.Segmented.  Returns a list of dicts like host.frontend_extract()."""
        import importlib

        host = importlib.import_module(__package__ + ".host")
        n = len(segs)
        arr = (host.SegmentedScanC * n)(*[s.c for s in segs])
        feats = (host.Features * n)()
        keep = []
        for k in range(n):
            f, bufs = host._features_buffers()
            feats[k] = f
            keep.append(bufs)
        L = lib()
        L.lins_extract_features_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(host.SegmentedScanC), C.c_double,
                                                  C.POINTER(host.Features)]
        self._check(L.lins_extract_features_batch(self._h, n, arr, scan_period, feats))
        return [host._features_dict(feats[k], keep[k]) for k in range(n)]

    def frontend_stats(self):
        ms, b = C.c_float(0), C.c_uint64(0)
        L = lib()
        L.lins_last_frontend_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        self._check(L.lins_last_frontend_stats(self._h, C.byref(ms), C.byref(b)))
        return ms.value, b.value

    # -- device-resident streams: front-end -> update -> re-projection per scan -----------
    def streams_init(self, n):
        L = lib()
        L.lins_streams_init.argtypes = [C.c_void_p, C.c_int]
        self._check(L.lins_streams_init(self._h, n))
        self._streams = n

    def streams_step(self, segs, prior_state, prior_cov, scan_period=0.1):
        """segs: one host.Segmented per stream; prior_state (n,19), prior_cov (n,18,18).
        Returns (results, feature_counts (n,4) = sharp, less sharp, flat, less flat)."""
        import importlib

        host = importlib.import_module(__package__ + ".host")
        n = self._streams
        assert len(segs) == n
        arr = (host.SegmentedScanC * n)(*[s.c for s in segs])
        ps = np.ascontiguousarray(prior_state, dtype=np.float64).reshape(n, 19)
        pc = np.ascontiguousarray(prior_cov, dtype=np.float64).reshape(n, 324)
        res = (ResultC * n)()
        counts = np.zeros((n, 4), np.int32)
        L = lib()
        L.lins_streams_step.argtypes = [C.c_void_p, C.POINTER(host.SegmentedScanC), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), C.c_double, C.POINTER(ResultC), C.POINTER(C.c_int32)]
        self._check(L.lins_streams_step(self._h, arr, ps.ctypes.data_as(C.POINTER(C.c_double)),
                                        pc.ctypes.data_as(C.POINTER(C.c_double)), scan_period, res,
                                        counts.ctypes.data_as(C.POINTER(C.c_int32))))
        self._n = 0
        return [Result(r) for r in res], counts

    def streams_step_raw(self, raws, prior_state, prior_cov, scan_period=0.1):
        """Like streams_step, from raw clouds (firing order): image projection / segmentation on the device too."""
        import importlib

        host = importlib.import_module(__package__ + ".host")
        n = self._streams
        assert len(raws) == n
        raws = [np.ascontiguousarray(r, dtype=np.float32).reshape(-1, 4) for r in raws]
        ptrs = (C.POINTER(host.Point) * n)(*[r.ctypes.data_as(C.POINTER(host.Point)) for r in raws])
        cnts = (C.c_int32 * n)(*[len(r) for r in raws])
        ps = np.ascontiguousarray(prior_state, dtype=np.float64).reshape(n, 19)
        pc = np.ascontiguousarray(prior_cov, dtype=np.float64).reshape(n, 324)
        res = (ResultC * n)()
        counts = np.zeros((n, 4), np.int32)
        L = lib()
        L.lins_streams_step_raw.argtypes = [C.c_void_p, C.POINTER(C.POINTER(host.Point)), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(ResultC),
                                            C.POINTER(C.c_int32)]
        self._check(L.lins_streams_step_raw(self._h, ptrs, cnts, ps.ctypes.data_as(C.POINTER(C.c_double)),
                                            pc.ctypes.data_as(C.POINTER(C.c_double)), scan_period, res,
                                            counts.ctypes.data_as(C.POINTER(C.c_int32))))
        self._n = 0
        return [Result(r) for r in res], counts

    # -- the streams' filter on the device: IMU propagation, update from the resident prior, reset, global pose ------
    def streams_filter_set(self, stream, filt, global_state):
        """filt: a host.Filter; global_state: globalState_ (19,)"""
        g = np.ascontiguousarray(global_state, dtype=np.float64).reshape(19)
        L = lib()
        L.lins_streams_filter_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        self._check(L.lins_streams_filter_set(self._h, stream, C.byref(filt), g.ctypes.data_as(C.POINTER(C.c_double))))

    def streams_filter_get(self, stream):
        """-> (host.Filter, globalState_ (19,)) of one stream (synchronises)"""
        import importlib

        host = importlib.import_module(__package__ + ".host")
        filt, g = host.Filter(), np.zeros(19)
        L = lib()
        L.lins_streams_filter_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        self._check(L.lins_streams_filter_get(self._h, stream, C.byref(filt), g.ctypes.data_as(C.POINTER(C.c_double))))
        return filt, g

    def _imu_args(self, imu):
        """imu: per stream an (m, 7) array of rows (dt, acc, gyr), m may be 0 -> (counts, pointers, keep-alive)"""
        n = self._streams
        assert len(imu) == n
        rows = [np.ascontiguousarray(r, dtype=np.float64).reshape(-1, 7) for r in imu]
        dp = C.POINTER(C.c_double)
        ptrs = (dp * n)(*[r.ctypes.data_as(dp) if len(r) else dp() for r in rows])
        return (C.c_int32 * n)(*[len(r) for r in rows]), ptrs, rows

    def streams_filter_predict(self, imu):
        """StatePredictor::predict of every stream over its own IMU rows (see _imu_args), one launch."""
        cnt, ptrs, _keep = self._imu_args(imu)
        L = lib()
        L.lins_streams_filter_predict.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_double))]
        self._check(L.lins_streams_filter_predict(self._h, cnt, ptrs))

    def streams_step_imu(self, segs, imu, scan_period=0.1):
        """streams_step with the prior from the device filter, propagated over `imu` first.
        Returns (results, feature_counts (n, 4), global states (n, 19))."""
        import importlib

        host = importlib.import_module(__package__ + ".host")
        n = self._streams
        assert len(segs) == n
        arr = (host.SegmentedScanC * n)(*[s.c for s in segs])
        cnt, ptrs, _keep = self._imu_args(imu)
        res = (ResultC * n)()
        counts, g = np.zeros((n, 4), np.int32), np.zeros((n, 19))
        L = lib()
        L.lins_streams_step_imu.argtypes = [C.c_void_p, C.POINTER(host.SegmentedScanC), C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_double)),
                                            C.c_double, C.POINTER(ResultC), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
        self._check(L.lins_streams_step_imu(self._h, arr, cnt, ptrs, scan_period, res, counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                            g.ctypes.data_as(C.POINTER(C.c_double))))
        self._n = 0
        return [Result(r) for r in res], counts, g

    def streams_step_imu_raw(self, raws, imu, scan_period=0.1):
        """Like streams_step_imu, from raw clouds (firing order)."""
        import importlib

        host = importlib.import_module(__package__ + ".host")
        n = self._streams
        assert len(raws) == n
        raws = [np.ascontiguousarray(r, dtype=np.float32).reshape(-1, 4) for r in raws]
        rptrs = (C.POINTER(host.Point) * n)(*[r.ctypes.data_as(C.POINTER(host.Point)) for r in raws])
        rcnt = (C.c_int32 * n)(*[len(r) for r in raws])
        cnt, ptrs, _keep = self._imu_args(imu)
        res = (ResultC * n)()
        counts, g = np.zeros((n, 4), np.int32), np.zeros((n, 19))
        L = lib()
        L.lins_streams_step_imu_raw.argtypes = [C.c_void_p, C.POINTER(C.POINTER(host.Point)), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                C.POINTER(C.POINTER(C.c_double)), C.c_double, C.POINTER(ResultC), C.POINTER(C.c_int32),
                                                C.POINTER(C.c_double)]
        self._check(L.lins_streams_step_imu_raw(self._h, rptrs, rcnt, cnt, ptrs, scan_period, res,
                                                counts.ctypes.data_as(C.POINTER(C.c_int32)), g.ctypes.data_as(C.POINTER(C.c_double))))
        self._n = 0
        return [Result(r) for r in res], counts, g

    # -- the streams' state machine: INIT -> FIRST_SCAN -> RUNNING on the device (lins_streams_machine_init, _process*) ----
    def streams_machine_init(self, boot_params=None):
        """every stream to INIT; boot_params: a host.BootParams (default: lins_boot_default_params)"""
        import importlib

        host = importlib.import_module(__package__ + ".host")
        L = lib()
        if boot_params is None:
            boot_params = host.BootParams()
            L.lins_boot_default_params.argtypes = [C.c_void_p]
            L.lins_boot_default_params.restype = None
            L.lins_boot_default_params(C.byref(boot_params))
        L.lins_streams_machine_init.argtypes = [C.c_void_p, C.c_void_p]
        self._check(L.lins_streams_machine_init(self._h, C.byref(boot_params)))

    def _process(self, fn, head_types, head, imu, scan_time, scan_imu, scan_period):
        n = self._streams
        cnt, ptrs, _keep = self._imu_args(imu)
        dp = C.POINTER(C.c_double)
        st = np.ascontiguousarray(scan_time, dtype=np.float64).reshape(n)
        si = None if scan_imu is None else np.ascontiguousarray(scan_imu, dtype=np.float64).reshape(n, 6)
        res = (ResultC * n)()
        counts, g, status = np.zeros((n, 4), np.int32), np.zeros((n, 19)), np.zeros(n, np.int32)
        fn.argtypes = [C.c_void_p] + head_types + [C.POINTER(C.c_int32), C.POINTER(dp), dp, dp, C.c_double, C.POINTER(ResultC),
                                                   C.POINTER(C.c_int32), dp, C.POINTER(C.c_int32)]
        self._check(fn(self._h, *head, cnt, ptrs, si.ctypes.data_as(dp) if si is not None else dp(), st.ctypes.data_as(dp), scan_period, res,
                       counts.ctypes.data_as(C.POINTER(C.c_int32)), g.ctypes.data_as(dp), status.ctypes.data_as(C.POINTER(C.c_int32))))
        self._n = 0
        return [Result(r) for r in res], counts, g, status

    def streams_process(self, segs, imu, scan_time, scan_imu=None, scan_period=0.1):
        """processImu over each stream's rows (see _imu_args), then processPCL of its segmented scan, whatever the stream's
        status.  scan_imu: (n, 6) imu_last_ or None (the last row given).  Returns (results, feature_counts (n, 4), global
        states (n, 19), status (n,))."""
        import importlib

        host = importlib.import_module(__package__ + ".host")
        n = self._streams
        assert len(segs) == n
        arr = (host.SegmentedScanC * n)(*[s.c for s in segs])
        return self._process(lib().lins_streams_process, [C.POINTER(host.SegmentedScanC)], [arr], imu, scan_time, scan_imu, scan_period)

    def streams_process_raw(self, raws, imu, scan_time, scan_imu=None, scan_period=0.1):
        """Like streams_process, from raw clouds (firing order)."""
        import importlib

        host = importlib.import_module(__package__ + ".host")
        n = self._streams
        assert len(raws) == n
        raws = [np.ascontiguousarray(r, dtype=np.float32).reshape(-1, 4) for r in raws]
        rptrs = (C.POINTER(host.Point) * n)(*[r.ctypes.data_as(C.POINTER(host.Point)) for r in raws])
        rcnt = (C.c_int32 * n)(*[len(r) for r in raws])
        return self._process(lib().lins_streams_process_raw, [C.POINTER(C.POINTER(host.Point)), C.POINTER(C.c_int32)], [rptrs, rcnt], imu,
                             scan_time, scan_imu, scan_period)

    def streams_status(self):
        status = np.zeros(self._streams, np.int32)
        L = lib()
        L.lins_streams_status.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        self._check(L.lins_streams_status(self._h, status.ctypes.data_as(C.POINTER(C.c_int32))))
        return status

    def streams_preintegration_get(self, stream):
        """-> host.Preintegration of a stream in FIRST_SCAN (synchronises)"""
        import importlib

        host = importlib.import_module(__package__ + ".host")
        pre = host.Preintegration()
        L = lib()
        L.lins_streams_preintegration_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self._check(L.lins_streams_preintegration_get(self._h, stream, C.byref(pre)))
        return pre

    def streams_lin_state(self):
        """linState_ of every stream (n, 19) as the last step's re-projection read it"""
        lin = np.zeros((self._streams, 19))
        L = lib()
        L.lins_streams_lin_state.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self._check(L.lins_streams_lin_state(self._h, lin.ctypes.data_as(C.POINTER(C.c_double))))
        return lin

    def streams_boot_stats(self):
        """HIP-event times (ms) of the last call's pre-integration kernel, bootstrap ICP and bootstrap finish kernel"""
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        L = lib()
        L.lins_streams_boot_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_float)] * 3
        self._check(L.lins_streams_boot_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def streams_filter_stats(self):
        """HIP-event times (ms) of the last predict and finish kernels"""
        a, b = C.c_float(0), C.c_float(0)
        L = lib()
        L.lins_streams_filter_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_float)] * 2
        self._check(L.lins_streams_filter_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def streams_stats(self):
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        L = lib()
        L.lins_streams_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_float)] * 3
        self._check(L.lins_streams_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def streams_peek(self, stream, which):
        buf = np.zeros((28800, 4), np.float32)
        L = lib()
        L.lins_streams_peek.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        n = L.lins_streams_peek(self._h, stream, which, buf.ctypes.data, len(buf))
        self._check(min(n, 0))
        return buf[:n].copy()

    def streams_put_outliers(self, outliers):
        """one (m, 4) outlier cloud per stream for the NEXT segmented step (lins_streams_put_outliers)"""
        n = self._streams
        assert len(outliers) == n
        cl = [np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 4) for o in outliers]
        pp = C.POINTER(Point)
        ptrs = (pp * n)(*[c.ctypes.data_as(pp) if len(c) else pp() for c in cl])
        cnt = (C.c_int32 * n)(*[len(c) for c in cl])
        L = lib()
        L.lins_streams_put_outliers.argtypes = [C.c_void_p, C.POINTER(pp), C.POINTER(C.c_int32)]
        self._check(L.lins_streams_put_outliers(self._h, ptrs, cnt))

    def streams_map_cloud(self, stream, which):
        """what the mapping node reads of a stream's last step, in its axes (y, z, x): which = 0 corner last,
        1 surf last, 2 outlier last (lins_streams_map_cloud)"""
        buf = np.zeros((28800, 4), np.float32)
        L = lib()
        L.lins_streams_map_cloud.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        n = L.lins_streams_map_cloud(self._h, stream, which, buf.ctypes.data, len(buf))
        self._check(min(n, 0))
        return buf[:n].copy()

    def icp_update_batch(self, pairs):
        """estimateTransform (the ICP fallback) on the device, from each pair's state pose."""
        arr = pairs_to_c(pairs)
        res = (ResultC * len(pairs))()
        self._check(lib().lins_icp_update_batch(self._h, len(pairs), arr, res))
        self._n = 0
        return [Result(r) for r in res]

    # -- staged batch form -------------------------------------------------------------
    def upload(self, pairs, arr=None):
        arr = pairs_to_c(pairs) if arr is None else arr
        self._check(lib().lins_batch_upload(self._h, len(pairs), arr))
        self._n = len(pairs)

    def run(self, poses_ptr=None, scan_id_base=0):
        self._check(lib().lins_batch_run(self._h, C.c_void_p(poses_ptr) if poses_ptr else None, scan_id_base))

    def sync(self):
        self._check(lib().lins_sync(self._h))

    def download(self, n=None):
        n = self._n if n is None else n
        res = (ResultC * n)()
        self._check(lib().lins_batch_download(self._h, n, res))
        return [Result(r) for r in res]

    def last_kernel_ms(self):
        ms = C.c_float(0)
        self._check(lib().lins_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def last_index_ms(self):
        """HIP-event time (ms) of the search-index build of the last upload (the reference's kd-tree build, SE:1156-1160)."""
        ms = C.c_float(0)
        self._check(lib().lins_last_index_ms(self._h, C.byref(ms)))
        return ms.value

    def last_cut(self):
        """(parts, queue_timeouts): pieces every update of the last run() was cut into (1 = whole updates), and the waits at
        the work queue that ran out over the life of the context (0 in a healthy process)."""
        parts, tail = C.c_int(0), C.c_int(0)
        self._check(lib().lins_last_cut(self._h, C.byref(parts), C.byref(tail)))
        return parts.value, tail.value

    def kernel_ms_history(self, n):
        """HIP-event times (ms) of the update kernels of the last n run() calls, oldest first."""
        ms = (C.c_float * n)()
        self._check(lib().lins_kernel_ms_history(self._h, n, ms))
        return [float(v) for v in ms]

    def set_pipelined(self, on=True):
        """Pipelined staged mode: Joseph kernel / pose gather of run k beside the update kernel of run k + 1."""
        self._check(lib().lins_set_pipelined(self._h, 1 if on else 0))

    def runs_span_ms(self, n):
        """GPU time the last n runs took together (first launch's start to last launch's end, both launch queues)."""
        v = C.c_float(0)
        self._check(lib().lins_runs_span_ms(self._h, int(n), C.byref(v)))
        return float(v.value)

    def launch_ms_history(self, n):
        """durations of the launches of the last n runs, each by its own queue's events: [(first, second or 0.0), ...]"""
        a = (C.c_float * (2 * n))()
        self._check(lib().lins_launch_ms_history(self._h, int(n), a))
        return [(float(a[2 * k]), float(a[2 * k + 1])) for k in range(n)]

    def set_launch_queues(self, queues):
        """2 (default): a batch beyond the device's slots runs as whole-update launches on two streams; 1: one launch, several-part updates."""
        self._check(lib().lins_set_launch_queues(self._h, int(queues)))

    # -- multi-GPU: RCCL all-gather of the pose records through the C ABI (include/lins_ieskf.h) ------
    def rccl_unique_id(self):
        buf = (C.c_char * 128)()
        self._check(lib().lins_rccl_unique_id(self._h, buf))
        return bytes(buf)

    def rccl_init(self, uid, rank, world):
        assert len(uid) == 128
        self._check(lib().lins_rccl_init(self._h, C.c_char_p(uid), rank, world))

    def pose_allgather(self, d_local_ptr, n_records, d_all_ptr):
        self._check(lib().lins_pose_allgather(self._h, C.c_void_p(d_local_ptr), n_records, C.c_void_p(d_all_ptr)))

    def rccl_destroy(self):
        self._check(lib().lins_rccl_destroy(self._h))

    def last_search(self):
        """Kernel family the last batch / pass actually ran (after "auto" and the eligibility fall-backs)."""
        f = lib().lins_last_search
        f.restype = C.c_char_p
        f.argtypes = [C.c_void_p]
        return f(self._h).decode()

    def bytes_per_iter(self):
        b = C.c_uint64(0)
        self._check(lib().lins_batch_bytes_per_iter(self._h, C.byref(b)))
        return b.value

    def total_iters(self):
        b = C.c_uint64(0)
        self._check(lib().lins_batch_total_iters(self._h, C.byref(b)))
        return b.value

    # -- StateEstimator::updatePointCloud's re-projection (transformToEnd) -----------------
    def transform_to_end(self, clouds, poses, yzx=True):
        """clouds: list of (n,4) f32 arrays; poses: list of (t[3], q[4]).  Returns (xyz, yzx) lists."""
        jobs = (ReprojectJob * len(clouds))()
        keep = []
        for k, (cl, (t, q)) in enumerate(zip(clouds, poses)):
            cl = np.ascontiguousarray(cl, dtype=np.float32).reshape(-1, 4)
            o1 = np.empty_like(cl)
            o2 = np.empty_like(cl) if yzx else None
            keep.append((cl, o1, o2))
            jobs[k].inp, jobs[k].out_xyz = cl.ctypes.data, o1.ctypes.data
            jobs[k].out_yzx = o2.ctypes.data if yzx else None
            jobs[k].n = len(cl)
            jobs[k].t[:] = list(t)
            jobs[k].q[:] = list(q)
        self._check(lib().lins_transform_to_end_batch(self._h, len(clouds), jobs))
        self._n = 0
        return [k[1] for k in keep], [k[2] for k in keep]

    def reproject_stats(self):
        ms, b = C.c_float(0), C.c_uint64(0)
        self._check(lib().lins_last_reproject_stats(self._h, C.byref(ms), C.byref(b)))
        return ms.value, b.value

    # -- findCorrespondingSurfFeatures / findCorrespondingCornerFeatures ---------------
    def correspondences(self, pair, lin_state, it):
        c = pair.as_c()
        lin = np.ascontiguousarray(lin_state, dtype=np.float64)
        surf = np.zeros(c.n_surf_flat, dtype=CORR_DTYPE)
        corner = np.zeros(c.n_corner_sharp, dtype=CORR_DTYPE)
        self._check(lib().lins_correspondences(self._h, C.byref(c), lin.ctypes.data_as(C.POINTER(C.c_double)), it,
                                               surf.ctypes.data, corner.ctypes.data))
        return surf, corner

    def reduce_pass(self, pair, lin_state, it):
        c = pair.as_c()
        lin = np.ascontiguousarray(lin_state, dtype=np.float64)
        sums = np.zeros(28)
        ms, mc = C.c_int32(0), C.c_int32(0)
        self._check(lib().lins_reduce_pass(self._h, C.byref(c), lin.ctypes.data_as(C.POINTER(C.c_double)), it,
                                           sums.ctypes.data_as(C.POINTER(C.c_double)), C.byref(ms), C.byref(mc)))
        return sums, ms.value, mc.value


def host_solve_from_sums(params, pair, lin_state, sums):
    """BASELINE.json configs[1]: device correspondences + reduction, host-side
    18x18 solve.  Faithful dense algebra on the 18-state system embedded from the
    28 sums: dx = -W P (g + A d) + d with W = (sigma^2 I + P A)^-1."""
    lin = np.asarray(lin_state, dtype=np.float64)
    filt = pair.state
    P = pair.cov

    def quat2axis(q):
        v = q[1:4]
        m = np.linalg.norm(v)
        if m < 1e-10:
            return v.copy()
        a = 2.0 * np.arctan2(m, q[0])
        a = (a + np.pi) % (2 * np.pi) - np.pi
        return v / m * a

    def qmul(a, b):
        return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                         a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                         a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                         a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])

    ql, qf = lin[6:10], filt[6:10]
    qinv = np.array([ql[0], -ql[1], -ql[2], -ql[3]]) / np.dot(ql, ql)
    d = np.zeros(18)
    d[0:3] = filt[0:3] - lin[0:3]
    d[3:6] = filt[3:6] - lin[3:6]
    d[6:9] = quat2axis(qmul(qinv, qf))
    d[9:12] = filt[10:13] - lin[10:13]
    d[12:15] = filt[13:16] - lin[13:16]
    d[15:18] = filt[16:19] - lin[16:19]
    S = [0, 1, 2, 6, 7, 8]
    A6 = np.zeros((6, 6))
    A6[np.triu_indices(6)] = sums[:21]
    A6 = A6 + np.triu(A6, 1).T
    A = np.zeros((18, 18))
    A[np.ix_(S, S)] = A6
    g = np.zeros(18)
    g[S] = sums[21:27]
    r2 = params.lidar_std ** 2
    W = np.linalg.inv(r2 * np.eye(18) + P @ A)
    dx = -W @ P @ (g + A @ d) + d
    return dx, A, W


def snapshot_info(blob):
    """the header of a snapshot blob (bytes) as a dict, after the whole format check; LinsError when it is refused"""
    from ._ctypes_defs import SnapshotInfoC

    L = lib()
    buf = np.frombuffer(blob, np.uint8)
    out = SnapshotInfoC()
    L.lins_snapshot_info_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(SnapshotInfoC)]
    rc = L.lins_snapshot_info_get(buf.ctypes.data if len(buf) else None, len(buf), C.byref(out))
    if rc != 0:
        raise LinsError(f"liblins_ieskf error {rc}: {L.lins_strerror(rc).decode()}")
    return out.as_dict()
