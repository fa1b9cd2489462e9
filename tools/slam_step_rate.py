#!/usr/bin/env python3
"""lins_streams_slam_step against the chain it replaces; profiles/slam_step_rate.txt keeps one run.

The chain, per sweep: lins_streams_process_raw with the global states downloaded, lins_host_odom_from_global per RUNNING
stream, lins_streams_map_step with those rows, lins_map_associate_batch for the fusion.  The poses the fusion needs are
read with lins_streams_map_get_pose, one call per RUNNING stream: given apart, as a second figure of the chain, since a
caller could keep them itself; lins_host_pose_quat is not counted.  Per stream count --runs runs from fresh state, two
contexts in ONE process taking the same sweeps, alternating — which side goes first changes from sweep to sweep and from
run to run; the clock runs inside the library calls only (arguments are marshalled before it starts).  A run's figure is
the time of its sweeps from the second on (the sweeps with mapping work), per sweep; median of the runs with min .. max.

    python tools/slam_step_rate.py [--streams 64 256] [--out profiles/slam_step_rate.txt]
"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "lins---lidar-inertial-slam_amd"
RUNNING = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=6)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slam_step_rate.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g

    g.build()
    pkg, host, ieskf, sm, sl, defs = (importlib.import_module(PKG + m) for m in ("", ".host", ".ieskf", ".streams_map", ".streams_slam", "._ctypes_defs"))
    import boot_common as bc

    L, H = ieskf.lib(), host.lib()
    dp, ip, pp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(host.Point)
    L.lins_streams_slam_step.argtypes = [C.c_void_p, C.POINTER(pp), ip, ip, C.POINTER(dp), dp, dp, C.c_double, C.c_void_p, C.POINTER(ieskf.ResultC), ip,
                                         C.POINTER(defs.MapStepResultC), C.POINTER(defs.FusedPoseC)]
    L.lins_streams_process_raw.argtypes = [C.c_void_p, C.POINTER(pp), ip, ip, C.POINTER(dp), dp, dp, C.c_double, C.POINTER(ieskf.ResultC), ip, dp, ip]
    L.lins_streams_map_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(defs.MapOdomC), C.POINTER(defs.MapStepResultC)]
    L.lins_streams_map_get_pose.argtypes = [C.c_void_p, C.c_int, C.POINTER(defs.MapPoseStateC)]
    L.lins_map_associate_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    H.lins_host_odom_from_global.argtypes, H.lins_host_odom_from_global.restype = [dp, C.POINTER(defs.StreamOdomC)], None

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def clocked(fn, *a):
        t0 = time.perf_counter()
        rc = fn(*a)
        dt = time.perf_counter() - t0
        assert not rc, rc
        return dt

    data = [bc.load(host, s, args.sweeps) for s in bc.SEQS]
    for ns in args.streams:
        seq = [data[i % len(data)] for i in range(ns)]
        per_sweep = dict(one=[], one_dev=[], chain=[], chain_poses=[])
        same = total = 0
        for r in range(args.runs):
            with ieskf.IeskfContext(pkg.default_params(num_iter=8), max_batch=ns, max_targets=16 * 1800) as a, \
                    ieskf.IeskfContext(pkg.default_params(num_iter=8), max_batch=ns, max_targets=16 * 1800) as b:
                for c in (a, b):
                    c.streams_init(ns)
                    c.streams_machine_init()
                    c.local_map_init(ns, args.window, 16384)
                    sm.init(c, ns, 0.0)  # (every sweep passes the interval gate: every sweep has mapping work)
                t_one = t_dev = t_chain = t_poses = 0.0
                for k in range(args.sweeps):
                    raws = [np.ascontiguousarray(s["raws"][k], np.float32).reshape(-1, 4) for s in seq]
                    rptr = (pp * ns)(*[r.ctypes.data_as(pp) for r in raws])
                    rcnt = (C.c_int32 * ns)(*[len(r) for r in raws])
                    cnt, ptrs, _keep = a._imu_args([s["rows"][k] for s in seq])
                    st = np.full(ns, bc.scan_time(k))
                    res, status = (ieskf.ResultC * ns)(), np.zeros(ns, np.int32)
                    mp, fz = (defs.MapStepResultC * ns)(), (defs.FusedPoseC * ns)()

                    def one_call():
                        return clocked(L.lins_streams_slam_step, a._h, rptr, rcnt, cnt, ptrs, dp(), st.ctypes.data_as(dp), 0.1, None, res,
                                       status.ctypes.data_as(ip), mp, fz)

                    res_b, status_b, gs = (ieskf.ResultC * ns)(), np.zeros(ns, np.int32), np.zeros((ns, 19))
                    counts = np.zeros((ns, 4), np.int32)
                    chain_out = {}

                    def chain():
                        """-> (seconds inside the four kinds of call of the chain, seconds inside its pose downloads)"""
                        e = clocked(L.lins_streams_process_raw, b._h, rptr, rcnt, cnt, ptrs, dp(), st.ctypes.data_as(dp), 0.1, res_b,
                                    counts.ctypes.data_as(ip), gs.ctypes.data_as(dp), status_b.ctypes.data_as(ip))
                        g = 0.0
                        run = [i for i in range(ns) if status_b[i] == RUNNING]
                        tm = np.zeros((len(run), 6), np.float32)
                        if run:
                            recs = (defs.StreamOdomC * len(run))()
                            t0 = time.perf_counter()
                            for j, i in enumerate(run):
                                H.lins_host_odom_from_global(gs[i].ctypes.data_as(dp), C.byref(recs[j]))
                            e += time.perf_counter() - t0
                            od = (defs.MapOdomC * len(run))()
                            for j in range(len(run)):
                                od[j].transform_sum[:] = recs[j].transform_sum[:]
                                od[j].time = bc.scan_time(k)
                            sv = np.ascontiguousarray(run, np.int32)
                            mp_b = (defs.MapStepResultC * len(run))()
                            e += clocked(L.lins_streams_map_step, b._h, len(run), sv.ctypes.data, od, mp_b)
                            poses = (defs.MapPoseStateC * len(run))()
                            for j, i in enumerate(run):
                                g += clocked(L.lins_streams_map_get_pose, b._h, int(i), C.byref(poses[j]))
                            bef = np.ascontiguousarray([p.bef[:] for p in poses], np.float32)
                            aft = np.ascontiguousarray([p.aft[:] for p in poses], np.float32)
                            sums = np.ascontiguousarray([recs[j].transform_sum[:] for j in range(len(run))], np.float32)
                            e += clocked(L.lins_map_associate_batch, b._h, len(run), bef.ctypes.data, aft.ctypes.data, sums.ctypes.data, tm.ctypes.data)
                        chain_out["run"], chain_out["tm"] = run, tm
                        return e, g

                    if (r + k) % 2 == 0:  # alternating: which side goes first changes from sweep to sweep and from run to run
                        d = one_call()
                        e, gp = chain()
                    else:
                        e, gp = chain()
                        d = one_call()
                    run, tm = chain_out["run"], chain_out["tm"]
                    ok = list(status) == list(status_b)
                    for j, i in enumerate(run):
                        ok = ok and np.array_equal(np.array(fz[i].transform_mapped[:], np.float32).view(np.int32), tm[j].view(np.int32))
                    same += ok
                    total += 1
                    if k >= 1:
                        t_one += d
                        t_dev += sum(a.streams_stats())  # (front-end + update + re-projection of the one call's streams step)
                        t_chain += e
                        t_poses += gp
                per_sweep["one"].append(t_one * 1e3 / (args.sweeps - 1))
                per_sweep["one_dev"].append(t_dev / (args.sweeps - 1))
                per_sweep["chain"].append(t_chain * 1e3 / (args.sweeps - 1))
                per_sweep["chain_poses"].append((t_chain + t_poses) * 1e3 / (args.sweeps - 1))
        say(f"{ns} streams, {args.sweeps} sweeps from INIT (sequences 11 / 12 / 13 in turn), window {args.window}; status and fused pose equal bit for bit "
            f"in {same} of {total} sweeps")
        for name, v in (("lins_streams_slam_step, inside the call        ", per_sweep["one"]), ("  its streams step on the device (HIP events)  ", per_sweep["one_dev"]),
                        ("the chain, inside its library calls            ", per_sweep["chain"]),
                        ("the chain, its pose downloads counted too      ", per_sweep["chain_poses"])):
            say(f"  {name}: median {statistics.median(v):9.4f} ms per sweep   min {min(v):9.4f}   max {max(v):9.4f}   ({len(v)} runs from fresh state)")
        m_one, m_chain = statistics.median(per_sweep["one"]), statistics.median(per_sweep["chain"])
        spread = max(per_sweep["chain"]) - min(per_sweep["chain"])
        say(f"  one call {m_one:.4f} <= chain {m_chain:.4f} + the chain's own spread {spread:.4f}: {'yes' if m_one <= m_chain + spread else 'NO'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
