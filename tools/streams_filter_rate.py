#!/usr/bin/env python3
"""Time per step of n device-resident streams with the filter (a) on the host — lins_filter_predict x 40 and
lins_filter_finish per stream on 16 host threads around lins_streams_step_raw, priors up and posteriors down — and (b) on
the device, lins_streams_step_imu_raw.  Every stream replays synthetic sequence 11 (scan k + 2 in step k) from a filter
started at the trajectory's speed.  Wall-clock medians over --steps steps after --warmup, spread as min .. max; the
predict / finish kernel times are HIP-event times of the same steps.  profiles/streams_filter_rate.txt keeps one run.

    python tools/streams_filter_rate.py [--streams 1 64 1024] [--steps 7] [--warmup 2]
"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "lins---lidar-inertial-slam_amd"
SEQ, DT = 11, 0.1 / 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import __graft_entry__ as g

    g.build()
    pkg, host, ieskf = (importlib.import_module(PKG + m) for m in ("", ".host", ".ieskf"))
    defs = importlib.import_module(PKG + "._ctypes_defs")
    L = host.lib()
    total = args.warmup + args.steps
    raws = [host.synth_seq_raw_scan(SEQ, k) for k in range(1, total + 2)]
    rows = []
    for k in range(1, total + 2):
        acc, gyr = host.synth_seq_imu(SEQ, k)
        rows.append(np.ascontiguousarray(np.hstack([np.full((len(acc), 1), DT), acc, gyr])))
    speed = host.synth_seq_truth(SEQ, 0.2)[3]
    dp = C.POINTER(C.c_double)
    prm = pkg.default_params(num_iter=30)
    pool = ThreadPoolExecutor(16)  # (ctypes calls release the interpreter lock)

    def new_filter():
        fp, f = host.FilterParams(), host.Filter()
        L.lins_filter_default_params(C.byref(fp))
        v, z = np.array([speed, 0.0, 0.0]), np.zeros(3)
        L.lins_filter_init(C.byref(f), C.byref(fp), v.ctypes.data_as(dp), z.ctypes.data_as(dp), z.ctypes.data_as(dp))
        return f

    def boot(ctx, n):
        ctx.streams_init(n)
        s0 = np.zeros(19)
        s0[0], s0[6], s0[18] = speed * 0.1, 1.0, -9.81
        ctx.streams_step_raw([raws[0]] * n, np.tile(s0, (n, 1)), np.tile(np.eye(18)[None] * 1e-4, (n, 1, 1)))

    def report(name, t):
        ms = [x * 1e3 for x in t[args.warmup:]]
        print(f"  {name}: median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f}   max {max(ms):9.3f}   ({len(ms)} steps after {args.warmup} warm-up)")

    res_bytes, raw_bytes = C.sizeof(defs.ResultC), sum(r.nbytes for r in raws[1:]) // total
    for n in args.streams:
        print(f"{n} streams, {raw_bytes} B of raw cloud per stream and step")
        g0 = np.zeros(19)
        g0[6], g0[18] = 1.0, -9.81
        # (a) the filter on the host
        with ieskf.IeskfContext(prm, max_batch=n, max_targets=16 * 1800) as ctx:
            boot(ctx, n)
            filts, gs = [new_filter() for _ in range(n)], [g0.copy() for _ in range(n)]
            t_all, t_host = [], []
            for k in range(total):
                r = rows[k + 1]

                def predict(i):
                    f = filts[i]
                    for row in r:
                        L.lins_filter_predict(C.byref(f), row[0], row[1:4].ctypes.data_as(dp), row[4:7].ctypes.data_as(dp))

                t0 = time.perf_counter()
                list(pool.map(predict, range(n)))
                ps = np.array([f.state[:] for f in filts])
                pc = np.array([f.cov[:] for f in filts])
                t1 = time.perf_counter()
                res, _ = ctx.streams_step_raw([raws[k + 1]] * n, ps, pc)
                t2 = time.perf_counter()

                def finish(i):
                    gs[i] = host.filter_finish(filts[i], gs[i], res[i].state, res[i].cov, used_prior_cov=bool(res[i].diverged))

                list(pool.map(finish, range(n)))
                t3 = time.perf_counter()
                t_all.append(t3 - t0), t_host.append((t1 - t0) + (t3 - t2))
            report("(a) host filter, whole step      ", t_all)
            report("    of which predict + finish    ", t_host)
            print(f"    PCIe per step: up {n * (raw_bytes + (19 + 324) * 8)} B, down {n * res_bytes} B")
        # (b) the filter on the device
        with ieskf.IeskfContext(prm, max_batch=n, max_targets=16 * 1800) as ctx:
            boot(ctx, n)
            f0 = new_filter()
            for i in range(n):
                ctx.streams_filter_set(i, f0, g0)
            t_all, t_pred, t_fin, t_dev = [], [], [], []
            for k in range(total):
                t0 = time.perf_counter()
                res, _, _ = ctx.streams_step_imu_raw([raws[k + 1]] * n, [rows[k + 1]] * n)
                t_all.append(time.perf_counter() - t0)
                pm, fm = ctx.streams_filter_stats()
                t_pred.append(pm * 1e-3), t_fin.append(fm * 1e-3), t_dev.append(sum(ctx.streams_stats()) * 1e-3)
            report("(b) device filter, whole step    ", t_all)
            report("    predict kernel (HIP events)  ", t_pred)
            report("    finish kernel (HIP events)   ", t_fin)
            report("    fe + update + re-projection  ", t_dev)
            print(f"    PCIe per step: up {n * (raw_bytes + 40 * 7 * 8)} B, down {n * (res_bytes + 19 * 8)} B")
            print(f"    last step: iterations {sorted(set(r.iters for r in res))}, diverged {sum(1 for r in res if r.diverged)}")


if __name__ == "__main__":
    main()
