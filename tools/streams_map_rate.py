#!/usr/bin/env python3
"""Two measurements around the outlier cloud and the streams -> local map hand-over; profiles/streams_map_rate.txt keeps
one run.  HIP-event medians and minimums over --runs runs after --warmup, both sides of every comparison in ONE process
and one GPU visit, alternating.

1. Cost of the emission: lins_last_segment_ms of lins_segment_batch_outliers against lins_segment_batch (the same kernel
   with a null outlier arena) on --scans stock raw scans, and — with --parent-lib, a liblins_ieskf.so built from the
   parent commit — against that library's lins_segment_batch in the same loop.
2. What the hand-over saves: one lins_local_map_build_streams against the host route (three lins_streams_map_cloud
   downloads per stream + lins_local_map_build), wall time around the calls and the device time of
   lins_last_local_map_stats, on --streams streams after one raw step.

    python tools/streams_map_rate.py [--parent-lib ab/liblins_ieskf_parent.so] [--out profiles/streams_map_rate.txt]
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
PKG = "lins---lidar-inertial-slam_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64, help="distinct stock scans (repeated up to --scans)")
    ap.add_argument("--streams", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streams_map_rate.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g

    g.build()
    pkg, host, ieskf = (importlib.import_module(PKG + m) for m in ("", ".host", ".ieskf"))
    defs = importlib.import_module(PKG + "._ctypes_defs")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stat(name, v):
        say(f"  {name}: median {statistics.median(v):9.4f} ms   min {min(v):9.4f}   max {max(v):9.4f}   ({len(v)} runs after {args.warmup} warm-up)")
        return statistics.median(v)

    # ---- 1. the emission
    distinct = [host.synth_raw_scan(i, 1) for i in range(args.distinct)]
    raws = [distinct[i % len(distinct)] for i in range(args.scans)]
    n = len(raws)
    P = C.POINTER(host.Point)
    ptrs = (P * n)(*[r.ctypes.data_as(P) for r in raws])
    cnts = (C.c_int32 * n)(*[len(r) for r in raws])
    segs = (host.SegmentedScanC * n)()
    N = defs.CLOUD_MAX
    keep = [np.zeros((N, 4), np.float32), np.zeros(N, np.float32), np.zeros(N, np.uint32), np.zeros(N, np.uint8)]  # (one scratch scan: timing only)
    for k in range(n):
        segs[k].cloud, segs[k].range = keep[0].ctypes.data_as(P), keep[1].ctypes.data_as(C.POINTER(C.c_float))
        segs[k].col, segs[k].ground = keep[2].ctypes.data_as(C.POINTER(C.c_uint32)), keep[3].ctypes.data_as(C.POINTER(C.c_uint8))
    obuf = np.zeros((defs.OUTLIER_MAX, 4), np.float32)
    optrs = (P * n)(*[obuf.ctypes.data_as(P)] * n)
    prm = pkg.default_params()

    def open_lib(path):
        L = C.CDLL(path)
        L.lins_create.argtypes = [C.POINTER(defs.Params), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        assert L.lins_create(C.byref(prm), 0, 1, 1024, C.byref(h)) == 0
        L.lins_segment_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(P), C.POINTER(C.c_int32), C.POINTER(host.SegmentedScanC)]
        L.lins_last_segment_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.lins_destroy.argtypes = [C.c_void_p]
        L.lins_destroy.restype = None
        return L, h

    def seg_ms(L, h, outliers):
        if outliers:
            L.lins_segment_batch_outliers.argtypes = [C.c_void_p, C.c_int, C.POINTER(P), C.POINTER(C.c_int32), C.POINTER(host.SegmentedScanC), C.POINTER(P)]
            rc = L.lins_segment_batch_outliers(h, n, ptrs, cnts, segs, optrs)
        else:
            rc = L.lins_segment_batch(h, n, ptrs, cnts, segs)
        assert rc == 0, rc
        ms = C.c_float(0)
        L.lins_last_segment_ms(h, C.byref(ms))
        return ms.value

    new = open_lib(ieskf.lib_path())
    old = open_lib(args.parent_lib) if args.parent_lib else None
    t = dict(outl=[], null=[], parent=[])
    for r in range(args.warmup + args.runs):
        a, b = seg_ms(*new, True), seg_ms(*new, False)
        p = seg_ms(*old, False) if old else None
        if r >= args.warmup:
            t["outl"].append(a), t["null"].append(b)
            if old:
                t["parent"].append(p)
    say(f"segmentation kernel, {n} stock raw scans ({args.distinct} distinct), {sum(int(s.n_outlier) for s in segs) / n:.0f} outliers per scan on average")
    m_o = stat("lins_segment_batch_outliers          ", t["outl"])
    m_n = stat("lins_segment_batch (null arena)      ", t["null"])
    if old:
        m_p = stat("parent commit's lins_segment_batch   ", t["parent"])
        say(f"  ratios to the parent: with the emission {m_o / m_p:.4f}, null arena {m_n / m_p:.4f}   (bar: each <= 1.05)")
    else:
        say(f"  parent commit's library: not measured (no --parent-lib); emission / null arena = {m_o / m_n:.4f}")
    for L, h in (new,) + ((old,) if old else ()):
        L.lins_destroy(h)

    # ---- 2. the hand-over
    for ns in args.streams:
        with ieskf.IeskfContext(pkg.default_params(num_iter=8), max_batch=ns, max_targets=16 * 1800) as c:
            c.streams_init(ns)
            st = np.zeros((ns, 19))
            st[:, 6] = 1.0
            c.streams_step_raw([distinct[i % len(distinct)] for i in range(ns)], st, np.tile(np.eye(18)[None] * 1e-4, (ns, 1, 1)))
            c.local_map_init(ns, 5, 16384)
            slots = list(range(ns))
            w = dict(dev=[], host=[])
            d = dict(dev=[], host=[], stage=[])
            pts = 0
            for r in range(args.warmup + args.runs):
                t0 = time.perf_counter()
                c.local_map_build_streams(slots, slots)
                t1 = time.perf_counter()
                ms_dev, pts = c.local_map_stats()
                ms_stage = c.local_map_stage_ms()
                t2 = time.perf_counter()
                clouds = [tuple(c.streams_map_cloud(i, k) for k in range(3)) for i in range(ns)]
                c.local_map_build(slots, clouds)
                t3 = time.perf_counter()
                ms_host, _ = c.local_map_stats()
                if r >= args.warmup:
                    w["dev"].append((t1 - t0) * 1e3), w["host"].append((t3 - t2) * 1e3)
                    d["dev"].append(ms_dev), d["host"].append(ms_host), d["stage"].append(ms_stage)
            say(f"{ns} streams, {pts} scan points per build, {sum(a.nbytes for cl in clouds for a in cl)} B over PCIe each way on the host route")
            stat("build_streams, wall                  ", w["dev"])
            stat("map_cloud x 3 + build, wall          ", w["host"])
            a = stat("build_streams, device time           ", d["dev"])
            s = stat("  of which the staging kernel        ", d["stage"])
            b = stat("host route's build, device time      ", d["host"])
            say(f"  device time {a:.4f} <= host route's {b:.4f} + staging {s:.4f} = {b + s:.4f}: {'yes' if a <= b + s else 'NO'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
