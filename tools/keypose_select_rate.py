#!/usr/bin/env python3
"""Where the key-pose selection on the device pays (lins_keyposes_*, LINS_KEYPOSES_DEVICE) against the host loops of the
same library (lins_archive_select_radius / _find_loop per slot, LINS_KEYPOSES_HOST); profiles/keypose_select_rate.txt
keeps one run.  Medians of --runs with min .. max, wall time around the library calls, both modes in the same run on the
same context and poses.

For each layout of tools/surround_rate.py (exploring: key poses 0.5 m apart along a spiral, the robot at its end; yard:
every key pose within 35 m of the robot), each number of key poses per slot and 1 / 64 / 256 slots:
  select     n x lins_archive_select_radius                                 against  one lins_keyposes_select_batch
  find-loop  n x lins_archive_find_loop (radius 5 m, gap 30 s, 10 poses/s)  against  one lins_keyposes_find_loop_batch
  surround   n x (lins_archive_select_radius + lins_host_surround_update)   against  one lins_keyposes_surround_batch
  step       lins_streams_map_step in surround mode over n streams, the two modes on alternate steps
radius 50 m, pose leaf 1 m.  Key frames hold one point each, so the step's map build is small and what differs between
the modes is the selection.

    python tools/keypose_select_rate.py [--slots 1 64 256] [--poses 500 2000 8000] [--runs 5] [--out profiles/keypose_select_rate.txt]
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
RADIUS, LEAF, LOOP_RADIUS, GAP = 50.0, 1.0, 5.0, 30.0


def layout_xy(name, npose, rng):
    """key poses (x, y) with the robot at the origin"""
    if name == "exploring":
        k = np.arange(npose)
        r, th = 2.0 + 0.05 * k, 0.0 * k
        th[1:] = np.cumsum(0.5 / r[:-1])  # arc steps of 0.5 m
        xy = np.stack([r * np.cos(th), r * np.sin(th)], 1)
        return xy - xy[-1]
    rr, th = 35.0 * np.sqrt(rng.uniform(0, 1, npose)), rng.uniform(0, 2 * np.pi, npose)
    return np.stack([rr * np.cos(th), rr * np.sin(th)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 64, 256])
    ap.add_argument("--poses", type=int, nargs="+", default=[500, 2000, 8000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypose_select_rate.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g

    g.build()
    pkg, host, ieskf, sm = (importlib.import_module(PKG + m) for m in ("", ".host", ".ieskf", ".streams_map"))
    defs = importlib.import_module(PKG + "._ctypes_defs")

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    def pair(name, h, d):
        mh, md = statistics.median(h), statistics.median(d)
        say(f"    {name:9s} host {mh:9.3f} ms ({min(h):9.3f} .. {max(h):9.3f})   device {md:8.3f} ms ({min(d):8.3f} .. {max(d):8.3f})   "
            f"host / device {mh / md:7.2f}")

    L, H = ieskf.lib(), host.lib()
    Q, LQ, R = defs.KeyposesQueryC, defs.KeyposesLoopQueryC, defs.KeyposesResultC
    fp, ip = C.POINTER(C.c_float), C.c_void_p
    L.lins_archive_push.argtypes = [C.c_void_p, C.c_int, C.POINTER(defs.KeyframeC), C.c_double]
    L.lins_archive_select_radius.argtypes = [C.c_void_p, C.c_int, fp, C.c_float, C.c_float, ip, C.c_int]
    L.lins_archive_find_loop.argtypes = [C.c_void_p, C.c_int, fp, C.c_float, C.c_double, C.c_double, C.POINTER(C.c_int32)]
    L.lins_keyposes_select_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(Q), ip, C.c_int, C.POINTER(R)]
    L.lins_keyposes_find_loop_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(LQ), ip]
    L.lins_keyposes_surround_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(Q), ip, C.c_int, ip, C.POINTER(R)]
    H.lins_host_surround_update.argtypes = [ip, C.c_int, C.c_int, ip, C.c_int]
    H.lins_host_surround_update.restype = C.c_int

    ns_max = max(args.slots)
    point = np.array([[0.1, 0.2, 0.3, 0.0]], np.float32)
    none = np.zeros((0, 4), np.float32)
    raws = [host.synth_raw_scan(i, 0) for i in range(4)]
    st = np.zeros((ns_max, 19))
    st[:, 6] = 1.0
    cov = np.tile(np.eye(18)[None] * 1e-4, (ns_max, 1, 1))
    rng = np.random.default_rng(3)
    say(f"radius {RADIUS:g} m, pose leaf {LEAF:g} m; wall ms around the library calls, median (min .. max) of {args.runs}; "
        f"host: the per-slot calls of LINS_KEYPOSES_HOST, device: one batched call")
    for layout in ("exploring", "yard"):
        for npose in args.poses:
            xy = layout_xy(layout, npose, rng)
            steps = len(args.slots) * (2 + 2 * args.runs)  # (every step may store a key frame of a whole scan per stream)
            cap = npose + steps + 8
            with ieskf.IeskfContext(pkg.default_params(num_iter=8), max_batch=ns_max, max_targets=16 * 1800) as c:
                c.streams_init(ns_max)
                c.local_map_init(ns_max, 3, 16384)
                c.archive_init(ns_max, cap, ns_max * (npose + (0 if args.skip_step else steps * 16384)))
                frame, _keep = defs.keyframe_c(point, none, none, np.zeros(6, np.float32))
                for i in range(npose):  # the same poses in every slot, 10 a second
                    frame.pose.x, frame.pose.y = float(xy[i, 0]), float(xy[i, 1])
                    for s in range(ns_max):
                        assert L.lins_archive_push(c._h, s, C.byref(frame), 0.1 * i) == i
                now = 0.1 * npose
                centre = (C.c_float * 3)(0.0, 0.0, 0.0)
                ids = np.zeros(npose, np.int32)
                say(f"{layout}, {npose} key poses per slot")
                for n in args.slots:
                    qs = (Q * n)(*[defs.keyposes_query(s, (0, 0, 0), RADIUS, LEAF) for s in range(n)])
                    lqs = (LQ * n)(*[LQ(defs.keyposes_query(s, (0, 0, 0), LOOP_RADIUS, 0.0), now, GAP) for s in range(n)])
                    res = (R * n)()
                    out = np.zeros((n, 2 * npose), np.int32)
                    closest = np.zeros(n, np.int32)
                    one = C.c_int32(0)
                    t = {k: [] for k in ("sel_h", "sel_d", "loop_h", "loop_d", "sur_h", "sur_d")}
                    nd = 0
                    for run in range(args.runs + 1):  # (the first round loads code and grows buffers: not kept)
                        t0 = time.perf_counter()
                        for s in range(n):
                            nd = L.lins_archive_select_radius(c._h, s, centre, RADIUS, LEAF, ids.ctypes.data, npose)
                        t1 = time.perf_counter()
                        assert L.lins_keyposes_select_batch(c._h, n, qs, out.ctypes.data, 2 * npose, res) == 0
                        t2 = time.perf_counter()
                        assert nd == res[n - 1].n and np.array_equal(ids[:nd], out[n - 1, :nd])
                        for s in range(n):
                            assert L.lins_archive_find_loop(c._h, s, centre, LOOP_RADIUS, now, GAP, C.byref(one)) == 0
                        t3 = time.perf_counter()
                        assert L.lins_keyposes_find_loop_batch(c._h, n, lqs, closest.ctypes.data) == 0
                        t4 = time.perf_counter()
                        assert one.value == closest[n - 1]
                        lists = np.zeros((n, 2 * npose), np.int32)  # a list of every second frame
                        n_list = np.full(n, npose // 2, np.int32)
                        lists[:, : npose // 2] = np.arange(0, 2 * (npose // 2), 2)
                        mine = lists.copy()
                        t5 = time.perf_counter()
                        for s in range(n):
                            nd = L.lins_archive_select_radius(c._h, s, centre, RADIUS, LEAF, ids.ctypes.data, npose)
                            nl = H.lins_host_surround_update(mine[s].ctypes.data, npose // 2, 2 * npose, ids.ctypes.data, nd)
                        t6 = time.perf_counter()
                        assert L.lins_keyposes_surround_batch(c._h, n, qs, lists.ctypes.data, 2 * npose, n_list.ctypes.data, res) == 0
                        t7 = time.perf_counter()
                        assert nl == n_list[n - 1] and np.array_equal(mine[n - 1, :nl], lists[n - 1, :nl])
                        if run:
                            for k, v in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t6 - t5, t7 - t6)):
                                t[k].append(v * 1e3)
                    stats = c.keyposes_stats()
                    say(f"  {n} slot(s): {res[n - 1].hits} hits, {res[n - 1].n} selected, {int(n_list[n - 1])} listed per slot; "
                        f"{stats['host_entries']} entries served by the host")
                    pair("select", t["sel_h"], t["sel_d"])
                    pair("find-loop", t["loop_h"], t["loop_d"])
                    pair("surround", t["sur_h"], t["sur_d"])
                    flush()
                if args.skip_step:
                    continue
                # the step as a whole: the robot stands at the origin; two steps fill the lists, then the modes alternate
                sm.init(c, ns_max, 0.3)
                sm.surround(c, True, RADIUS, LEAF)
                step_no = 0
                for n in args.slots:
                    streams = list(range(n))
                    w = {defs.KEYPOSES_HOST: [], defs.KEYPOSES_DEVICE: []}
                    for r in range(2 + 2 * args.runs):
                        step_no += 1
                        c.streams_step_raw([raws[(i + r) % 4] for i in range(ns_max)], st, cov)
                        od = [sm.odom(np.zeros(6, np.float32), 0.4 * step_no) for _ in streams]
                        mode = defs.KEYPOSES_DEVICE if r % 2 else defs.KEYPOSES_HOST
                        c.keyposes_set_mode(mode)
                        t0 = time.perf_counter()
                        out = sm.step(c, streams, od)
                        t1 = time.perf_counter()
                        assert all(o["status"] == 0 for o in out)
                        if r >= 2:
                            w[mode].append((t1 - t0) * 1e3)
                    say(f"  {n} stream(s), lins_streams_map_step in surround mode, {len(sm.surround_list(c, 0))} frames listed")
                    pair("step", w[defs.KEYPOSES_HOST], w[defs.KEYPOSES_DEVICE])
                    flush()
    flush()


if __name__ == "__main__":
    main()
