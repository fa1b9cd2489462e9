#!/usr/bin/env python3
"""What the surrounding-key-frame map costs (lins_local_map_build_surround, lins_streams_map_surround);
profiles/surround_map_rate.txt keeps one run.  Medians of --runs runs, each on a FRESH context, with min .. max.

1. Device time (HIP events, lins_last_local_map_stats) of the surround build at 1 and --slots slots for lists of 50, 200
   and 500 room frames (~4.7 k points each), and beside them, in the same run and on the same frames: lins_local_map_build
   on a full 50-frame ring, and lins_archive_assemble of the same two specs per slot (lins_last_archive_stats).
2. Host time of one stream's selection plus list rule (lins_host_select_radius + lins_host_surround_update, the text the
   step compiles) at 500, 2 000 and 8 000 key poses, radius 50 m, pose leaf 1 m, the robot moving 1 m between calls.

    python tools/surround_rate.py [--slots 64] [--runs 5] [--out profiles/surround_map_rate.txt]
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
LISTS = (50, 200, 500)
DISTINCT = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--poses", type=int, nargs="+", default=[500, 2000, 8000])
    ap.add_argument("--skip-device", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surround_map_rate.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g

    g.build()
    pkg, host, ieskf = (importlib.import_module(PKG + m) for m in ("", ".host", ".ieskf"))
    defs = importlib.import_module(PKG + "._ctypes_defs")
    from local_map_synth import room_scan, trajectory

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stat(name, v, unit="ms"):
        say(f"  {name}: median {statistics.median(v):10.4f} {unit}   min {min(v):10.4f} .. max {max(v):10.4f}   ({len(v)} runs)")
        return statistics.median(v), min(v), max(v)

    # ---- 1. the build
    if not args.skip_device:
        ns, most = args.slots, max(LISTS)
        poses = trajectory(DISTINCT, seed=1)
        frames = [defs.keyframe_c(*room_scan(i, poses[i]), poses[i]) for i in range(DISTINCT)]  # (struct, arrays kept alive)
        per_frame = [int(f.n_corner + f.n_surf + f.n_outlier) for f, _ in frames]
        scans = [room_scan(900 + i, poses[i]) for i in range(4)]
        L = ieskf.lib()
        L.lins_archive_push.argtypes = [C.c_void_p, C.c_int, C.POINTER(defs.KeyframeC), C.c_double]
        L.lins_local_map_push.argtypes = [C.c_void_p, C.c_int, C.POINTER(defs.KeyframeC)]
        t = {}
        for run in range(args.runs):
            with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
                c.local_map_init(ns, 50, 8192)
                c.archive_init(ns, most, ns * most * max(per_frame))
                for s in range(ns):  # frame i of every slot: the room seen from pose i mod 16 of a loop through it
                    for i in range(most):
                        assert L.lins_archive_push(c._h, s, C.byref(frames[i % DISTINCT][0]), float(i)) == i
                    for i in range(50):
                        assert L.lins_local_map_push(c._h, s, C.byref(frames[i % DISTINCT][0])) == 0
                c.local_map_build_surround([0], [[0]], [scans[0]])  # (the kernels' code is loaded before anything is timed)
                c.archive_assemble([(0, [0], defs.SUBMAP_CORNER, 0.2, 0)])
                for n in (1, ns):
                    slots, sc = list(range(n)), [scans[k % 4] for k in range(n)]
                    c.local_map_build(slots, sc)
                    t.setdefault(("ring", n, 50), []).append(c.local_map_stats()[0])
                    for ll in LISTS:
                        ids = list(range(ll))
                        c.local_map_build_surround(slots, [ids] * n, sc)
                        ms, pts = c.local_map_stats()
                        t.setdefault(("surround", n, ll), []).append(ms)
                        t[("points", n, ll)] = pts
                        c.archive_assemble([(s, ids, cl, leaf, 0) for s in slots
                                            for cl, leaf in ((defs.SUBMAP_CORNER, 0.2), (defs.SUBMAP_SURF | defs.SUBMAP_OUTLIER, 0.4))])
                        t.setdefault(("assemble", n, ll), []).append(c.archive_stats()[0])
                    c.archive_set_scan_chunk(2 ** 31 - 1)  # the 50-frame list with every scan in one workgroup, as the ring build's are
                    c.local_map_build_surround(slots, [list(range(50))] * n, sc)
                    t.setdefault(("unsplit", n, 50), []).append(c.local_map_stats()[0])
                    c.archive_set_scan_chunk(0)
        say(f"device time of one build, room frames of {statistics.mean(per_frame):.0f} points, scans of {sum(len(a) for a in scans[0])} points; "
            f"fresh context per run")
        spread = {}
        for n in (1, ns):
            say(f"{n} slot(s)")
            spread[n] = stat("lins_local_map_build, full ring of 50 frames       ", t[("ring", n, 50)])
            for ll in LISTS:
                say(f" list of {ll} frames ({t[('points', n, ll)]} points read per build)")
                m = stat(f"lins_local_map_build_surround                    ", t[("surround", n, ll)])
                stat(f"lins_archive_assemble, the two specs per slot    ", t[("assemble", n, ll)])
                if ll == 50:
                    u = stat(f"  the same with no scan split (chunk = INT_MAX)  ", t[("unsplit", n, 50)])
                    lo, hi = spread[n][1], spread[n][2]
                    say(f"  the 50-frame list against the ring build: {m[0] / spread[n][0]:.3f} x its median, "
                        f"{'within' if lo <= m[0] <= hi else 'OUTSIDE'} the ring runs' min .. max; with no scan split {u[0] / spread[n][0]:.3f} x, "
                        f"{'within' if lo <= u[0] <= hi else 'OUTSIDE'}")
        say("(a 50-frame list and a full ring read the same points through the same VoxelGrid kernels.  They differ in the scans: a")
        say(" ring build scans every job's (256 digits x tiles) histogram in one workgroup, whatever its size — a 50-frame surf job is")
        say(" ~410 tiles — while a listed job of more than 16 tiles takes the archive's split scans.  The line \"no scan split\" is the")
        say(" surround build made to scan as the ring build does.  What the two then still differ in is the first kernel, not timed")
        say(" apart here: ar_gather_kernel issues one set of six box atomics per workgroup, lm_transform_kernel one per wave, and surf")
        say(" and outlier of a listed frame travel as one segment.  Giving the ring build the split scans is a follow-up: this change")
        say(" leaves its launches as they were.)")
        say()

    # ---- 2. selection + list rule on the host
    H = host.lib()
    H.lins_host_select_radius.argtypes = [C.POINTER(defs.KeyPoseC), C.c_int, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_void_p, C.c_int]
    H.lins_host_select_radius.restype = C.c_int
    H.lins_host_surround_update.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    H.lins_host_surround_update.restype = C.c_int
    say("host time of one stream's selection + list rule, radius 50 m, pose leaf 1 m, the robot 1 m further at each call")
    rng = np.random.default_rng(3)
    for layout in ("exploring: key poses 0.5 m apart along an outward spiral, the robot at its end",
                   "staying: every key pose within 35 m of the robot (uniform in a disc)"):
        say(" " + layout)
        for npose in args.poses:
            if layout.startswith("exploring"):
                k = np.arange(npose)
                r, th = 2.0 + 0.05 * k, 0.0 * k
                th[1:] = np.cumsum(0.5 / r[:-1])  # arc steps of 0.5 m
                xy = np.stack([r * np.cos(th), r * np.sin(th)], 1)
                centres = [xy[at] for at in (npose - 5, npose - 3, npose - 1)]
            else:
                rr, th = 35.0 * np.sqrt(rng.uniform(0, 1, npose)), rng.uniform(0, 2 * np.pi, npose)
                xy = np.stack([rr * np.cos(th), rr * np.sin(th)], 1)
                centres = [np.array([x, 0.0]) for x in (-1.0, 0.0, 1.0)]
            arr = (defs.KeyPoseC * npose)(*[defs.KeyPoseC(float(p[0]), float(p[1]), 0.0, 0.0, 0.0, 0.0) for p in xy])
            ds, lst = np.zeros(npose, np.int32), np.zeros(npose, np.int32)
            v, listed = [], 0
            for run in range(args.runs):
                n_list = 0
                for ctr in centres:  # two calls fill the list, the third is timed
                    centre = (C.c_float * 3)(float(ctr[0]), float(ctr[1]), 0.0)
                    t0 = time.perf_counter()
                    nd = H.lins_host_select_radius(arr, npose, centre, 50.0, 1.0, ds.ctypes.data, npose)
                    n_list = H.lins_host_surround_update(lst.ctypes.data, n_list, npose, ds.ctypes.data, nd)
                    t1 = time.perf_counter()
                    assert nd >= 0 and n_list >= 0
                v.append((t1 - t0) * 1e3)
                listed = n_list
            stat(f"{npose:5d} key poses, {listed:4d} listed", v)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
