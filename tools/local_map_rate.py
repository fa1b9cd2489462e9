#!/usr/bin/env python
"""Device time / rate of the mapping node's local map (lins_local_map_build) next to the CPU restatement
(lins_host_local_map) on the same inputs: 50-frame windows of synthetic room scans (tests/local_map_synth.py; per key
frame 470 corner, 4000 surf, 200 outlier points — a downsampled scan of the host front-end's size), raw scans of
470 corner / 8200 surf / 200 outlier points.  usage: tools/local_map_rate.py [reps]"""
import importlib, os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "lins---lidar-inertial-slam_amd"
pkg = importlib.import_module(PKG); ieskf = importlib.import_module(PKG + ".ieskf"); host = importlib.import_module(PKG + ".host")
import numpy as np
from local_map_synth import room_scan, trajectory

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
poses = trajectory(120, seed=7)
frames = [room_scan(i, poses[i]) + (poses[i],) for i in range(60)]  # (kept DS-sized clouds)
scans = [room_scan(500 + i, poses[i], n_corner=470, n_surf=8200, n_outlier=200) for i in range(8)]
n_in = sum(len(f[0]) + len(f[1]) + len(f[2]) for f in frames[:50])
med = lambda xs: float(np.median(xs))
with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
    # a live node: one key frame pushed and one map built per call, the window full (what the node waits for)
    c.local_map_init(1, 50, 8192)
    for f in frames[:50]:
        c.local_map_push(0, *f)
    c.local_map_build([0], [scans[0]])
    dev, wall, wall_b = [], [], []
    for r in range(reps):
        f = frames[50 + r % 10]
        t0 = time.perf_counter()
        c.local_map_push(0, *f)
        t1 = time.perf_counter()
        s = c.local_map_build([0], [scans[r % 8]])
        t2 = time.perf_counter()
        dev.append(c.local_map_stats()[0]), wall.append(t2 - t0), wall_b.append(t2 - t1)
    ms1 = med(dev)
    print(f"single slot, 50-frame window ({n_in} map input points, maps {s[0]['n'][0]} corner / {s[0]['n'][1]} surf): device "
          f"{ms1:.3f} ms, build call {med(wall_b) * 1e3:.3f} ms, push + build {med(wall) * 1e3:.3f} ms (medians of {reps})")
    for n in (64, 256):
        c.local_map_init(n, 50, 8192)
        for s_ in range(n):
            for f in frames[s_ % 10:s_ % 10 + 50]:
                c.local_map_push(s_, *f)
        sl = list(range(n))
        sc = [scans[k % 8] for k in range(n)]
        c.local_map_build(sl, sc)
        dev, wall = [], []
        for r in range(max(3, reps // 4)):
            t0 = time.perf_counter()
            c.local_map_build(sl, sc)
            wall.append(time.perf_counter() - t0)
            dev.append(c.local_map_stats()[0])
        ms, pts = med(dev), c.local_map_stats()[1]
        print(f"batch of {n} slots: device {ms:.3f} ms = {ms / n * 1e3:.1f} us per map, {pts / ms / 1e6:.2f} G points/s "
              f"({pts} input points); whole call {med(wall) * 1e3:.2f} ms")
# the restatement on the CPU, same inputs (ctypes lets the threads run in parallel)
jobs = [(frames[k % 10:k % 10 + 50], scans[k % 8]) for k in range(64)]
t0 = time.perf_counter()
for fr, sc in jobs[:8]:
    host.local_map(fr, sc)
one = (time.perf_counter() - t0) / 8
t0 = time.perf_counter()
with ThreadPoolExecutor(16) as ex:
    list(ex.map(lambda j: host.local_map(*j), jobs))
sixteen = (time.perf_counter() - t0) / len(jobs)
print(f"host restatement: {one * 1e3:.2f} ms per map on 1 thread, {sixteen * 1e3:.2f} ms per map on 16 threads "
      f"(single slot: {one * 1e3 / ms1:.1f} x the device time)")
