#!/usr/bin/env python
"""Device time of place recognition (include/lins_place.h).  Build: 2000 and 6000 synthetic room key frames of 4670
points (tests/local_map_synth.room_scan) described in one lins_place_sync — 149 MB of points, which fit the device's
256 MB last-level cache and are re-read by every repeat, and 448 MB, which do not.  Search: 1 / 64 / 256 entries
against slots of 500 / 2000 / 8000 frames (small synthetic places, tests/place_cases.place: what a descriptor holds does not change the
search's work), min_gap_s < 0 so that every frame is a candidate.  HIP-event times, median [min .. max] of 5 runs after
one warm-up; beside each search the fused multiply-adds per second (72 000 a pair) and their share of the f32 vector
peak of 78.6 T FMA/s (157.3 TFLOPS).  The CPU restatement on ONE thread is timed on the smallest case for scale.
usage: tools/place_rate.py [output file]"""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "lins---lidar-inertial-slam_amd"
pkg = importlib.import_module(PKG); ieskf = importlib.import_module(PKG + ".ieskf"); host = importlib.import_module(PKG + ".host")
import numpy as np
import place_cases as pc
from local_map_synth import room_scan, trajectory

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "place_rate.txt")
PEAK_FMA, FMA_PER_PAIR, REPS = 78.6e12, 72000, 5
lines = []
def say(s):
    print(s, flush=True); lines.append(s)

def stat(v):
    v = np.array(v)
    return f"{np.median(v):9.3f} ms [{v.min():9.3f} .. {v.max():9.3f}]"

say(f"place recognition: HIP-event ms, median [min .. max] of {REPS} runs after 1 warm-up")
poses = trajectory(50, seed=6)
scans = [room_scan(i, poses[i]) for i in range(50)]
for NB in (2000, 6000):
    with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
        c.archive_init(1, NB, NB * 4670)
        for i in range(NB):
            c.archive_push(0, *scans[i % 50], poses[i % 50], time=float(i))
        ms = []
        for _ in range(REPS + 1):
            assert c.place_init(up_axis=2) == 0 and c.place_sync([0]) == 0
            st = c.place_stats()
            assert st["frames_built"] == NB
            ms.append(st["build_ms"])
        ms = ms[1:]
        mb = NB * 4670 * 16e-6
        say(f"build   {NB} frames of 4670 points ({mb:4.0f} MB, {'within' if mb < 256 else 'beyond'} the 256 MB last-level cache), one launch   {stat(ms)}   "
            f"{NB / np.median(ms) * 1e3:12.0f} frames/s   {mb / np.median(ms):8.2f} GB/s of points")

SIZES, NQ = (500, 2000, 8000), 256
small = [pc.frame(pc.place(1000 + i, n=150)) for i in range(64)]
with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
    c.archive_init(4, 8000, (sum(SIZES) + NQ) * 150)
    for s, n in enumerate(SIZES):
        for i in range(n):
            c.archive_push(s, *small[(i * 7 + s) % 64], (0, 0, 0, 0, 0, 0), time=float(i))
    for i in range(NQ):
        c.archive_push(3, *small[(i * 5 + 1) % 64], (0, 0, 0, 0, 0, 0), time=1e6)
    assert c.place_init() == 0 and c.place_sync([0, 1, 2, 3]) == 0
    for s, n in enumerate(SIZES):
        for ne in (1, 64, 256):
            q = [(3, k, s, 1e6, -1.0) for k in range(ne)]
            ms, wall = [], []
            for _ in range(REPS + 1):
                t0 = time.perf_counter()
                r = c.place_search(q)
                wall.append((time.perf_counter() - t0) * 1e3)
                st = c.place_stats()
                assert st["pairs"] == ne * n and st["frames_built"] == 0 and all(x["candidates"] == n for x in r)
                ms.append(st["search_ms"])
            ms, wall = ms[1:], wall[1:]
            rate = ne * n * FMA_PER_PAIR / (np.median(ms) * 1e-3)
            say(f"search  {ne:4d} entries x {n:5d} candidates   device {stat(ms)}   whole call {stat(wall)}   {rate * 1e-12:7.2f} T FMA/s = {100 * rate / PEAK_FMA:5.1f} % of the f32 peak")
    D = [c.place_descriptor(2, i) for i in range(SIZES[0])]
    qd = c.place_descriptor(3, 0)
t0 = time.perf_counter()
w = host.place_search(qd, D, np.arange(SIZES[0], dtype=np.float64), 1e6, -1.0)
say(f"host restatement, 1 entry x {SIZES[0]} candidates, ONE thread: {(time.perf_counter() - t0) * 1e3:.1f} ms (winner {w['id']}, shift {w['shift']})")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
