#!/usr/bin/env python
"""Device time of the loop-closure alignment (lins_loop_icp_batch) at the reference's size: 60 synthetic room key frames
(tests/local_map_synth.room_scan: 470 corner, 4000 surf, 200 outlier points a frame) in the archive, the latest frame
stored with a pose error of (0.3, 0.2, 0.1) m and 2 degrees of yaw; source = the latest frame (corner | surf, leaf 0,
DROP_NEGATIVE), target = a history window of 51 frames (corner | surf, leaf 0.4) — both read on the device where the
assembly left them.  HIP-event time (gridding excluded) and whole-call wall time, median / min over `reps` runs after 3
warm-up runs, for a sweep of the group size (rounds queued between two reads of the "still running" word), next to the
CPU restatement on one core.  usage: tools/loop_icp_rate.py [reps] [output file]"""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "lins---lidar-inertial-slam_amd"
pkg = importlib.import_module(PKG); ieskf = importlib.import_module(PKG + ".ieskf"); host = importlib.import_module(PKG + ".host")
import numpy as np
from local_map_synth import room_scan, trajectory

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "loop_icp_rate.txt")
N = 60
lines = []
def say(s):
    print(s, flush=True); lines.append(s)

poses = trajectory(N, seed=6)
frames = [room_scan(i, poses[i]) + (poses[i],) for i in range(N)]
wrong = (poses[N - 1].astype(np.float64) + np.array([0.3, 0.2, 0.1, 0, 0, np.deg2rad(2.0)])).astype(np.float32)
frames[N - 1] = frames[N - 1][:3] + (wrong,)
specs = [dict(slot=0, ids=[N - 1], clouds=3, leaf=0.0, flags=1), dict(slot=0, ids=list(range(4, 55)), clouds=3, leaf=0.4, flags=0)]
with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
    c.archive_init(1, N, sum(len(f[0]) + len(f[1]) + len(f[2]) for f in frames))
    for i, f in enumerate(frames):
        c.archive_push(0, *f, time=0.1 * i)
    info = c.archive_assemble(specs)
    say(f"source: {info[0]['n']} points (latest frame); target: {info[1]['n']} points ({info[1]['points_in']} in, 51 frames, leaf 0.4), "
        f"box {info[1]['box_dim']} cells")
    res = None
    for label, group in [("default group", 0)] + [(f"group {g}", g) for g in (1, 2, 4, 8, 16, 32, 100)]:
        c.debug_loop_icp_group(group)
        for _ in range(3):
            c.loop_icp([(0, 1)])
        ms, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            res = c.loop_icp([(0, 1)])[0]
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(c.loop_icp_stats()[0])
        ms, wall = np.array(ms), np.array(wall)
        say(f"  {label:14s} device median {np.median(ms):8.3f} ms  min {ms.min():8.3f}  max {ms.max():8.3f}   whole call median {np.median(wall):8.3f} ms  "
            f"min {wall.min():8.3f}  [{len(ms)} runs]")
    c.debug_loop_icp_group(0)
    say(f"result: {res['iterations']} rounds, reason {res['reason']}, converged {res['converged']}, fitness {res['fitness']:.5f}, "
        f"n_corr {res['n_corr']}, far searches {res['far_searches']} of {c.loop_icp_stats()[1]} query evaluations")
    s, t = c.archive_download(0), c.archive_download(1)
t0 = time.perf_counter()
want = host.loop_icp(s, t)
say(f"host restatement (exhaustive search), same clouds: {(time.perf_counter() - t0) * 1e3:.0f} ms on 1 thread; {want['iterations']} rounds, reason "
    f"{want['reason']}, max |T - T_device| {np.abs(want['transform'] - res['transform']).max():.3g}")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
