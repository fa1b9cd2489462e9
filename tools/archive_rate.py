#!/usr/bin/env python
"""Device time of the key-frame archive's assembly (lins_archive_assemble) on one slot of synthetic room key frames
(tests/local_map_synth.room_scan: 470 corner, 4000 surf, 200 outlier points a frame): a global map of 1 000 frames (all
three clouds, 0.4 m) and a loop-closure history submap of 51 frames (corner + surf, 0.4 m), each through the scans split
over workgroups (the default chunk and a sweep of chunks) and, with the chunk set to "never split", through the local-map
build's one-workgroup scans.  HIP-event times; per case 3 warm-up runs, then `reps` timed ones in alternation with the
other path.  usage: tools/archive_rate.py [reps] [output file]"""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "lins---lidar-inertial-slam_amd"
pkg = importlib.import_module(PKG); ieskf = importlib.import_module(PKG + ".ieskf"); host = importlib.import_module(PKG + ".host")
import numpy as np
from local_map_synth import room_scan, trajectory

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "keyframe_archive_rate.txt")
NEVER, N = 2 ** 31 - 1, 1000
lines = []
def say(s):
    print(s, flush=True); lines.append(s)

poses = trajectory(N, seed=7)
frames = [room_scan(i, poses[i]) + (poses[i],) for i in range(N)]
with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
    c.archive_init(1, N, sum(len(f[0]) + len(f[1]) + len(f[2]) for f in frames))
    t0 = time.perf_counter()
    for i, f in enumerate(frames):
        c.archive_push(0, *f, time=0.1 * i)
    say(f"{N} key frames pushed in {time.perf_counter() - t0:.2f} s ({(time.perf_counter() - t0) / N * 1e3:.3f} ms a frame)")
    cases = [("global map, 1000 frames, corner + surf + outlier, leaf 0.4", dict(slot=0, ids=list(range(N)), clouds=7, leaf=0.4, flags=0)),
             ("history submap, 51 frames, corner + surf, leaf 0.4", dict(slot=0, ids=list(range(475, 526)), clouds=3, leaf=0.4, flags=0)),
             ("latest frame, corner + surf, leaf 0, DROP_NEGATIVE", dict(slot=0, ids=[N - 1], clouds=3, leaf=0.0, flags=1))]
    def timed(spec, chunk, k):
        c.archive_set_scan_chunk(chunk)
        ms, wall = [], []
        for r in range(k):
            t0 = time.perf_counter()
            info = c.archive_assemble([spec])[0]
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(c.archive_stats()[0])
        return ms, wall, info
    for name, spec in cases:
        chunks = [("default chunk (split)", 0), ("never split (one-workgroup scans)", NEVER)] + [(f"chunk {k}", k) for k in (4, 8, 32, 64, 128)]
        res = {label: ([], []) for label, _ in chunks}
        for label, ch in chunks:
            timed(spec, ch, 3)  # warm-up (the arenas grow on the first)
        for r in range(reps):  # the paths in alternation, so that drift hits them alike
            for label, ch in chunks:
                ms, wall, info = timed(spec, ch, 1)
                res[label][0].extend(ms), res[label][1].extend(wall)
        say(f"{name}: {info['points_in']} points in, {info['n']} out, {-(-info['points_in'] // 512)} tiles, status {info['status']}")
        for label, _ in chunks:
            ms, wall = np.array(res[label][0]), np.array(res[label][1])
            say(f"  {label:36s} device median {np.median(ms):8.3f} ms  min {ms.min():8.3f}  max {ms.max():8.3f}  "
                f"(spread {100 * (ms.max() - ms.min()) / np.median(ms):.1f} %)  whole call median {np.median(wall):8.3f} ms  [{len(ms)} runs]")
    c.archive_set_scan_chunk(0)
    # the restatement on one CPU thread, same history submap
    t0 = time.perf_counter()
    host.submap(frames[475:526], list(range(51)), 3, 0.4, 0)
    say(f"host restatement of the history submap: {(time.perf_counter() - t0) * 1e3:.1f} ms on 1 thread")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
