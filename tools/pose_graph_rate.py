#!/usr/bin/env python
"""Device time of the pose graph's batched solve (lins_pose_graph_solve): 64 and 256 slots, chains of 500 and 2000 key
frames along an arc (tests/pose_graph_cases.trajectory), 1 / 4 / 16 loops a slot — each loop closes a span of the chain
with a correction of 0.3 m and 1.5 degrees at variance 1e-6, the spans spread over the chain and overlapping.  Every
slot holds the same graph (a problem's cost does not depend on its neighbours; the launch is one workgroup per slot).

Method: the graphs are rebuilt (lins_pose_graph_init + pushes) before EVERY run, so that each run solves from the pushed
state; 1 warm-up run, then 5 runs; reported are the median with min..max of the HIP-event time of the device sequence
(the trial launches between the first and the last, the reads of the "still running" word included) and of the whole
call's wall time (uploads of the graph, the solve, the download of the poses).  One process, the device otherwise idle.
usage: tools/pose_graph_rate.py [output file]"""
import ctypes as C
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "lins---lidar-inertial-slam_amd"
pkg = importlib.import_module(PKG); ieskf = importlib.import_module(PKG + ".ieskf"); defs = importlib.import_module(PKG + "._ctypes_defs")
import numpy as np
import pose_graph_cases as cases

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pose_graph_rate.txt")
WARM, REPS = 1, 5
lines = []
def say(s):
    print(s, flush=True); lines.append(s)

def graph(n_frames, n_loops):
    """(six floats per frame, loops (latest, closest, pose_from)): loop i closes the span that ends at frame
    N - 1 - i * step and is N / 2 frames long at most — spans overlap their neighbours"""
    aft = cases.trajectory(3, n_frames, radius=25.0, turn=1.5 * np.pi, centre=(0.0, 0.0))
    step = max(1, (n_frames // 2) // n_loops)
    loops = []
    for i in range(n_loops):
        b = n_frames - 1 - i * step
        a = max(0, b - n_frames // 2)
        loops.append((b, a, cases.corrected(aft[b], 0.3, 1.5, 50 + i)))
    return aft, loops

L = ieskf.lib()
L.lins_pose_graph_push.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
L.lins_pose_graph_add_loop.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(defs.KeyPoseC), C.c_double]

def fill(c, n_slots, aft, loops):
    c.pose_graph_init(n_slots, len(aft), max(len(loops), 1))
    rows = [defs.six_floats(p) for p in aft]
    pfs = [defs.key_pose(pf) for _, _, pf in loops]
    for s in range(n_slots):
        for k in range(len(rows)):
            rc = L.lins_pose_graph_push(c._h, s, rows[k - 1] if k else None, rows[k])
            assert rc == k, rc
        for (b, a, _), pf in zip(loops, pfs):
            assert L.lins_pose_graph_add_loop(c._h, s, b, a, C.byref(pf), 1e-6) == 0

say("pose graph solve: HIP-event ms of the device sequence and wall ms of the whole call; median [min .. max] of %d runs after %d warm-up" % (REPS, WARM))
say("default parameters (lins_pose_graph_default_params); every run starts from freshly pushed graphs")
with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
    for n_frames in (500, 2000):
        for n_loops in (1, 4, 16):
            aft, loops = graph(n_frames, n_loops)
            for n_slots in (64, 256):
                dev, wall, res = [], [], None
                for run in range(WARM + REPS):
                    fill(c, n_slots, aft, loops)
                    t0 = time.perf_counter()
                    res = c.pose_graph_solve(list(range(n_slots)))
                    w = (time.perf_counter() - t0) * 1e3
                    if run >= WARM:
                        dev.append(c.pose_graph_stats()[0]); wall.append(w)
                dev, wall = np.array(dev), np.array(wall)
                its = sorted(set(r["iterations"] for r in res))
                say(f"  slots {n_slots:4d}  frames {n_frames:5d}  loops {n_loops:3d}   device {np.median(dev):9.3f} ms [{dev.min():9.3f} .. {dev.max():9.3f}]   "
                    f"whole call {np.median(wall):9.3f} ms [{wall.min():9.3f} .. {wall.max():9.3f}]   trials {its}  reason {sorted(set(r['reason'] for r in res))}  "
                    f"cost {res[0]['cost_before']:.4g} -> {res[0]['cost_after']:.4g}")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
