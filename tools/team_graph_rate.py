#!/usr/bin/env python
"""Time of the team graph's batched solve (lins_team_graph_solve): 64 and 256 slots of 2 000 key frames along an arc
(tests/pose_graph_cases.trajectory), solved in groups of 1, 2 and 4 with 1 and 4 team factors per pair of neighbouring
members.  Every slot holds the same chain with one loop of its own (frame 1999 to frame 999, 0.3 m and 1.5 degrees at
variance 1e-6), so that a group of one has something to solve; a team factor ties frame 1999 - 300 j of member m + 1 to
frame 300 j of member m, their relative pose as pushed moved by 0.1 m and 0.5 degrees, at variance 1e-4; root variances
(0.01 rad)^2 and (0.1 m)^2.  Nothing here is a pass bar.

Method: the graphs are rebuilt (lins_pose_graph_init + pushes) before EVERY run, so that each run solves from the pushed
state; 1 warm-up run, then 5 runs; reported are the median with min..max of the HIP-event time of the device sequence
(gather, begin and trial launches, the reads of the "still running" word included) and of the whole call's wall time
(uploads, the solve, the download of the poses, the scatter).  Against it: lins_pose_graph_solve of the same slots (the
same method; it knows nothing of the factors: the cost of solving every slot alone), and lins_host_team_graph_solve
looped over the groups on the CPU (one run, wall time of the solves alone, one thread).  One process, the device
otherwise idle.
usage: tools/team_graph_rate.py [output file]"""
import ctypes as C
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "lins---lidar-inertial-slam_amd"
pkg = importlib.import_module(PKG); ieskf = importlib.import_module(PKG + ".ieskf"); defs = importlib.import_module(PKG + "._ctypes_defs")
host = importlib.import_module(PKG + ".host"); team = importlib.import_module(PKG + ".team")
import numpy as np
import pose_graph_cases as cases
import team_graph_cases as tgc

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "team_graph_rate.txt")
WARM, REPS, FRAMES, MAX_LOOPS = 1, 5, 2000, 5
ROOT_VARIANCE = tgc.ROOT_VARIANCE
lines = []
def say(s):
    print(s, flush=True); lines.append(s)

aft = cases.trajectory(3, FRAMES, radius=25.0, turn=1.5 * np.pi, centre=(0.0, 0.0))
own = (FRAMES - 1, FRAMES // 2 - 1, cases.corrected(aft[FRAMES - 1], 0.3, 1.5, 50))
member = dict(aft=aft)

def factors_of(slots, per_pair):
    """the factors of one group on the slots given: per_pair between every pair of neighbouring members"""
    out = []
    for m in range(len(slots) - 1):
        for j in range(per_pair):
            mb, ib, ma, ia, Z, var = tgc.factor([member, member], 1, FRAMES - 1 - 300 * j, 0, 300 * j, 0.1, 0.5, 1e-4, 900 + 10 * m + j)
            out.append((slots[m + 1], ib, slots[m], ia, Z, var))
    return out

L = ieskf.lib()
L.lins_pose_graph_push.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
L.lins_pose_graph_add_loop.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(defs.KeyPoseC), C.c_double]
rows, pf = [defs.six_floats(p) for p in aft], defs.key_pose(own[2])

def fill(c, n_slots):
    c.pose_graph_init(n_slots, FRAMES, MAX_LOOPS)
    for s in range(n_slots):
        for k in range(FRAMES):
            rc = L.lins_pose_graph_push(c._h, s, rows[k - 1] if k else None, rows[k])
            assert rc == k, rc
        assert L.lins_pose_graph_add_loop(c._h, s, own[0], own[1], C.byref(pf), 1e-6) == 0

def host_graphs(n):
    gs = []
    for _ in range(n):
        g = host.PoseGraph(FRAMES, MAX_LOOPS)
        cases.fill(g, dict(aft=aft, loops=[(own[0], own[1], own[2], 1e-6)]))
        gs.append(g)
    return gs

def stat(v):
    v = np.array(v)
    return f"{np.median(v):9.3f} ms [{v.min():9.3f} .. {v.max():9.3f}]"

say("team graph solve: HIP-event ms of the device sequence and wall ms of the whole call; median [min .. max] of %d runs after %d warm-up" % (REPS, WARM))
say("default parameters (lins_pose_graph_default_params); every run starts from freshly pushed graphs; %d frames a slot, 1 own loop a slot" % FRAMES)
with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
    for n_slots in (64, 256):
        dev, wall = [], []
        for run in range(WARM + REPS):
            fill(c, n_slots)
            t0 = time.perf_counter()
            res = c.pose_graph_solve(list(range(n_slots)))
            w = (time.perf_counter() - t0) * 1e3
            if run >= WARM:
                dev.append(c.pose_graph_stats()[0]); wall.append(w)
        say(f"  slots {n_slots:4d}  lins_pose_graph_solve (every slot alone, no factors)        device {stat(dev)}   whole call {stat(wall)}   "
            f"trials {sorted(set(r['iterations'] for r in res))}")
        for size in (1, 2, 4):
            for per_pair in ((0,) if size == 1 else (1, 4)):
                groups = [(list(range(g, g + size)), factors_of(list(range(g, g + size)), per_pair)) for g in range(0, n_slots, size)]
                dev, wall, res = [], [], None
                for run in range(WARM + REPS):
                    fill(c, n_slots)
                    t0 = time.perf_counter()
                    res = team.graph_solve(c, groups, root_variance=ROOT_VARIANCE)
                    w = (time.perf_counter() - t0) * 1e3
                    assert not isinstance(res, int), res
                    if run >= WARM:
                        dev.append(team.graph_stats(c)[0]); wall.append(w)
                gs = host_graphs(n_slots)
                t0 = time.perf_counter()
                hres = [host.team_graph_solve(gs[g:g + size], [(mb - g, ib, ma - g, ia, Z, var) for mb, ib, ma, ia, Z, var in groups[g // size][1]],
                                              None, ROOT_VARIANCE) for g in range(0, n_slots, size)]
                hw = (time.perf_counter() - t0) * 1e3
                del gs
                say(f"  slots {n_slots:4d}  groups of {size}  factors a pair {per_pair}  ({len(groups):3d} groups, {len(groups[0][1]) + size:2d} loops each)   "
                    f"device {stat(dev)}   whole call {stat(wall)}   trials {sorted(set(r['iterations'] for r in res))}  "
                    f"status {sorted(set(r['status'] for r in res))}  cost {res[0]['cost_before']:.4g} -> {res[0]['cost_after']:.4g}   "
                    f"host twin looped {hw:10.1f} ms  trials {sorted(set(r['iterations'] for r in hres))}")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
