#!/usr/bin/env python3
"""What the team map costs (lins_keyposes_team_select_batch, lins_local_map_build_team, lins_streams_map_team), and that
what a caller already has is unchanged; profiles/team_map_rate.txt and profiles/team_map_ab.txt keep one run each.
Medians of --runs with min .. max, everything compared inside one run on the same context and poses.

    python tools/team_map_rate.py [--runs 5] [--out profiles/team_map_rate.txt]
  selection  lins_keyposes_team_select_batch at 1 / 64 / 256 entries over groups of 1 / 4 / 16 slots x 2 000 key poses,
             layouts of tools/keypose_select_rate.py (exploring, yard): HIP-event ms and wall ms, against
             lins_host_team_select looped over the same entries, and for a group of one against lins_keyposes_select_batch
  build      lins_local_map_build_team against lins_local_map_build_surround of the same number of frames
  step       lins_streams_map_step with the team mode on (groups of 1 and of 4) against surround mode, 64 and 256 streams

    python tools/team_map_rate.py --ab PARENT_LIB [--out profiles/team_map_ab.txt]
  the parent commit's library and this one's alternating in one visit, each run a process of its own:
  lins_local_map_build, lins_local_map_build_surround, lins_streams_map_step in surround mode, bench.py's headline
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "lins---lidar-inertial-slam_amd"
RADIUS, LEAF, NPOSE = 50.0, 1.0, 2000
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def stat(v):
    return f"{statistics.median(v):9.3f} ms [{min(v):9.3f} .. {max(v):9.3f}]"


def mods():
    return [importlib.import_module(PKG + m) for m in ("", ".host", ".ieskf", ".streams_map", ".team", "._ctypes_defs")]


def frames_and_scans(n_frames, n_scans):
    from local_map_synth import room_scan, trajectory

    poses = trajectory(n_frames, seed=4)
    kw = dict(n_corner=300, n_surf=1100, n_outlier=100)
    return [room_scan(400 + i, poses[i], **kw) + (poses[i],) for i in range(n_frames)], [room_scan(980 + k, poses[k % n_frames], **kw) for k in range(n_scans)]


def step_context(pkg, ieskf, host, defs, ns, npose, steps):
    """ns streams whose archives hold npose one-point key frames each (the yard layout), ready for lins_streams_map_step"""
    from keypose_select_rate import layout_xy

    L = ieskf.lib()
    L.lins_archive_push.argtypes = [C.c_void_p, C.c_int, C.POINTER(defs.KeyframeC), C.c_double]
    c = ieskf.IeskfContext(pkg.default_params(num_iter=8), max_batch=ns, max_targets=16 * 1800)
    c.streams_init(ns)
    c.local_map_init(ns, 3, 16384)
    c.archive_init(ns, npose + steps + 8, ns * (npose + steps * 16384))
    xy = layout_xy("yard", npose, np.random.default_rng(3))
    frame, _keep = defs.keyframe_c(np.array([[0.1, 0.2, 0.3, 0.0]], np.float32), np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32),
                                   np.zeros(6, np.float32))
    for i in range(npose):
        frame.pose.x, frame.pose.y = float(xy[i, 0]), float(xy[i, 1])
        for s in range(ns):
            assert L.lins_archive_push(c._h, s, C.byref(frame), 0.1 * i) == i
    raws = [host.synth_raw_scan(i, 0) for i in range(4)]
    st = np.zeros((ns, 19))
    st[:, 6] = 1.0
    cov = np.tile(np.eye(18)[None] * 1e-4, (ns, 1, 1))
    return c, raws, st, cov


# ---- what a caller already has: one process per library -----------------------------------------------------------------
def main_child(runs):
    pkg, host, ieskf, sm, _, defs = mods()
    fr, scans = frames_and_scans(8, 16)
    with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
        c.local_map_init(16, 3, 4096)
        c.archive_init(16, 8, 1 << 18)
        for s in range(16):
            for i, f in enumerate(fr):
                assert c.archive_push(s, *f[:3], f[3], time=float(i)) == i
            for f in fr[:3]:
                c.local_map_push(s, *f)
        ring, sur = [], []
        for r in range(runs + 1):
            c.local_map_build(list(range(16)), scans)
            a = c.local_map_stats()[0]
            c.local_map_build_surround(list(range(16)), [list(range(8))] * 16, scans)
            b = c.local_map_stats()[0]
            if r:
                ring.append(a), sur.append(b)
        print(f"child lins_local_map_build, 16 entries x 3 ring frames             device {stat(ring)}", flush=True)
        print(f"child lins_local_map_build_surround, 16 entries x 8 listed frames  device {stat(sur)}", flush=True)
    ns = 64
    c, raws, st, cov = step_context(pkg, ieskf, host, defs, ns, 500, 2 + runs)
    sm.init(c, ns, 0.3)
    sm.surround(c, True, RADIUS, LEAF)
    w = []
    for r in range(2 + runs):
        c.streams_step_raw([raws[(i + r) % 4] for i in range(ns)], st, cov)
        od = [sm.odom(np.zeros(6, np.float32), 0.4 * (r + 1)) for _ in range(ns)]
        t0 = time.perf_counter()
        out = sm.step(c, list(range(ns)), od)
        t1 = time.perf_counter()
        assert all(o["status"] == 0 for o in out)
        if r >= 2:
            w.append((t1 - t0) * 1e3)
    c.close()
    print(f"child lins_streams_map_step in surround mode, 64 streams x 500 key poses  wall {stat(w)}", flush=True)


def main_ab(parent, out_path, runs):
    say("What a caller already has: the parent commit's library and this branch's alternating in one visit (one MI355X), each run a")
    say(f"process of its own; median [min .. max] of {runs} runs after the warm-up")
    for rnd in range(2):
        for name, lib in (("parent", parent), ("branch", "")):
            env = dict(os.environ)
            env.pop("LINS_IESKF_LIB", None)
            if lib:
                env["LINS_IESKF_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(runs)], env=env, stdout=subprocess.PIPE,
                                 timeout=500, check=True)
            for l in out.stdout.decode().splitlines():
                if l.startswith("child "):
                    say(f"  round {rnd + 1}  {name}  {l[6:]}")
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"], env=env,
                                 stdout=subprocess.PIPE, timeout=500, check=True)
            rec = json.loads([l for l in out.stdout.decode().splitlines() if l.startswith("{")][-1])
            say(f"  round {rnd + 1}  {name}  bench.py --gpus 1 --steps 20 --warmup 3: {rec['value']:.0f} {rec['unit']}  {rec['ms_per_step']:.4f} ms per step")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


# ---- the team map's own figures ------------------------------------------------------------------------------------------
def main_rate(out_path, runs):
    import __graft_entry__ as g
    from keypose_select_rate import layout_xy

    g.build()
    pkg, host, ieskf, sm, team, defs = mods()
    L, H = ieskf.lib(), host.lib()
    Q, TQ, R = defs.KeyposesQueryC, defs.KeyposesTeamQueryC, defs.KeyposesResultC
    vp = C.c_void_p
    L.lins_archive_push.argtypes = [vp, C.c_int, C.POINTER(defs.KeyframeC), C.c_double]
    L.lins_keyposes_team_select_batch.argtypes = [vp, C.c_int, C.POINTER(TQ), vp, C.c_int, vp, C.c_int, C.POINTER(R)]
    L.lins_keyposes_select_batch.argtypes = [vp, C.c_int, C.POINTER(Q), vp, C.c_int, C.POINTER(R)]
    H.lins_host_team_select.argtypes = [C.c_int, vp, vp, vp, C.POINTER(C.c_float), C.c_float, C.c_float, vp, C.c_int]
    H.lins_host_team_select.restype = C.c_int

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write("\n".join(lines) + "\n")

    say(f"The team map, one MI355X, one visit; median [min .. max] of {runs} runs after a warm-up; radius {RADIUS:g} m, pose leaf {LEAF:g} m")
    say("")
    say(f"selection: lins_keyposes_team_select_batch over 16 slots x {NPOSE} key poses (one point a frame); entry k asks the g slots from (k g) mod 16 on")
    NS = 16
    rng = np.random.default_rng(3)
    for layout in ("exploring", "yard"):
        xy = layout_xy(layout, NPOSE, rng)
        with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
            c.archive_init(NS, NPOSE, NS * NPOSE + 1)
            frame, _keep = defs.keyframe_c(np.array([[0.1, 0.2, 0.3, 0.0]], np.float32), np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32),
                                           np.zeros(6, np.float32))
            kp = (defs.KeyPoseC * NPOSE)()
            for i in range(NPOSE):
                frame.pose.x, frame.pose.y = float(xy[i, 0]), float(xy[i, 1])
                kp[i].x, kp[i].y = float(xy[i, 0]), float(xy[i, 1])
                for s in range(NS):
                    assert L.lins_archive_push(c._h, s, C.byref(frame), 0.1 * i) == i
            centre = (C.c_float * 3)(0.0, 0.0, 0.0)
            say(f"{layout}")
            for grp in (1, 4, 16):
                for n in (1, 64, 256):
                    table = np.array([(k * grp + t) % NS for k in range(n) for t in range(grp)], np.int32)
                    qs = (TQ * n)(*[defs.keyposes_team_query((0, 0, 0), RADIUS, LEAF, grp, k * grp) for k in range(n)])
                    res, stride = (R * n)(), grp * NPOSE
                    pairs = np.zeros((n, stride, 2), np.int32)
                    hp = np.zeros((stride, 2), np.int32)
                    pp, cnt = (vp * grp)(*[C.addressof(kp)] * grp), np.full(grp, NPOSE, np.int32)
                    dev, wall, hst, one_d, one_w = [], [], [], [], []
                    for r in range(runs + 1):
                        t0 = time.perf_counter()
                        assert L.lins_keyposes_team_select_batch(c._h, n, qs, table.ctypes.data, len(table), pairs.ctypes.data, stride, res) == 0
                        t1 = time.perf_counter()
                        ms = team.select_stats(c)
                        for k in range(n):
                            nh = H.lins_host_team_select(grp, table[k * grp:].ctypes.data, pp, cnt.ctypes.data, centre, RADIUS, LEAF, hp.ctypes.data, stride)
                        t2 = time.perf_counter()
                        assert nh == res[n - 1].n and np.array_equal(hp[:nh], pairs[n - 1, :nh]) and ms["host_entries"] == 0
                        if grp == 1:
                            q1 = (Q * n)(*[defs.keyposes_query(int(table[k]), (0, 0, 0), RADIUS, LEAF) for k in range(n)])
                            ids = np.zeros((n, NPOSE), np.int32)
                            t3 = time.perf_counter()
                            assert L.lins_keyposes_select_batch(c._h, n, q1, ids.ctypes.data, NPOSE, res) == 0
                            t4 = time.perf_counter()
                            if r:
                                one_d.append(c.keyposes_stats()["device_ms"]), one_w.append((t4 - t3) * 1e3)
                            assert L.lins_keyposes_team_select_batch(c._h, n, qs, table.ctypes.data, len(table), pairs.ctypes.data, stride, res) == 0
                        if r:
                            dev.append(ms["device_ms"]), wall.append((t1 - t0) * 1e3), hst.append((t2 - t1) * 1e3)
                    say(f"  group of {grp:2d}, {n:3d} entries ({res[n - 1].hits} hits, {res[n - 1].n} selected an entry)")
                    say(f"      device {stat(dev)}   wall {stat(wall)}   host text {stat(hst)}   host / wall {statistics.median(hst) / statistics.median(wall):7.2f}")
                    if grp == 1:
                        say(f"      lins_keyposes_select_batch (the node's rule, one slot): device {stat(one_d)}   wall {stat(one_w)}")
                    flush()
    say("")
    say("build: 16 entries, each over 8 listed frames of 1 500 points; the team lists alternate between two slots that hold the same frames")
    fr, scans = frames_and_scans(8, 16)
    with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
        c.local_map_init(16, 3, 4096)
        c.archive_init(16, 8, 1 << 18)
        for s in range(16):
            for i, f in enumerate(fr):
                assert c.archive_push(s, *f[:3], f[3], time=float(i)) == i
        slots = list(range(16))
        ids = [list(range(8))] * 16
        prs = [[(s if i % 2 else (s + 1) % 16, i) for i in range(8)] for s in slots]
        t = dict(sd=[], sw=[], td=[], tw=[])
        for r in range(runs + 1):
            t0 = time.perf_counter()
            a = c.local_map_build_surround(slots, ids, scans)
            t1 = time.perf_counter()
            sd = c.local_map_stats()[0]
            t2 = time.perf_counter()
            b = c.local_map_build_team(slots, prs, scans)
            t3 = time.perf_counter()
            assert a == b
            if r:
                t["sd"].append(sd), t["sw"].append((t1 - t0) * 1e3), t["td"].append(c.local_map_stats()[0]), t["tw"].append((t3 - t2) * 1e3)
        say(f"  lins_local_map_build_surround  device {stat(t['sd'])}   wall {stat(t['sw'])}")
        say(f"  lins_local_map_build_team      device {stat(t['td'])}   wall {stat(t['tw'])}")
        flush()
    say("")
    say(f"step: lins_streams_map_step, wall ms around the call; {NPOSE} one-point key frames a stream (yard); the modes on alternate steps")
    for ns in (64, 256):
        kinds = ("surround", "team, alone", "team, groups of 4")
        steps = 2 + len(kinds) * runs
        c, raws, st, cov = step_context(pkg, ieskf, host, defs, ns, NPOSE, 2 * steps)
        sm.init(c, ns, 0.3)
        for mode in (defs.KEYPOSES_HOST, defs.KEYPOSES_DEVICE):
            c.keyposes_set_mode(mode)
            w = {k: [] for k in kinds}
            listed = {}
            for r in range(steps):
                kind = kinds[r % len(kinds)]
                assert sm.team(c, False) == 0
                sm.surround(c, False)
                if kind == "surround":
                    sm.surround(c, True, RADIUS, LEAF)
                else:
                    assert sm.team(c, True, RADIUS, LEAF) == 0
                    assert sm.team_groups(c, list(range(ns)), [s // 4 if kind.endswith("4") else -1 for s in range(ns)]) == 0
                c.streams_step_raw([raws[(i + r) % 4] for i in range(ns)], st, cov)
                od = [sm.odom(np.zeros(6, np.float32), 0.4 * (r + 1) + (1e4 if mode else 0)) for _ in range(ns)]
                t0 = time.perf_counter()
                out = sm.step(c, list(range(ns)), od)
                t1 = time.perf_counter()
                assert all(o["status"] == 0 for o in out)
                listed[kind] = len(sm.surround_list(c, 0)) if kind == "surround" else len(sm.team_list(c, 0))
                if r >= len(kinds):
                    w[kind].append((t1 - t0) * 1e3)
            say(f"  {ns} streams, selection {'on the device' if mode else 'on the host'}")
            for k in kinds:
                say(f"      {k:18s} {stat(w[k])}   {listed[k]} frames listed")
            flush()
        c.close()
    flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ab", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        main_child(a.runs)
    elif a.ab:
        main_ab(a.ab, a.out or os.path.join(ROOT, "profiles", "team_map_ab.txt"), a.runs)
    else:
        main_rate(a.out or os.path.join(ROOT, "profiles", "team_map_rate.txt"), a.runs)
