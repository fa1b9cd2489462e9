#!/usr/bin/env python3
"""What the pairwise-consistent team factors cost (lins_team_factors_consistent_batch), and that what a caller already has
is unchanged; profiles/team_pcm_rate.txt and profiles/team_pcm_ab.txt keep one run each.  Medians of --runs with
min .. max after one warm-up, everything compared inside one run on the same context.  Nothing here is a pass bar.

    python tools/team_pcm_rate.py [--runs 5] [--out profiles/team_pcm_rate.txt]
  one lins_team_factors_consistent_batch at 1 / 64 / 256 groups: HIP-event ms of the launch and wall ms of the call (checks,
  records, upload, launch, download, synchronisation), against lins_host_team_factors_consistent looped over the same
  groups — both through ctypes on arrays packed beforehand; the records are compared bit for bit.  Two shapes:
    planted   groups of 16 and of 64 factors between two members: two thirds of them claim the identity (a planted
              clique), the others translations drawn on a 20 m segment beyond it, so that about 10 % of THEIR pairs agree
              (an interval graph stands in for random edges: claims are transforms, and agreement between them is
              nearly transitive); every line reports the share of those pairs that do agree, counted by the numpy
              checker of tests/team_pcm_np.py
    worst     the 63 factors of tests/team_pcm_cases.py duplicates(21), 21 frame pairs x 3 identical factors, at the default
              budget: the first subproblems run out of their 65 536 nodes

    python tools/team_pcm_rate.py --ab PARENT_LIB [--rounds 3] [--out profiles/team_pcm_ab.txt]
  the parent commit's library and this one's alternating in one visit, each run a process of its own: bench.py's headline
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
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def stat(v):
    return f"{statistics.median(v):9.3f} ms [{min(v):9.3f} .. {max(v):9.3f}]"


def main_ab(parent, out_path, rounds):
    say("What a caller already has: the parent commit's library and this branch's alternating in one visit (one MI355X), each run a")
    say("process of its own; bench.py's headline")
    for rnd in range(rounds):
        for name, lib in (("parent", parent), ("branch", "")):
            env = dict(os.environ)
            env.pop("LINS_IESKF_LIB", None)
            if lib:
                env["LINS_IESKF_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"], env=env,
                                 stdout=subprocess.PIPE, timeout=500, check=True)
            rec = json.loads([l for l in out.stdout.decode().splitlines() if l.startswith("{")][-1])
            say(f"  round {rnd + 1}  {name}  bench.py --gpus 1 --steps 20 --warmup 3: {rec['value']:.0f} {rec['unit']}  {rec['ms_per_step']:.4f} ms per step")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


def planted_factors(tpc, members, L, seed):
    """L factors with member indices: two thirds claim the identity, the others a translation on a segment 2 .. 22 m off
    -> (factors, the indices of the others)"""
    rng = np.random.default_rng(seed)
    inliers = set(rng.choice(L, size=(2 * L + 2) // 3, replace=False).tolist())
    fs = []
    for i in range(L):
        if i in inliers:
            fs.append(tpc.near(members, i, 1000 * seed + i))
        else:
            X = (np.eye(3), np.array([2.0 + 20.0 * rng.random(), 0.0, 0.0]))
            fs.append(tpc.factor(members, 0, i, 1, i, X, 0.02, 0.1, 1000 * seed + i))
    return fs, [i for i in range(L) if i not in inliers]


def others_density(tpn, pool, T):
    """the share of the pairs among a group's non-clique factors that are consistent, over the pool, by the numpy checker"""
    edges = pairs = 0
    for fs, others in pool:
        recs = tpn.records(fs, [T[f[0]][f[1]] for f in fs], [T[f[2]][f[3]] for f in fs])
        for a, l in enumerate(others):
            for m in others[a + 1:]:
                pairs += 1
                edges += bool(tpn.consistent(recs[l], recs[m], tpn.DEFAULTS))
    return edges, pairs


def main_rate(out_path, runs):
    import __graft_entry__ as g
    import pose_graph_cases as pgc
    import team_pcm_cases as tpc
    import team_pcm_np as tpn

    g.build()
    pkg, host, ieskf, team, defs = [importlib.import_module(PKG + m) for m in ("", ".host", ".ieskf", ".team", "._ctypes_defs")]
    L, Hl = ieskf.lib(), host.lib()
    Fac, Mem, Prm, Res = defs.TeamFactorC, defs.TeamMemberC, defs.TeamPcmParamsC, defs.TeamPcmResultC
    L.lins_team_factors_consistent_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(Mem), C.c_void_p, C.POINTER(Fac), C.c_void_p, C.POINTER(Prm), C.POINTER(Res)]
    Hl.lins_host_team_factors_consistent.argtypes = [C.c_int, C.POINTER(Fac), C.c_void_p, C.c_void_p, C.POINTER(Prm), C.POINTER(Res)]
    Hl.lins_host_team_factors_consistent.restype = C.c_int

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write("\n".join(lines) + "\n")

    say(f"Pairwise-consistent team factors, one MI355X, one visit; median [min .. max] of {runs} runs after a warm-up")
    say("one lins_team_factors_consistent_batch (device: HIP events around the launch; wall: the whole call) against")
    say("lins_host_team_factors_consistent looped over the same groups (host); default parameters; records equal bit for bit")
    members = tpc.pair_members(64)
    worst = (tpc.duplicates(21)[1], [])
    shapes = [("planted", 16, [planted_factors(tpc, members, 16, 1 + k) for k in range(8)]),
              ("planted", 64, [planted_factors(tpc, members, 64, 11 + k) for k in range(8)]),
              ("worst", 63, [worst])]
    n_max = 256
    prm = defs.team_pcm_params(L)
    with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
        c.pose_graph_init(2 * n_max, 64, 1)  # group e: slots 2 e and 2 e + 1, the same two trajectories in every group

        class Slot:
            def __init__(self, s):
                self.s = s

            def push(self, last6, aft6):
                return c.pose_graph_push(self.s, last6, aft6)

        for e in range(n_max):
            for k in (0, 1):
                pgc.fill(Slot(2 * e + k), dict(aft=members[k]["aft"], loops=[]))
        T = [c.debug_pose_graph_poses_f64(k) for k in (0, 1)]
        for name, per, pool in shapes:
            edges, pairs = others_density(tpn, pool, T)
            density = f"{100.0 * edges / pairs:4.1f} % of the others' {pairs} pairs agree" if pairs else "no others"
            for n in (1, 64, 256):
                dev_f, host_f, Tb, Ta = [], [], [], []
                for e in range(n):
                    for f in pool[e % len(pool)][0]:
                        host_f.append(defs.team_factor(f))
                        dev_f.append(defs.team_factor((2 * e + f[0], f[1], 2 * e + f[2], f[3], f[4], f[5])))
                        Tb.append(T[f[0]][f[1]]), Ta.append(T[f[2]][f[3]])
                darr, harr = (Fac * len(dev_f))(*dev_f), (Fac * len(host_f))(*host_f)
                Tb, Ta = np.ascontiguousarray(Tb), np.ascontiguousarray(Ta)
                marr = (Mem * (2 * n))(*[Mem(s, 0) for s in range(2 * n)])
                moff, foff = np.arange(n + 1, dtype=np.int32) * 2, np.arange(n + 1, dtype=np.int32) * per
                out, hout = (Res * n)(), (Res * n)()
                dev, wall, hst = [], [], []
                for r in range(runs + 1):
                    t0 = time.perf_counter()
                    assert L.lins_team_factors_consistent_batch(c._h, n, marr, moff.ctypes.data, darr, foff.ctypes.data, C.byref(prm), out) == 0
                    t1 = time.perf_counter()
                    for e in range(n):
                        rc = Hl.lins_host_team_factors_consistent(per, C.cast(C.byref(harr, e * per * C.sizeof(Fac)), C.POINTER(Fac)),
                                                                  Tb.ctypes.data + e * per * 96, Ta.ctypes.data + e * per * 96, C.byref(prm), C.byref(hout[e]))
                        assert rc == 0
                    t2 = time.perf_counter()
                    assert bytes(out) == bytes(hout)
                    if r:
                        dev.append(team.pcm_stats(c)), wall.append((t1 - t0) * 1e3), hst.append((t2 - t1) * 1e3)
                verdict = "the host wins" if statistics.median(hst) < statistics.median(wall) else "the device wins"
                kept = sorted(set(int(o.n_kept) for o in out))
                say(f"  {name:8s} {n:3d} groups x {per:2d} factors   device {stat(dev)}   wall {stat(wall)}   host {stat(hst)}   host / wall "
                    f"{statistics.median(hst) / statistics.median(wall):7.2f}   {verdict}   kept {kept[0]} .. {kept[-1]}, nodes_max <= {max(int(o.nodes_max) for o in out)}   {density}")
                flush()
    flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ab", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.ab:
        main_ab(a.ab, a.out or os.path.join(ROOT, "profiles", "team_pcm_ab.txt"), a.rounds)
    else:
        main_rate(a.out or os.path.join(ROOT, "profiles", "team_pcm_rate.txt"), a.runs)
