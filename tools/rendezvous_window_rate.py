#!/usr/bin/env python3
"""What a rendezvous over a window costs (lins_rendezvous_consensus_batch, lins_rendezvous_window_step), and that what a
caller already has is unchanged; profiles/rendezvous_window_rate.txt and profiles/rendezvous_window_ab.txt keep one run
each.  Medians of --runs with min .. max after one warm-up, everything compared inside one run on the same context.

    python tools/rendezvous_window_rate.py [--runs 5] [--out profiles/rendezvous_window_rate.txt]
  consensus  one lins_rendezvous_consensus_batch at 1 / 64 / 256 entries x 16 / 64 / 128 hypotheses (two clusters of X, as
             tests/rendezvous_window_np.py sized()): HIP-event ms of the launch and wall ms of the call (upload, launch,
             download, synchronisation), against lins_host_rendezvous_consensus looped over the same entries — both through
             ctypes on tables packed beforehand
  step       lins_rendezvous_window_step at 64 and 256 entries for windows of 1 / 5 / 8 frames (k = 4, shortlist 8), wall ms
             and the stage times of lins_last_rendezvous_window_stats, against lins_rendezvous_step over the same entries.
             Fixture: slot s holds the twelve frames of slot s mod 4 of tests/rendezvous_window_cases.py; every slot is a
             target.  Slots s and s + 4 are copies, so every entry meets itself: the outcomes say nothing, the times do.

    python tools/rendezvous_window_rate.py --ab PARENT_LIB [--out profiles/rendezvous_window_ab.txt]
  the parent commit's library and this one's alternating in one visit, each run a process of its own:
  lins_rendezvous_step at 64 entries on the same fixture, and bench.py's headline
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


def mods():
    return [importlib.import_module(PKG + m) for m in ("", ".host", ".ieskf", ".team", "._ctypes_defs")]


def fixture_context(pkg, ieskf, n_slots):
    """n_slots slots, slot s with the twelve frames of slot s mod 4 of the window fixture, place store on"""
    import rendezvous_window_cases as rwc

    fr = rwc.slots()
    per = max(sum(len(x) for f in fr[s] for x in f[:3]) for s in fr)
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    c.archive_init(n_slots, 16, n_slots * per + 16)
    for s in range(n_slots):
        for i, f in enumerate(fr[s % 4]):
            assert c.archive_push(s, *f[:3], tuple(float(v) for v in f[3]), time=float(i)) == i
    assert c.place_init(up_axis=rwc.UP) == 0 and c.place_sync(list(range(n_slots))) == 0
    return c, rwc


def loop_params(ieskf, rwc):
    import loop_step_cases as lsc

    return lsc.params(ieskf.lib(), min_gap_s=rwc.GAP, search_num=rwc.H)


def lone_step(team, c, rwc, prm, n):
    t0 = time.perf_counter()
    r = team.rendezvous_step(c, [(s, rwc.NOW) for s in range(n)], list(range(n)), prm, shortlist=rwc.M, k=rwc.K)
    t1 = time.perf_counter()
    assert isinstance(r, list)
    return (t1 - t0) * 1e3, r


# ---- what a caller already has: one process per library -----------------------------------------------------------------
def main_child(runs):
    pkg, host, ieskf, team, defs = mods()
    c, rwc = fixture_context(pkg, ieskf, 64)
    prm = loop_params(ieskf, rwc)
    w = []
    for r in range(runs + 1):
        ms, res = lone_step(team, c, rwc, prm, 64)
        if r:
            w.append(ms)
    found = sum(x["outcome"] == defs.RENDEZVOUS_FOUND for x in res)
    c.close()
    print(f"child lins_rendezvous_step, 64 entries x 64 target slots of 12 frames ({found} found)  wall {stat(w)}", flush=True)


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


# ---- the window's own figures --------------------------------------------------------------------------------------------
def main_rate(out_path, runs):
    import __graft_entry__ as g
    import rendezvous_window_np as rw

    g.build()
    pkg, host, ieskf, team, defs = mods()
    L, Hl = ieskf.lib(), host.lib()
    Hyp, Prm, Res = defs.ConsensusHypC, defs.ConsensusParamsC, defs.ConsensusResultC
    L.lins_rendezvous_consensus_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(Hyp), C.c_void_p, C.POINTER(Prm), C.POINTER(Res)]
    Hl.lins_host_rendezvous_consensus.argtypes = [C.POINTER(Hyp), C.c_int, C.POINTER(Prm), C.POINTER(Res)]
    Hl.lins_host_rendezvous_consensus.restype = C.c_int

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write("\n".join(lines) + "\n")

    say(f"Rendezvous over a window, one MI355X, one visit; median [min .. max] of {runs} runs after a warm-up")
    say("")
    say("consensus: one lins_rendezvous_consensus_batch (device: HIP events around the launch; wall: the whole call) against")
    say("lins_host_rendezvous_consensus looped over the same entries (host); every entry a table of its own, results equal bit for bit")
    prm = defs.consensus_params(L)
    with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
        for H in (16, 64, 128):
            pool = [rw.sized(H, seed=100 + k) for k in range(8)]  # (eight distinct tables, repeated)
            for n in (1, 64, 256):
                flat = [h for e in range(n) for h in pool[e % 8]]
                arr = defs.consensus_table(flat)
                off = np.arange(n + 1, dtype=np.int32) * H
                out, hout = (Res * n)(), (Res * n)()
                dev, wall, hst = [], [], []
                for r in range(runs + 1):
                    t0 = time.perf_counter()
                    assert L.lins_rendezvous_consensus_batch(c._h, n, arr, off.ctypes.data, C.byref(prm), out) == 0
                    t1 = time.perf_counter()
                    for e in range(n):
                        Hl.lins_host_rendezvous_consensus(C.cast(C.byref(arr, e * H * C.sizeof(Hyp)), C.POINTER(Hyp)), H, C.byref(prm), C.byref(hout[e]))
                    t2 = time.perf_counter()
                    assert bytes(out) == bytes(hout)
                    if r:
                        dev.append(team.consensus_stats(c)), wall.append((t1 - t0) * 1e3), hst.append((t2 - t1) * 1e3)
                verdict = "the host wins" if statistics.median(hst) < statistics.median(wall) else "the device wins"
                say(f"  {n:3d} entries x {H:3d} hypotheses   device {stat(dev)}   wall {stat(wall)}   host {stat(hst)}   host / wall "
                    f"{statistics.median(hst) / statistics.median(wall):7.2f}   {verdict}")
                flush()
    say("")
    say("step: lins_rendezvous_window_step, wall ms around the call and the stages of lins_last_rendezvous_window_stats (host clock);")
    say("every slot an entry and a target, 12 frames a slot, k = 4, shortlist 8, default bars.  wall: around the Python wrapper, which also")
    say("turns every record into a dict; total: inside the C call.  Slots s and s + 4 hold the same frames at the same stored poses, so")
    say("every slot meets copies of itself and is found, slot 3's copies included: the outcomes say nothing here, the times do.")
    for n in (64, 256):
        c, rwc = fixture_context(pkg, ieskf, n)
        lp = loop_params(ieskf, rwc)
        entries, targets = [(s, rwc.NOW) for s in range(n)], list(range(n))
        w = []
        for r in range(runs + 1):
            ms, res = lone_step(team, c, rwc, lp, n)
            if r:
                w.append(ms)
        say(f"  {n} entries")
        say(f"      lins_rendezvous_step (one frame)      wall {stat(w)}   {sum(x['outcome'] == defs.RENDEZVOUS_FOUND for x in res)} found, "
            f"{sum(x['n_candidates'] for x in res)} alignments")
        for W in (1, 5, 8):
            w, st = [], {k: [] for k in ("detect_ms", "assemble_ms", "align_ms", "consensus_ms", "total_ms")}
            for r in range(runs + 1):
                t0 = time.perf_counter()
                res = team.rendezvous_window_step(c, entries, targets, lp, dict(window=W, min_support=min(3, W)), shortlist=rwc.M, k=rwc.K)
                t1 = time.perf_counter()
                assert isinstance(res, list)
                if r:
                    w.append((t1 - t0) * 1e3)
                    s = team.rendezvous_window_stats(c)
                    for k in st:
                        st[k].append(s[k])
            outcomes = [sum(x["outcome"] == o for x in res) for o in (defs.RENDEZVOUS_FOUND, defs.RENDEZVOUS_UNCONFIRMED, defs.RENDEZVOUS_REJECTED)]
            say(f"      window {W}, min_support {min(3, W)}               wall {stat(w)}   {outcomes[0]} found, {outcomes[1]} unconfirmed, "
                f"{outcomes[2]} rejected, {sum(x['n_hypotheses'] for x in res)} alignments")
            say("          " + "   ".join(f"{k[:-3]} {stat(v)}" for k, v in st.items()))
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
        main_ab(a.ab, a.out or os.path.join(ROOT, "profiles", "rendezvous_window_ab.txt"), a.runs)
    else:
        main_rate(a.out or os.path.join(ROOT, "profiles", "rendezvous_window_rate.txt"), a.runs)
