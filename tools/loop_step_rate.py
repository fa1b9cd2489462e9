#!/usr/bin/env python3
"""lins_loop_step against the explicit chain it replaces (lins_archive_find_loop, lins_archive_assemble,
lins_loop_icp_batch, lins_pose_graph_poses + lins_host_loop_pose_from, lins_pose_graph_add_loop, lins_pose_graph_solve,
lins_pose_graph_apply — tests/loop_step_cases.py explicit_chain, the chain the tests hold the step against), and
lins_pose_graph_apply_batch against n single applies; profiles/loop_step_rate.txt keeps one run.

Per slot count two contexts in ONE process hold the 12-frame loop case of the tests in every slot (archive, ring, graph,
one stream per slot), every slot closing its loop.  Each run starts from freshly pushed state on both, then, alternating:
one lins_loop_step over all slots on the first context, the chain slot by slot on the second.  Wall time around both — the
chain's twice: whole (with the decisions between the calls, here Python over ctypes) and inside its library calls only,
the one a C caller would see — and the HIP-event times of the step's three device sequences.  Then, on the closed graphs,
one lins_pose_graph_apply_batch against n lins_pose_graph_apply (the write-back is idempotent).  Medians of --runs runs
after --warmup, min .. max beside them.

    python tools/loop_step_rate.py [--slots 64 256] [--out profiles/loop_step_rate.txt]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "lins---lidar-inertial-slam_amd"


class Timed:
    """a context whose method calls add their seconds to clock[0]"""

    def __init__(self, ctx, clock):
        self._ctx, self._clock = ctx, clock

    def __getattr__(self, name):
        fn = getattr(self._ctx, name)

        def call(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self._clock[0] += time.perf_counter() - t0

        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_step_rate.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g

    g.build()
    pkg, ieskf, sm = (importlib.import_module(PKG + m) for m in ("", ".ieskf", ".streams_map"))
    import loop_step_cases as lsc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stat(name, v):
        say(f"  {name}: median {statistics.median(v):10.4f} ms   min {min(v):10.4f}   max {max(v):10.4f}   ({len(v)} runs after {args.warmup} warm-up)")
        return statistics.median(v)

    prm = lsc.params(ieskf.lib())
    for ns in args.slots:
        slots = list(range(ns))
        with ieskf.IeskfContext(pkg.default_params(), max_batch=ns, max_targets=1024) as a, \
                ieskf.IeskfContext(pkg.default_params(), max_batch=ns, max_targets=1024) as b:
            for c in (a, b):
                c.streams_init(ns)
            w = dict(step=[], chain=[], calls=[], assemble=[], icp=[], solve=[], batch=[], singles=[])
            closed = same = 0
            for r in range(args.warmup + args.runs):
                for c in (a, b):  # freshly pushed state: every init drops what the last run left
                    lsc.init(c, ns)
                    sm.init(c, ns)
                    for s in slots:
                        lsc.push(c, s, "loop")
                entries = [lsc.defs.loop_step_entry(s, lsc.centre(), lsc.NOW, stream=s) for s in slots]
                t0 = time.perf_counter()
                ra = a.loop_step(entries, prm)
                t1 = time.perf_counter()
                clock = [0.0]
                tb = Timed(b, clock)
                rb = [lsc.explicit_chain(tb, s, lsc.centre(), lsc.NOW, prm, stream=s) for s in slots]
                t2 = time.perf_counter()
                a.pose_graph_apply_batch(slots, slots)
                t3 = time.perf_counter()
                for s in slots:
                    b.pose_graph_apply(s, s)
                t4 = time.perf_counter()
                same += all(lsc.frozen(p) == lsc.frozen(q) for p, q in zip(ra, rb))
                if r >= args.warmup:
                    st = a.loop_step_stats()
                    w["step"].append((t1 - t0) * 1e3), w["chain"].append((t2 - t1) * 1e3), w["calls"].append(clock[0] * 1e3)
                    w["assemble"].append(st["assemble_ms"]), w["icp"].append(st["icp_ms"]), w["solve"].append(st["solve_ms"])
                    w["batch"].append((t3 - t2) * 1e3), w["singles"].append((t4 - t3) * 1e3)
                    closed += st["closed"]
            say(f"{ns} slots of 12 frames, {closed / args.runs:.1f} loops closed per step; results equal bit for bit in {same} of {args.warmup + args.runs} runs")
            m_s = stat("lins_loop_step, wall                        ", w["step"])
            stat("explicit chain, wall (decisions in Python)  ", w["chain"])
            m_c = stat("explicit chain, inside its library calls    ", w["calls"])
            stat("  assembly of 2 n submaps (HIP events)      ", w["assemble"])
            stat("  alignment of n problems (HIP events)      ", w["icp"])
            stat("  solve of n graphs (HIP events)            ", w["solve"])
            m_b = stat("lins_pose_graph_apply_batch, wall           ", w["batch"])
            m_n = stat(f"{ns:3d} x lins_pose_graph_apply, wall            ", w["singles"])
            say(f"  step / chain's library calls: {m_s / m_c:.3f}   (chain's own spread {max(w['calls']) - min(w['calls']):.4f} ms)")
            say(f"  apply_batch / single applies: {m_b / m_n:.3f}   (singles' own spread {max(w['singles']) - min(w['singles']):.4f} ms)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
