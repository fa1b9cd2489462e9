#!/usr/bin/env python3
"""lins_streams_map_step against the explicit chain it replaces (lins_map_associate_batch, lins_local_map_build_streams,
lins_scan2map_batch with LINS_MAP_LOCAL, host transform_update + key_rule, lins_local_map_push_scans,
lins_archive_push_scans — tests/map_step_chain.py explicit_step, the chain the tests hold the step against);
profiles/streams_map_step_rate.txt keeps one run.

Per stream count two contexts in ONE process take the same raw scans and the same transformSum rows, alternating: wall
time around the step and around the chain, median / min / max of --runs steps after --warmup, and the associate / finish
kernel times of lins_last_streams_map_ms.  The chain's wall time is given twice: whole (with the per-stream host
arithmetic, here Python over ctypes) and inside its five library calls only — the second is the one a C caller would
see, and the one the step is held against.  Both sides keep the build's synchronisation.

    python tools/streams_map_step_rate.py [--streams 64 256] [--out profiles/streams_map_step_rate.txt]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "lins---lidar-inertial-slam_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--distinct", type=int, default=32, help="distinct stock scans (repeated over the streams)")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streams_map_step_rate.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g

    g.build()
    pkg, host, ieskf, sm = (importlib.import_module(PKG + m) for m in ("", ".host", ".ieskf", ".streams_map"))
    import map_step_chain as ch

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stat(name, v):
        say(f"  {name}: median {statistics.median(v):9.4f} ms   min {min(v):9.4f}   max {max(v):9.4f}   ({len(v)} steps after {args.warmup} warm-up)")
        return statistics.median(v)

    distinct = [[host.synth_raw_scan(i, k) for i in range(args.distinct)] for k in range(2)]
    total = args.warmup + args.runs
    for ns in args.streams:
        streams = list(range(ns))
        st = np.zeros((ns, 19))
        st[:, 6] = 1.0
        cov = np.tile(np.eye(18)[None] * 1e-4, (ns, 1, 1))
        with ieskf.IeskfContext(pkg.default_params(num_iter=8), max_batch=ns, max_targets=16 * 1800) as a, \
                ieskf.IeskfContext(pkg.default_params(num_iter=8), max_batch=ns, max_targets=16 * 1800) as b:
            for c in (a, b):
                c.streams_init(ns)
                c.local_map_init(ns, args.window, 16384)
                c.archive_init(ns, total + 1, ns * (total + 1) * 8192)
            sm.init(a, ns, ch.INTERVAL)
            states = [ch.fresh_state() for _ in streams]
            w = dict(step=[], chain=[], calls=[], assoc=[], finish=[])
            keys = same = 0
            for r in range(total):
                raws = [distinct[r % 2][i % args.distinct] for i in streams]
                for c in (a, b):
                    c.streams_step_raw(raws, st, cov)
                odo = [(np.array([0.001 * r, 0.002 * r, 0.0, 0.01 * r, 0.0, 0.4 * r + 0.001 * i], np.float32), 0.4 * r, np.float32(0.01), np.float32(0.02), i % 2 == 0)
                       for i in streams]
                od = [sm.odom(*o) for o in odo]
                t0 = time.perf_counter()
                ra = sm.step(a, streams, od)
                t1 = time.perf_counter()
                clock = [0.0]
                rb = ch.explicit_step(b, states, streams, odo, clock=clock)
                t2 = time.perf_counter()
                same += all(ch.same_result(p, q) for p, q in zip(ra, rb))
                if r >= args.warmup:
                    ms = sm.last_ms(a)
                    w["step"].append((t1 - t0) * 1e3), w["chain"].append((t2 - t1) * 1e3), w["calls"].append(clock[0] * 1e3)
                    w["assoc"].append(ms[0]), w["finish"].append(ms[1])
                    keys += sum(x["key_frame"] for x in ra)
            say(f"{ns} streams, window {args.window}, {keys / args.runs:.1f} key frames per step; results equal bit for bit in {same} of {total} steps")
            m_s = stat("lins_streams_map_step, wall              ", w["step"])
            stat("explicit chain, wall (host part in Python)", w["chain"])
            m_c = stat("explicit chain, inside its library calls ", w["calls"])
            stat("map_associate_kernel (HIP events)        ", w["assoc"])
            stat("map_pose_finish_kernel (HIP events)      ", w["finish"])
            spread = max(w["calls"]) - min(w["calls"])
            say(f"  step {m_s:.4f} <= chain's library calls {m_c:.4f} + the chain's own spread {spread:.4f}: {'yes' if m_s <= m_c + spread else 'NO'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
