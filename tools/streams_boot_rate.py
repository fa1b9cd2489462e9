#!/usr/bin/env python3
"""What the two-scan bootstrap of the device-resident streams costs (lins_streams_process_raw, lins_streams_boot_stats)
against the way the same work was done before it existed: the ICP of every stream's second scan through
lins_icp_update_batch on the downloaded clouds (what the divergence fallback does stream by stream), the rest on the host.
profiles/streams_boot_rate.txt keeps one run.

Per stream count: every stream takes scan 0 and scan 1 of a stock synthetic sequence (11, 12, 13 in turn); the three
HIP-event times of the call that takes the second scans — pre-integration kernel, bootstrap ICP (index of the first scans'
clouds, start rows, the ONE batched ICP launch), finish kernel — and the call's wall time, median / min / max of --runs
runs after --warmup (lins_streams_machine_init starts every run anew).  Beside them the wall time of
lins_icp_update_batch over the same clouds from the same start poses (upload, index, ICP, download), one stream at a
time as the fallback launches it, and as one batch.

    python tools/streams_boot_rate.py [--streams 64 256] [--out profiles/streams_boot_rate.txt]
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streams_boot_rate.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g

    g.build()
    pkg, host, ieskf, defs = (importlib.import_module(PKG + m) for m in ("", ".host", ".ieskf", "._ctypes_defs"))
    import boot_common as bc

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stat(name, v):
        say(f"  {name}: median {statistics.median(v):9.4f} ms   min {min(v):9.4f}   max {max(v):9.4f}   ({len(v)} runs after {args.warmup} warm-up)")

    seqs = [bc.load(host, s, 2) for s in bc.SEQS]
    prm = pkg.default_params(num_iter=30)
    # the parent's route needs the clouds on the host: the host front-end's (bit-equal to the device's) and the start poses
    pairs3 = []
    for s in seqs:
        f0, f1 = host.frontend_extract(s["raws"][0]), host.frontend_extract(s["raws"][1])
        pl, ql = bc.host_bootstrap(host, s)["start"]
        st = np.zeros(19)
        st[0:3], st[6:10], st[18] = pl, ql, -9.81
        pairs3.append(defs.ScanPair(f1["surf_flat"], f1["corner_sharp"], f0["surf_less_flat"], f0["corner_less_sharp"], st, np.eye(18) * 1e-4))
    total = args.warmup + args.runs
    for ns in args.streams:
        of = [seqs[i % 3] for i in range(ns)]
        pairs = [pairs3[i % 3] for i in range(ns)]
        w = dict(pre=[], icp=[], fin=[], wall=[], dev=[], one=[], batch=[])
        with ieskf.IeskfContext(prm, max_batch=ns, max_targets=16 * 1800) as ctx:
            ctx.streams_init(ns)
            for r in range(total):
                ctx.streams_machine_init()
                ctx.streams_process_raw([s["raws"][0] for s in of], [s["rows"][0] for s in of], [0.1] * ns)
                t0 = time.perf_counter()
                res, _, _, status = ctx.streams_process_raw([s["raws"][1] for s in of], [s["rows"][1] for s in of], [0.2] * ns)
                t1 = time.perf_counter()
                assert all(v == defs.STREAM_RUNNING for v in status)
                pm, im, fm = ctx.streams_boot_stats()
                if r >= args.warmup:
                    w["pre"].append(pm), w["icp"].append(im), w["fin"].append(fm), w["wall"].append((t1 - t0) * 1e3), w["dev"].append(sum(ctx.streams_stats()))
            rounds = [r.iters for r in res[:3]]
        with ieskf.IeskfContext(prm, max_batch=ns, max_targets=16 * 1800) as ctx:
            for r in range(total):
                t0 = time.perf_counter()
                for p in pairs:
                    ctx.icp_update_batch([p])
                t1 = time.perf_counter()
                ctx.icp_update_batch(pairs)
                t2 = time.perf_counter()
                if r >= args.warmup:
                    w["one"].append((t1 - t0) * 1e3), w["batch"].append((t2 - t1) * 1e3)
        say(f"{ns} streams taking their second scan (sequences 11 / 12 / 13 in turn; ICP rounds of the first three: {rounds})")
        stat("boot_preintegrate_kernel, 40 rows a stream (HIP events)  ", w["pre"])
        stat("index + start rows + ONE batched ICP launch (HIP events) ", w["icp"])
        stat("boot_finish_kernel (HIP events)                          ", w["fin"])
        stat("lins_streams_process_raw, wall (front-end, ... included) ", w["wall"])
        stat("  of which front-end + update + re-projection (HIP events)", w["dev"])
        stat("before: lins_icp_update_batch stream by stream, wall     ", w["one"])
        stat("before: lins_icp_update_batch as one batch, wall         ", w["batch"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
