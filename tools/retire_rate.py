#!/usr/bin/env python3
"""What retiring streams costs in the key-frame archive (lins_archive_release_slots: the arena's compaction on the
device, csrc/archive_kernels.hip ar_reclaim_*); profiles/retire_rate.txt keeps one run.  Device time (HIP events) of one
reclaim, and next to it the yardstick: two plain device-to-device hipMemcpyAsync copies of the same moved bytes, out to a
scratch buffer and back, timed by HIP events on the null stream.  The two alternate in one process; medians of --runs
with min .. max.

The arena: --slots slots of --frames key frames of --points points (a downsampled VLP-16 key frame with its outliers
keeps 4 - 5 k points).  Robots join one after the other, slot s --stagger frames behind slot s - 1, and the frames of
the robots that run at the same time interleave — so an early slot's release moves nearly the whole arena down and a
late slot's only the tail.  Cases: one early slot (slot 0), one late slot (the last), eight slots spread over the fleet.
The archive is initialised and filled anew before every run (not timed): every run compacts the same layout.

    python tools/retire_rate.py [--slots 64] [--frames 40] [--points 4600] [--stagger 5] [--runs 5] [--chunk 0] [--out profiles/retire_rate.txt]
"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "lins---lidar-inertial-slam_amd"
D2D = 3  # hipMemcpyDeviceToDevice


def hip_runtime():
    for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64.so not found")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--points", type=int, default=4600)
    ap.add_argument("--stagger", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=0, help="points per compaction pass (0: the library's default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retire_rate.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g

    g.build()
    pkg, ieskf, defs = (importlib.import_module(PKG + m) for m in ("", ".ieskf", "._ctypes_defs"))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    L, hip = ieskf.lib(), hip_runtime()
    L.lins_archive_push.argtypes = [C.c_void_p, C.c_int, C.POINTER(defs.KeyframeC), C.c_double]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    ns, nf = args.slots, args.frames
    n_corner, n_outl = args.points // 9, args.points // 3
    n_surf = args.points - n_corner - n_outl
    rng = np.random.default_rng(5)
    clouds = [np.concatenate([rng.uniform(-30, 30, (n, 3)), rng.uniform(0, 16, (n, 1))], 1).astype(np.float32) for n in (n_corner, n_surf, n_outl)]
    frame, _keep = defs.keyframe_c(clouds[0], clouds[1], clouds[2], np.zeros(6, np.float32))
    # the order of the pushes: at time t every robot that is running stores one frame
    order = [(s, t - s * args.stagger) for t in range((ns - 1) * args.stagger + nf) for s in range(ns) if 0 <= t - s * args.stagger < nf]
    total = ns * nf * args.points
    cases = [("one early slot (0)", [0]), (f"one late slot ({ns - 1})", [ns - 1]),
             ("eight slots", sorted({(ns * i) // 8 for i in range(8)}))]

    with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
        a, b, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        ok(hip.hipMalloc(C.byref(a), total * 16)), ok(hip.hipMalloc(C.byref(b), total * 16))
        ok(hip.hipMemset(a, 0, total * 16)), ok(hip.hipMemset(b, 0, total * 16))
        ok(hip.hipEventCreate(C.byref(e0))), ok(hip.hipEventCreate(C.byref(e1)))

        def fill():
            c.archive_init(ns, nf, total)
            for s, i in order:
                assert L.lins_archive_push(c._h, s, C.byref(frame), 0.1 * i) == i

        def copies(points):
            """two plain device-to-device copies of `points` points: out and back"""
            ms = C.c_float(0)
            ok(hip.hipEventRecord(e0, None))
            ok(hip.hipMemcpyAsync(b, a, points * 16, D2D, None))
            ok(hip.hipMemcpyAsync(a, b, points * 16, D2D, None))
            ok(hip.hipEventRecord(e1, None))
            ok(hip.hipEventSynchronize(e1))
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
            return ms.value

        c.archive_set_reclaim_chunk(args.chunk)
        say(f"{ns} slots x {nf} frames x {args.points} points = {total} points ({total * 16 / 2 ** 20:.0f} MiB) in the arena, slot s joins "
            f"{args.stagger} frames behind slot s - 1; reclaim chunk {args.chunk or 'default (2^20 points)'}")
        say(f"device ms (HIP events), median (min .. max) of {args.runs}; reclaim: lins_archive_release_slots' passes; copies: two "
            f"hipMemcpyAsync device-to-device of the moved bytes, out to scratch and back")
        for name, slots in cases:
            rc, cp, st = [], [], None
            for run in range(args.runs + 1):  # (the first round loads code and allocates the staging buffer: not kept)
                fill()
                freed = c.archive_release_slots(slots)
                st = c.reclaim_stats()
                assert freed == len(slots) * nf * args.points and c.archive_usage()[0] == total - freed
                t = copies(max(st["points_moved"], 1))
                if run:
                    rc.append(st["ms"]), cp.append(t)
            mb = st["points_moved"] * 16 / 2 ** 20
            mr, mc = statistics.median(rc), statistics.median(cp)
            say(f"  {name}: {st['points_moved']} points moved ({mb:.0f} MiB), {st['staged_passes']} staged + {st['direct_passes']} direct passes")
            say(f"    reclaim {mr:8.3f} ms ({min(rc):8.3f} .. {max(rc):8.3f})   copies {mc:8.3f} ms ({min(cp):8.3f} .. {max(cp):8.3f})   "
                f"reclaim / copies {mr / mc:5.2f}   ({mb / 1024 / (mr / 1e3):.0f} GiB/s moved)")
        ok(hip.hipFree(a)), ok(hip.hipFree(b))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
