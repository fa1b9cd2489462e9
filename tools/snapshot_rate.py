#!/usr/bin/env python3
"""What moving a robot costs (include/lins_snapshot.h: lins_streams_snapshot / lins_streams_restore, kernels snap_pack /
snap_unpack of csrc/snapshot_kernels.hip); profiles/snapshot_rate.txt keeps one run.  For a slot of --frames key frames
of --points points whose frames are interleaved with the other slots' (one small frame of another slot behind every
frame, round robin over the other --slots - 1 slots: every frame is a run of its own):
  pack / unpack   device time of the table-driven launches (lins_last_snapshot_stats, HIP events)
  one copy        one device-to-device hipMemcpyAsync of the same bytes — what the bytes alone cost
  per run         one device-to-device hipMemcpyAsync per frame — the alternative the kernels replace
  calls           wall time of the whole lins_streams_snapshot and lins_streams_restore, with the PCIe copy, the table and
                  the blob's sum
Medians of --runs with min .. max.  The restore goes into an empty slot of a second context that holds the same
neighbours; the slot is released again after every run (not timed).

    python tools/snapshot_rate.py [--slots 64] [--frames 50,500,2000] [--points 4600] [--runs 5] [--out profiles/snapshot_rate.txt]
"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

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
    ap.add_argument("--frames", default="50,500,2000")
    ap.add_argument("--points", type=int, default=4600)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_rate.txt"))
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

    ns, small, mine = args.slots, 64, 0
    n_corner, n_outl = args.points // 9, args.points // 3
    n_surf = args.points - n_corner - n_outl
    rng = np.random.default_rng(5)
    clouds = [np.concatenate([rng.uniform(-30, 30, (n, 3)), rng.uniform(0, 16, (n, 1))], 1).astype(np.float32) for n in (n_corner, n_surf, n_outl)]
    frame, _keep = defs.keyframe_c(clouds[0], clouds[1], clouds[2], np.zeros(6, np.float32))
    other, _keep2 = defs.keyframe_c(clouds[0][:small], clouds[1][:0], clouds[2][:0], np.zeros(6, np.float32))

    def med(v):
        return f"{statistics.median(v):9.3f} ({min(v):9.3f} .. {max(v):9.3f})"

    say(f"a slot of F key frames x {args.points} points among {ns} slots, every frame a run of its own; ms, median (min .. max) of {args.runs}")
    for nf in [int(x) for x in args.frames.split(",")]:
        per_other = -(-nf // (ns - 1))
        total = nf * args.points + nf * small
        pts = nf * args.points
        with ieskf.IeskfContext(pkg.default_params(), max_batch=ns, max_targets=1024) as a, \
                ieskf.IeskfContext(pkg.default_params(), max_batch=ns, max_targets=1024) as d:
            for c in (a, d):
                c.streams_init(ns)
            a.archive_init(ns, max(nf, per_other), total)
            d.archive_init(ns, max(nf, per_other), total)
            for i in range(nf):
                assert L.lins_archive_push(a._h, mine, C.byref(frame), 0.1 * i) == i
                s = 1 + i % (ns - 1)
                for c in (a, d):
                    assert L.lins_archive_push(c._h, s, C.byref(other), 0.1 * i) == i // (ns - 1)
            src, dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
            ok(hip.hipMalloc(C.byref(src), total * 16)), ok(hip.hipMalloc(C.byref(dst), pts * 16))
            ok(hip.hipMemset(src, 0, total * 16)), ok(hip.hipMemset(dst, 0, pts * 16))
            ok(hip.hipEventCreate(C.byref(e0))), ok(hip.hipEventCreate(C.byref(e1)))

            def timed(copies):
                ms = C.c_float(0)
                ok(hip.hipEventRecord(e0, None))
                for to, frm, n in copies:
                    ok(hip.hipMemcpyAsync(C.c_void_p(dst.value + to * 16), C.c_void_p(src.value + frm * 16), n * 16, D2D, None))
                ok(hip.hipEventRecord(e1, None))
                ok(hip.hipEventSynchronize(e1))
                ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
                return ms.value

            one = [(0, 0, pts)]
            runs = [(i * args.points, i * (args.points + small), args.points) for i in range(nf)]
            pack, unpack, snap, rest, c1, cn = [], [], [], [], [], []
            for run in range(args.runs + 1):  # (the first round loads code and allocates the staging buffers: not kept)
                t0 = time.perf_counter()
                (blob,) = a.streams_snapshot([mine])
                t1 = time.perf_counter()
                st = a.snapshot_stats()
                assert st["bytes"] == pts * 16 and st["segments"] == nf
                t2 = time.perf_counter()
                d.streams_restore([mine], [blob])
                t3 = time.perf_counter()
                su = d.snapshot_stats()
                assert su["segments"] == 1 and d.archive_count(mine) == nf
                d.archive_release_slots([mine])
                x, y = timed(one), timed(runs)
                if run:
                    pack.append(st["pack_ms"]), unpack.append(su["unpack_ms"]), snap.append((t1 - t0) * 1e3), rest.append((t3 - t2) * 1e3)
                    c1.append(x), cn.append(y)
            say(f"F = {nf}: {pts} points, {pts * 16 / 2 ** 20:.1f} MiB in {nf} runs; blob {len(blob)} bytes")
            say(f"  pack   {med(pack)}   unpack {med(unpack)}   (device, HIP events)")
            say(f"  one device-to-device copy {med(c1)}   one copy per run {med(cn)}")
            say(f"  pack / one copy {statistics.median(pack) / statistics.median(c1):5.2f}   copy per run / pack {statistics.median(cn) / statistics.median(pack):6.1f}")
            say(f"  lins_streams_snapshot {med(snap)}   lins_streams_restore {med(rest)}   (wall, with the PCIe copy and the blob's sum)")
            ok(hip.hipFree(src)), ok(hip.hipFree(dst))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
