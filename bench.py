#!/usr/bin/env python
"""bench.py — ESKF iterations/s of the HIP IESKF update path on MI355X.

Workload (BASELINE.json configs[3], the largest single-GPU configuration): a batch
of 1024 independent seeded synthetic 16x1800 VLP-16 scan pairs per GPU, exactly 10
IESKF iterations each (fixed_iters throughput mode), inputs resident in HBM before
the timed region — the scans and the search index of their target clouds, which
lins_batch_upload builds as the reference builds its kd-trees in updatePointCloud
(SE:1156-1160), outside performIESKF; `search_index` reports that kernel's time and
the rate with it added to every step.  One "step" = one pass of the hot path over the batch
(lins_batch_run: update kernel + Joseph covariance kernel) + for N>1 the RCCL
all-gather of the fixed-size pose records (lins_pose_allgather, C ABI).  The steps of
the timed region are enqueued back to back (the library's pipelined staged mode: the
gather of step k travels on its own stream beside the kernels of step k + 1) and
waited for ONCE, inside the timed region.  N GPUs: one process per GPU,
each with its own 1024 scans (weak scaling).

Prints ONE JSON line (rank 0).  `roofline` is measured live with HIP events on the
context's stream.  A plain run sets up, warms up, times the steps, writes the outputs
(--dump-outputs) and prints the line; everything else is measured with --full only:
the live PMC counter passes and the device-copy ceiling of `roofline`, the exchange
step alone (N > 1), `cpu_baseline`, `parity_checked` and the extra blocks.
`cpu_baseline` times the REFERENCE'S OWN CODE (kind "reference":
oracle/_ref = StateEstimator.hpp compiled verbatim against stand-in third-party
headers, built where /root/reference exists and shipped with the snapshot) on a
bounded sample of the same scans on this box's cores — or the oracle (kind "port")
when that library did not travel; `parity_checked` compares the GPU results of the
timed batch with that sample.

--dump-outputs DIR writes what the last timed step computed, as the caller of
lins_batch_run receives it (ctx.download(): per scan state, covariance, norms, flags),
to DIR/<name>.npy in float64.  The inputs are seeded: the same arguments give the same
inputs in every run, so two builds can be compared output for output.
"""
import argparse
import importlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PKG = "lins---lidar-inertial-slam_amd"

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec


def traffic_from_profiles(search, live=True):
    """HBM-side bytes per launch of the dominant kernel from the PMC counters.  PMC collection needs rocprofv3 around
    the process, so it happens in a separate run of this same command (tools/pmc_traffic.py on the GPU box, which
    also calibrates FETCH_SIZE / WRITE_SIZE on a streaming copy of known size) and is read back from the newest
    profiles/rNN_pmc_traffic.json — but only when that record was taken from exactly these sources (content digest
    of csrc/ + include/, the stamp build() uses): a record of another build is reported as stale, not as a number.
    -> (traffic dict | None, note)"""
    import glob
    import shutil

    import __graft_entry__ as g

    keep = ("bytes_lo", "bytes_hi", "fetch_size_bytes", "write_size_bytes", "calibration", "kernel", "meaning", "valu")
    # Measured in THIS run when rocprofv3 is on the box: the same command under --pmc FETCH_SIZE /
    # WRITE_SIZE (+ one SQ pass), each in its own rocprofv3 pass with --kernel-trace only, ~10 s per pass
    # (tools/pmc_traffic.py measure()).  LINS_BENCH_NO_LIVE_PMC=1 — set for the runs under the counters themselves —
    # or any failure falls back to the committed record below, and traffic_source says which it was.
    if live and shutil.which("rocprofv3") and os.environ.get("LINS_BENCH_NO_LIVE_PMC") != "1":
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import pmc_traffic

            t0 = time.perf_counter()
            rec = pmc_traffic.measure("live", ["--search", search])
            if rec.get("kernel") and rec.get("bytes_hi"):
                return {k: rec[k] for k in keep if k in rec}, "live: rocprofv3 --pmc passes of this bench run (%.0f s)" % (time.perf_counter() - t0)
        except Exception as e:  # noqa: BLE001  (a profiler that is missing a counter must not fail the bench)
            print("bench: live PMC measurement failed (%s), using the committed record" % e, file=sys.stderr)
        finally:
            os.environ.pop("LINS_BENCH_NO_LIVE_PMC", None)

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))
    if not files:
        return None, "no PMC record"
    try:
        rec = json.load(open(files[-1]))
    except (OSError, ValueError):
        return None, "unreadable PMC record"
    if rec.get("search") not in (search, "auto" if search == "mr" else search):
        return None, f"PMC record is for search={rec.get('search')}"
    if rec.get("source_digest") != g._source_digest():
        return None, "stale: PMC record taken from other sources (" + os.path.basename(files[-1]) + ")"
    return {k: rec[k] for k in keep if k in rec}, os.path.basename(files[-1])


def reference_stop_rule_rate(pkg, ieskf, pairs, args, max_targets):
    """The same scans under the reference's own loop control (SE:475, 575-578: NUM_ITER = 30, stop at |dx| <= 1e-2):
    what the path delivers when it is used as performIESKF is — scans/s, and the iterations they really needed."""
    import numpy as np

    prm = pkg.default_params(num_iter=30, fixed_iters=0)
    with ieskf.IeskfContext(prm, max_batch=len(pairs), max_targets=max(max_targets, 1024), search=args.search) as c:
        c.upload(pairs)
        for _ in range(2):
            c.run()
            c.sync()
        t0 = time.perf_counter()
        n = 10
        for _ in range(n):
            c.run()
            c.sync()
        dt = (time.perf_counter() - t0) / n
        # ... and queued back to back with one wait, as the headline's steps are (the context's two launch queues)
        for _ in range(3):  # (untimed: the first queued runs)
            c.run()
        c.sync()
        t0 = time.perf_counter()
        for _ in range(2 * n):
            c.run()
        c.sync()
        dtq = (time.perf_counter() - t0) / (2 * n)
        its = c.total_iters()
        res = c.download()
    return {"scans_per_s": len(pairs) / dt, "iterations_per_s": its / dt, "ms_per_step": dt * 1e3,
            "ms_per_step_queued": dtq * 1e3, "scans_per_s_queued": len(pairs) / dtq,
            "note": "ms_per_step: a host wait after every step (one launch with several-part updates); ms_per_step_queued: 20 steps back to back, one wait",
            "mean_iterations_per_scan": its / len(pairs), "converged": int(sum(r.converged for r in res)),
            "diverged": int(sum(r.diverged for r in res)), "num_iter": 30, "stop_rule": "|dx| <= 1e-2 (SE:575-578)"}


def two_batches_in_flight(pkg, ieskf, pairs, args, max_targets):
    """The same batch and step from TWO contexts (two streams) whose launches overlap: the slots one launch leaves idle
    at its end are taken by the other's workgroups — what a server with two batches in flight sees, by the wall clock.
    Not the headline: `value` times one context, where every launch has a duration of its own."""
    prm = pkg.default_params(num_iter=args.iters, fixed_iters=1)
    ctxs = [ieskf.IeskfContext(prm, max_batch=len(pairs), max_targets=max(max_targets, 1024), search=args.search) for _ in range(2)]
    try:
        for c in ctxs:
            c.set_launch_queues(1)  # (the one-launch form in both: since round 6 ONE context overlaps its queued runs by itself — the headline)
            c.upload(pairs)
            c.run()
            c.sync()
        n = 2 * max(args.steps, 10)
        t0 = time.perf_counter()
        for k in range(n):
            ctxs[k & 1].run()
        for c in ctxs:
            c.sync()
        dt = (time.perf_counter() - t0) / n
    finally:
        for c in ctxs:
            c.close()
    return {"iterations_per_s": len(pairs) * args.iters / dt, "ms_per_launch": dt * 1e3,
            "note": "two contexts in the one-launch form (lins_set_launch_queues 1), launches alternated, one wait at the end; wall clock"}


def scene_b_block(pkg, ieskf, host, args, workers):
    """The second scene family (csrc/host/synth.cpp "open": open ground, ~60 trunks, far wall segments, 30 % of the returns
    lost, a moving box): the same step on a batch of it — rate, kernel time, fraction of the HBM roofline on ITS algorithmic
    bytes, the kernel family `auto` chose, how many selections the certificates decided without a search, and a sample of
    the batch against the CPU oracle.  VERDICT r04: everything before round 5 ran one scene family."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(workers) as ex:
        pairs = list(ex.map(lambda i: host.synth_pair(i, scene=1), range(50000, 50000 + args.batch)))
    sizes = np.array([p.sizes() for p in pairs], dtype=np.float64)
    alg = float(sum(p.bytes_per_iter() for p in pairs)) * args.iters
    prm = pkg.default_params(num_iter=args.iters, fixed_iters=1)
    with ieskf.IeskfContext(prm, max_batch=len(pairs), max_targets=16384, search=args.search) as c:
        c.upload(pairs)
        for _ in range(3):
            c.run()
        c.sync()
        n = max(args.steps, 10)
        t0 = time.perf_counter()
        for _ in range(n):
            c.run()
        c.sync()
        dt = (time.perf_counter() - t0) / n
        k_ms = c.runs_span_ms(min(n, 64)) / min(n, 64)  # (device time per step over the timed steps: their launches overlap, see roofline.launches)
        lm = c.launch_ms_history(min(n, 64))
        res = c.download()
        search = c.last_search()
    out = {"workload": f"{len(pairs)} scan pairs of the open scene family x {args.iters} fixed iterations",
           "mean_sizes": {"n_sharp": float(sizes[:, 0].mean()), "n_flat": float(sizes[:, 1].mean()),
                          "n_less_sharp_last": float(sizes[:, 2].mean()), "n_less_flat_last": float(sizes[:, 3].mean())},
           "iterations_per_s": len(pairs) * args.iters / dt, "ms_per_step": dt * 1e3, "kernel_ms": k_ms, "lins_last_search": search,
           "launches_per_step": float(np.mean([1 + (b > 0) for _, b in lm])), "mean_launch_ms": float(np.mean([t for ab in lm for t in ab if t > 0])),
           "roofline": {"bound": "hbm", "achieved": alg / (k_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": alg / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "alg_bytes_per_launch": alg},
           # per query and search iteration: selections decided between the two tracked candidates, no search / no walk
           "certified": {"nn_per_scan": float(np.mean([r.reserved[1] for r in res])), "walks_per_scan": float(np.mean([r.reserved[2] for r in res])),
                         "queries_per_scan": float((sizes[:, 0] + sizes[:, 1]).mean()),
                         "note": "counted by the production kernel over the 10 iterations of an update (the cold iteration certifies nothing)"},
           "diverged_scans": int(sum(r.diverged for r in res))}
    if not args.no_cpu:
        from oracle import oracle

        k = min(64, len(pairs))
        with ThreadPoolExecutor(workers) as ex:
            want = list(ex.map(lambda p: oracle.ieskf(prm, p, oracle.FORM_REDUCED, oracle.NN_KDTREE), pairs[:k]))
        ok = all((g.iters, g.diverged, g.m_surf, g.m_corner) == (w.iters, w.diverged, w.m_surf, w.m_corner) for g, w in zip(res, want))
        dp = max(float(np.abs(g.state[:3] - w.state[:3]).max()) for g, w in zip(res, want))
        dc = max(float(np.abs(g.cov - w.cov).max() / np.abs(w.cov).max()) for g, w in zip(res, want))
        out["parity_checked"] = {"scans": k, "ok": bool(ok and dp <= 1e-6 and dc <= 1e-9), "max_dp_m": dp, "max_rel_dP": dc, "against": "oracle (reduced form, kd-tree)"}
    return out


def rotating_inputs_block(pkg, ieskf, host, pairs, args, workers, max_targets):
    """The timed step re-runs ONE resident batch (147 MB of clouds against a 256 MB Infinity Cache): a deployment streams new
    scans.  Four different batches resident in HBM in four contexts, run in turn (a host wait after every launch, kernel
    time by HIP events), against the same pattern on one batch: 4 x 147 MB walk through the cache between two launches
    on the same clouds, so every launch reads its clouds from HBM."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor

    prm = pkg.default_params(num_iter=args.iters, fixed_iters=1)
    n = len(pairs)
    with ThreadPoolExecutor(workers) as ex:
        more = list(ex.map(host.synth_pair, range(60000, 60000 + 3 * n)))
    batches = [pairs, more[:n], more[n:2 * n], more[2 * n:]]
    ctxs = [ieskf.IeskfContext(prm, max_batch=n, max_targets=max(max_targets, 16384), search=args.search) for _ in batches]
    try:
        for c, b in zip(ctxs, batches):
            c.upload(b)
            c.run()
            c.sync()
        rot, same = [], []
        for _ in range(6):
            for c in ctxs:
                c.run()
                c.sync()
                rot.append(c.last_kernel_ms())
        for _ in range(24):
            ctxs[0].run()
            ctxs[0].sync()
            same.append(ctxs[0].last_kernel_ms())
    finally:
        for c in ctxs:
            c.close()
    r, s0 = float(np.mean(rot[4:])), float(np.mean(same[4:]))
    return {"batches": len(batches), "scans_per_batch": n, "bytes_of_clouds_per_batch": int(sum(16 * sum(p.sizes()) for p in pairs)),
            "kernel_ms_rotating": r, "kernel_ms_one_batch": s0, "ratio": r / s0,
            "note": "kernel time by HIP events, one launch at a time; rotating: four different batches in turn (other scans, so the mean "
                    "differs by the batches' own work as well: ratio of the first batch's launches alone below)",
            "kernel_ms_first_batch_when_rotating": float(np.mean(rot[4::4])),
            "ratio_first_batch": float(np.mean(rot[4::4])) / s0}


def single_scan_latency(pkg, ieskf, pair):
    """BASELINE.json configs[2]: ONE scan pair, full on-device loop (the live lins_fusion_node case): kernel time
    of the single-scan kernel and the end-to-end latency of lins_ieskf_update (upload + kernels + download)."""
    import numpy as np

    prm = pkg.default_params(num_iter=30, fixed_iters=0)
    with ieskf.IeskfContext(prm, max_batch=1, max_targets=16384, search="auto") as c:
        c.upload([pair])
        ks, e2e = [], []
        for k in range(25):
            c.run()
            c.sync()
            if k >= 5:
                ks.append(c.last_kernel_ms())
        its = c.total_iters()
        for k in range(25):
            t0 = time.perf_counter()
            c.update(pair)
            if k >= 5:
                e2e.append((time.perf_counter() - t0) * 1e3)
    k_ms = float(np.median(ks))
    alg = float(pair.bytes_per_iter()) * int(its)  # B_iter of this pair x the iterations it ran
    return {"kernel": "lds_full::ieskf_lds_kernel<1024,3>", "kernel_ms": k_ms, "iterations": int(its),
            "us_per_iteration": k_ms * 1e3 / max(int(its), 1), "update_call_ms_incl_pcie": float(np.median(e2e)),
            "stop_rule": "|dx| <= 1e-2 (SE:575-578), NUM_ITER 30",
            # BASELINE.json configs[2]: "rocprof HBM GB/s" of the single-scan kernel — one workgroup on one CU of 256: a
            # latency figure, the fraction says how far ONE scan is from streaming its clouds at the whole device's rate
            "roofline": {"bound": "hbm", "achieved": alg / (k_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": alg / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "alg_bytes_per_launch": alg,
                         "note": "one scan = one workgroup = one of 256 CUs; kernel_ms by HIP events (profiles/: the kernel's row in the with-extras trace)"}}


def cpu_leg(pkg, args, prm, pairs, gpu_results):
    """cpu_baseline + parity_checked.  The sample (first --cpu-sample scan pairs of the timed batch) goes through the
    REFERENCE'S OWN CODE when oracle/_ref/liblins_ref.so travelled with the snapshot (kind "reference": performIESKF of
    StateEstimator.hpp compiled verbatim, dense M x M gain, kd-tree; it has no fixed-iteration mode, so it runs its own
    stop rule, NUM_ITER 30, and the rate counts the iterations it really executed) and through the oracle (same
    algorithm restated; also the fixed-iteration form the GPU batch ran, which is what parity_checked compares)."""
    import numpy as np
    from oracle import oracle, ref

    out = {}
    sample = pairs[: min(args.cpu_sample, len(pairs))]
    ncpu = os.cpu_count() or 1
    sec1, it1 = oracle.bench(prm, sample, oracle.FORM_DENSE, oracle.NN_KDTREE, threads=1)
    secn, itn = oracle.bench(prm, sample, oracle.FORM_DENSE, oracle.NN_KDTREE, threads=ncpu)
    secr, itr = oracle.bench(prm, sample, oracle.FORM_REDUCED, oracle.NN_KDTREE, threads=1)
    secrn, itrn = oracle.bench(prm, sample, oracle.FORM_REDUCED, oracle.NN_KDTREE, threads=ncpu)
    port = {"value": it1 / sec1, "unit": "iterations/s", "cores": 1, "kind": "port",
            "sample": f"first {len(sample)} scan pairs of the same batch x {args.iters} iterations (fixed), oracle dense MxM form + "
                      "kd-tree (the reference's cost model), g++ -O3 no FMA",
            "all_cores": {"value": itn / secn, "cores": ncpu},
            "reduced_6x6_form_1core": {"value": itr / secr, "cores": 1},
            "reduced_all_cores": {"value": itrn / secrn, "cores": ncpu}}
    if os.environ.get("LINS_REQUIRE_REF") == "1" and not ref.available():
        raise SystemExit("bench.py: LINS_REQUIRE_REF=1 and oracle/_ref/liblins_ref.so is not here (it is built where /root/reference "
                         "exists and travels with the snapshot): refusing to fall back to cpu_baseline kind \"port\"")
    if ref.available():
        stop = pkg.default_params(num_iter=30, fixed_iters=0)
        rs1, ri1 = ref.bench(stop, sample, threads=1)
        rsn, rin = ref.bench(stop, sample, threads=ncpu)
        out["cpu_baseline"] = {
            "value": ri1 / rs1, "unit": "iterations/s", "cores": 1, "kind": "reference",
            "sample": f"first {len(sample)} scan pairs of the same batch through the reference's own performIESKF "
                      "(the reference's TEXT — StateEstimator.hpp compiled verbatim — on stand-in Eigen / PCL headers: plain loops, "
                      "no vectorised Eigen kernels, so the real library would be somewhat faster; g++ -O3 no FMA, exact "
                      f"kd-tree): its own stop rule, NUM_ITER 30, {ri1} iterations executed.  `port` (the restated oracle, reduced "
                      "6 x 6 algebra, all cores) is the stronger CPU figure to compare against",
            "all_cores": {"value": rin / rsn, "cores": ncpu},
            "port": port}
    else:
        out["cpu_baseline"] = port
    # parity of the timed batch's results (fixed iterations) against the oracle's dense form on the same sample
    with ThreadPoolExecutor(max_workers=min(64, ncpu)) as ex:
        want = list(ex.map(lambda p: oracle.ieskf(prm, p, oracle.FORM_DENSE, oracle.NN_KDTREE), sample))
    got = gpu_results[: len(sample)]
    flags = all((g.iters, g.converged, g.diverged, g.m_surf, g.m_corner) == (w.iters, w.converged, w.diverged, w.m_surf, w.m_corner)
                for g, w in zip(got, want))
    dp = max(float(np.abs(g.state[:3] - w.state[:3]).max()) for g, w in zip(got, want))
    dq = max(float(np.abs(g.state[6:10] - w.state[6:10]).max()) for g, w in zip(got, want))
    dc = max(float(np.abs(g.cov - w.cov).max() / np.abs(w.cov).max()) for g, w in zip(got, want))
    ok = flags and dp <= 1e-6 and dq <= 1e-7 and dc <= 1e-9
    out["parity_checked"] = {"scans": len(sample), "against": "oracle dense M x M form + kd-tree, same fixed iteration count",
                             "flags_equal": bool(flags), "max_dp": dp, "max_dq": dq, "max_rel_dP": dc,
                             "tolerances": {"dp": 1e-6, "dq": 1e-7, "rel_dP": 1e-9}, "ok": bool(ok)}
    return out


def e2e_rates(pkg, ieskf, host, pairs, args):
    """What the C ABI delivers when the inputs are NOT resident: lins_ieskf_update_batch with host buffers in and out
    (validation + packing + H2D + kernels + D2H, pipelined in chunks of 256 scans) and the device-resident streams
    chain (lins_streams_step: front-end -> update -> re-projection, clouds staying in HBM between scans) as the C call
    sees it.  PCIe-bound; never the headline value."""
    import numpy as np

    prm = pkg.default_params(num_iter=args.iters, fixed_iters=1)
    n = len(pairs)
    out = {}
    import ctypes as C

    defs = importlib.import_module(PKG + "._ctypes_defs")
    L = ieskf.lib()
    with ieskf.IeskfContext(prm, max_batch=n, max_targets=16384, search=args.search) as c:
        arr = defs.pairs_to_c(pairs)  # (the C arrays are built once: the times below are the C call's, not Python's marshalling)
        res = (defs.ResultC * n)()
        ts = []
        for k in range(7):
            t0 = time.perf_counter()
            assert L.lins_ieskf_update_batch(c._h, n, arr, res) == 0
            ts.append(time.perf_counter() - t0)
        dt = float(np.median(ts[2:]))
        out["update_batch_it_s"] = sum(r.iters for r in res) / dt
        out["update_batch_ms"] = dt * 1e3
        # the same call with the clouds as pcl::PointXYZI arrays (point_stride_bytes 32: no repacking loop in the caller, the
        # library gathers the payload while it stages) and with the clouds written into the library's pinned staging arena
        # in the first place (lins_batch_map: no staging copy at all)
        arr32, keep = defs.pairs_strided(pairs)
        arrm = c.map_batch(pairs)
        for key, a in (("update_batch_ms_pcl_stride32", arr32), ("update_batch_ms_mapped_staging", arrm)):
            ts = []
            for k in range(6):
                t0 = time.perf_counter()
                assert L.lins_ieskf_update_batch(c._h, n, a, res) == 0
                ts.append(time.perf_counter() - t0)
            out[key] = float(np.median(ts[2:])) * 1e3
        del keep
    # as many streams as the batch has scans (1024: the device's workgroup slots are filled as in the headline), built
    # from 256 distinct scan pairs dealt round-robin — the host-side segmentation of a scan costs more than its GPU time
    ns, nd = n, min(n, 256)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        seg0 = list(ex.map(lambda i: host.frontend_segment(host.synth_raw_scan(i, 0)), range(nd)))
        seg1 = list(ex.map(lambda i: host.frontend_segment(host.synth_raw_scan(i, 1)), range(nd)))
    seg0, seg1 = [seg0[i % nd] for i in range(ns)], [seg1[i % nd] for i in range(ns)]
    boot = np.zeros((ns, 19))
    for i in range(ns):
        boot[i, 0:3], boot[i, 6:10] = pairs[i % nd].meta["true_t"], pairs[i % nd].meta["true_q"]
    st = np.ascontiguousarray(np.stack([pairs[i % nd].state for i in range(ns)]))
    cv = np.ascontiguousarray(np.stack([pairs[i % nd].cov.reshape(324) for i in range(ns)]))
    dp = C.POINTER(C.c_double)
    with ieskf.IeskfContext(prm, max_batch=ns, max_targets=16384) as c:
        L.lins_streams_step.argtypes = [C.c_void_p, C.POINTER(host.SegmentedScanC), dp, dp, C.c_double, C.POINTER(defs.ResultC),
                                        C.POINTER(C.c_int32)]
        a0 = (host.SegmentedScanC * ns)(*[s.c for s in seg0])
        a1 = (host.SegmentedScanC * ns)(*[s.c for s in seg1])
        res = (defs.ResultC * ns)()
        counts = np.zeros((ns, 4), np.int32)
        c.streams_init(ns)
        c.streams_step(seg0, boot, np.tile(np.eye(18)[None] * 1e-4, (ns, 1, 1)))
        ts = []
        for rep in range(5):
            t0 = time.perf_counter()
            assert L.lins_streams_step(c._h, a1 if rep % 2 == 0 else a0, st.ctypes.data_as(dp), cv.ctypes.data_as(dp), 0.1, res,
                                       counts.ctypes.data_as(C.POINTER(C.c_int32))) == 0
            ts.append(time.perf_counter() - t0)
        fe, up, rp = c.streams_stats()
        out["streams_scans_s"] = ns / float(np.min(ts[1:]))
        out["streams_scans_s_on_device"] = ns / ((fe + up + rp) * 1e-3)
        out["streams"] = ns
        # the device-resident chain stage by stage (HIP events of the last step): what a pipeline that keeps the clouds in
        # HBM runs per scan — feature front-end (SE:619-827), IESKF update + search index, re-projection (SE:1083-1161)
        out["chain"] = {"streams": ns, "distinct_scans": nd, "frontend_ms": fe, "update_ms": up, "reprojection_ms": rp, "device_ms": fe + up + rp,
                        "scans_per_s_on_device": ns / ((fe + up + rp) * 1e-3),
                        "ms_per_1024_streams": {"frontend": fe * 1024 / ns, "update": up * 1024 / ns, "reprojection": rp * 1024 / ns},
                        "longest_stage": max((fe, "frontend"), (up, "update"), (rp, "reprojection"))[1]}
    out["note"] = "the C calls as a C++ caller sees them: host buffers in and out (update_batch) / segmented clouds uploaded per scan (streams): PCIe-bound"
    return out


def ensure_built(g):
    """g.build() only when the libraries on disk were not built from these sources (the content digest build() stamps):
    a tree that is already built, perhaps by another user, is benchmarked as it is, without write access to it."""
    try:
        with open(g.STAMP) as f:
            current = all(os.path.exists(p) for p in g.LIBS) and f.read().strip() == g._source_digest()
    except OSError:
        current = False
    if not current:
        g.build()


def dump_outputs(out_dir, res):
    """The per-scan results of the last timed step (rank 0's shard), one float64 array per field, scan-major."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    arrays = {"state": np.stack([r.state for r in res]), "cov": np.stack([r.cov for r in res])}
    for f in ("residual_norm", "update_norm", "iters", "converged", "diverged", "m_surf", "m_corner"):
        arrays[f] = np.array([getattr(r, f) for r in res], dtype=np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def self_launch(args):
    """`python bench.py --gpus N` with no launcher around it: re-exec under torch.distributed.run, one rank per
    GPU on this node (the driver's own N > 1 command line does the same from outside and is honoured as is)."""
    import socket
    import subprocess

    if not args.dry_run:
        import torch

        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} needs {args.gpus} GPUs on this node, found {have}")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


def dry_run(args, rank, world):
    """No GPU, no kernels: the launcher + the benchmarked exchange step (dist.PoseGatherPipeline) over gloo with
    synthetic pose records.  Test aid for the N > 1 plumbing (tests/test_dist.py); prints a line marked dry_run."""
    import numpy as np
    import torch
    import torch.distributed as dist

    dist_mod = importlib.import_module(PKG + ".dist")
    defs = importlib.import_module(PKG + "._ctypes_defs")
    if world > 1:
        dist.init_process_group(backend="gloo")
    n_total = args.batch * world
    pipe = dist_mod.PoseGatherPipeline(n_total, rank, world, device="cpu")
    for k in range(args.warmup + args.steps):
        b, buf = pipe.begin_step()
        rec = np.zeros(pipe.hi - pipe.lo, dtype=defs.POSE_DTYPE)
        rec["scan_id"] = np.arange(pipe.lo, pipe.hi)
        rec["iters"] = args.iters
        rec["m_surf"] = k  # the step a record belongs to
        buf[: rec.nbytes] = torch.from_numpy(rec.view(np.uint8).copy())
        pipe.gather_newest()
        pipe.end_step(b)
    pipe.drain()
    rec = pipe.records()
    assert int(rec["iters"].sum()) == n_total * args.iters, "pose gather incomplete"
    assert (rec["m_surf"] == args.warmup + args.steps - 1).all(), "pose gather returned a stale step"
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "records": int(len(rec)), "ordered": True}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024, help="scans per GPU")
    ap.add_argument("--iters", type=int, default=10, help="IESKF iterations per scan")
    ap.add_argument("--search", default=os.environ.get("LINS_SEARCH", "auto"))
    ap.add_argument("--cpu-sample", type=int, default=192, help="scans timed on the CPU oracle (0 = skip)")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip cpu_baseline and parity_checked")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the reference-stop-rule, single-scan and other extra blocks")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: live PMC passes, copy ceiling, gather alone, CPU leg, extra blocks")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's results to DIR/<name>.npy")
    ap.add_argument("--dry-run", action="store_true", help="launcher + pose gather only, gloo, no GPU (test aid)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)  # does not return
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if args.dry_run:
        return dry_run(args, rank, world)

    import numpy as np
    import torch

    import __graft_entry__ as g

    ensure_built(g)
    pkg = importlib.import_module(PKG)
    host = importlib.import_module(PKG + ".host")
    ieskf = importlib.import_module(PKG + ".ieskf")
    dist_mod = importlib.import_module(PKG + ".dist")

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU fallback for the HIP path)")
    if torch.cuda.device_count() <= local_rank:
        raise SystemExit(f"bench.py: rank {rank} wants GPU {local_rank}, this node has {torch.cuda.device_count()}")
    torch.cuda.set_device(local_rank)
    use_dist = world > 1 or os.environ.get("LINS_FORCE_DIST") == "1"  # (force: exercise the RCCL path on 1 GPU)
    if use_dist:
        import torch.distributed as dist

        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))

    # ---- workload: this rank's contiguous shard of the global batch --------------------
    lo, hi = dist_mod.shard_range(args.batch * world, rank, world)
    t0 = time.time()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        pairs = list(ex.map(host.synth_pair, range(lo, hi)))
    gen_s = time.time() - t0
    sizes = np.array([p.sizes() for p in pairs])
    max_targets = int(sizes[:, 2:].max())

    prm = pkg.default_params(num_iter=args.iters, fixed_iters=1)
    ctx = ieskf.IeskfContext(prm, device=local_rank, max_batch=len(pairs), max_targets=max(max_targets, 1024),
                             search=args.search)
    ctx.upload(pairs)  # inputs resident in HBM, search index of the target clouds built (below: index_ms)
    try:
        index_ms = ctx.last_index_ms()
    except Exception:
        index_ms = None  # (a batch that cannot take the grid kernels: the any-size kernel bins for itself)
    # The exchange step: one flat all-gather of the 192-byte pose records through the C ABI
    # (lins_pose_allgather -> ncclAllGather on the context's communication stream).  torch.distributed only carries the
    # RCCL unique id to the ranks and the two scalars of the timing reduction; shards are padded to the largest
    # (dist.shard_range: sizes differ by at most one) and the padding is cut out on the host (dist.ordered_records).
    spans = [dist_mod.shard_range(args.batch * world, r, world) for r in range(world)]
    max_n = max(b - a for a, b in spans)
    rec_bytes = dist_mod.RECORD_BYTES
    poses = [torch.zeros(max(max_n, 1) * rec_bytes, dtype=torch.uint8, device="cuda") for _ in range(2)]
    gathered = [torch.zeros(world * max(max_n, 1) * rec_bytes, dtype=torch.uint8, device="cuda") for _ in range(2)] if use_dist else None
    c_abi_gather = use_dist
    if use_dist:
        ok = 1
        try:
            uid = [ctx.rccl_unique_id() if rank == 0 else None]
        except Exception as e:  # (rank 0 could not load RCCL through the library: every rank takes the fallback)
            uid, ok = [None], 0
            print(f"bench.py: lins_rccl_unique_id failed ({e}); pose gather falls back to torch.distributed", file=sys.stderr)
        dist.broadcast_object_list(uid, src=0)
        if uid[0] is None:
            ok = 0
        else:
            try:
                ctx.rccl_init(uid[0], rank, world)
            except Exception as e:
                ok = 0
                print(f"bench.py: lins_rccl_init failed on rank {rank} ({e}); pose gather falls back to torch.distributed", file=sys.stderr)
        flag = torch.tensor([ok], dtype=torch.int32, device="cuda")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)  # one rank without a communicator: nobody uses it
        c_abi_gather = bool(flag.item())
        if not c_abi_gather and ok:
            ctx.rccl_destroy()
    ctx.set_pipelined(c_abi_gather)  # (the gather's second stream and events: only where there is a gather)
    n_steps = [0]

    def step():  # everything asynchronous: no host wait inside a step
        b = n_steps[0] & 1
        n_steps[0] += 1
        ctx.run(poses[b].data_ptr(), lo)
        if c_abi_gather:
            ctx.pose_allgather(poses[b].data_ptr(), max_n, gathered[b].data_ptr())
        elif use_dist:  # fallback only (see above): the records leave through torch.distributed, one host wait per step
            ctx.sync()
            dist.all_gather_into_tensor(gathered[b], poses[b])

    def barrier():
        ctx.sync()  # update kernels, Joseph kernels and gathers of every step enqueued so far (one host wait)
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    kernel_ms = ctx.kernel_ms_history(min(args.steps, 64))  # HIP events of the timed steps, each step's first launch start to its last launch end
    # Runs queued back to back go out on the context's two launch queues (include/lins_ieskf.h lins_set_launch_queues): their
    # launches OVERLAP — the slots one launch leaves idle at its end are taken by the other queue's workgroups — so what the
    # timed steps took on the device is the span of all of them, not the sum of per-launch durations.
    span_ms = ctx.runs_span_ms(min(args.steps, 64))
    launches = ctx.launch_ms_history(min(args.steps, 64))
    res = ctx.download() if rank == 0 else None  # what the last timed step computed (before anything else runs on the context)
    if res is not None and args.dump_outputs:
        dump_outputs(args.dump_outputs, res)
    # N > 1: what a scaling curve needs to explain itself — every rank's own kernel time and step time, and (--full) the
    # cost of the exchange step alone (the same flat all-gather, back to back with one wait, outside the timed region)
    per_rank = None
    if use_dist:
        gather_us = None
        if c_abi_gather and args.full:
            reps = 20
            ctx.sync()
            tg = time.perf_counter()
            for k in range(reps):
                ctx.pose_allgather(poses[k & 1].data_ptr(), max_n, gathered[k & 1].data_ptr())
            ctx.sync()
            gather_us = (time.perf_counter() - tg) / reps * 1e6
        mine = torch.tensor([float(np.mean(kernel_ms)), elapsed / args.steps * 1e3, gather_us if gather_us is not None else -1.0],
                            dtype=torch.float64, device="cuda")
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = {"kernel_ms": [float(t[0]) for t in allr], "ms_per_step": [float(t[1]) for t in allr],
                    "gather_us": [float(t[2]) if float(t[2]) >= 0 else None for t in allr],
                    "note": "kernel_ms: HIP events of the update kernel on each rank's stream (mean of the timed steps); gather_us: the "
                            "all-gather of the pose records alone, 20 back to back, one wait"}

    # device-copy ceiling of this box (--full): a streaming float4 copy inside the context's arenas,
    # measured after the timed region (it overwrites the uploaded clouds)
    copy_gbs = None
    if rank == 0 and args.full:
        import ctypes as C

        L = ieskf.lib()
        L.lins_debug_stream_copy.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_double)]
        g_ = C.c_double(0)
        if L.lins_debug_stream_copy(ctx._h, 1 << 30, 5, C.byref(g_)) == 0:
            copy_gbs = g_.value

    iters_local = ctx.total_iters()
    bytes_iter_local = ctx.bytes_per_iter()  # sum over scans of B_iter
    stats = torch.tensor([elapsed, float(iters_local)], dtype=torch.float64, device="cuda")
    if use_dist:
        tmax = stats[:1].clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        isum = stats[1:].clone()
        dist.all_reduce(isum, op=dist.ReduceOp.SUM)
        elapsed_max, iters_all = float(tmax.item()), float(isum.item())
    else:
        elapsed_max, iters_all = elapsed, float(iters_local)

    if use_dist:  # the gathered pose records must be complete and in scan order (outside the timed region)
        last = (n_steps[0] - 1) & 1
        rec = dist_mod.ordered_records(gathered[last].cpu().numpy(), spans)  # (raises when out of order)
        assert int(rec["iters"].sum()) == int(iters_all), "pose gather incomplete"
        if c_abi_gather:
            ctx.rccl_destroy()

    if rank == 0:
        n_div = sum(1 for r in res if r.diverged)
        value = iters_all * args.steps / elapsed_max
        k_ms = span_ms / min(args.steps, 64)  # device time per step over the timed region (launches of successive steps overlap)
        # algorithmic bytes per launch = sum_scans B_iter(scan) * iterations(scan); with the
        # fixed-iteration mode every non-diverged scan runs args.iters iterations
        alg_bytes = bytes_iter_local / len(pairs) * iters_local
        # live counter passes: --full single-GPU runs only (they are runs of their own); otherwise the committed record
        traffic = traffic_from_profiles(args.search, live=(world == 1 and args.full))
        achieved = alg_bytes / (k_ms * 1e-3) / 1e9
        out = {
            "metric": "ESKF iterations/sec (16x1800 VLP-16, ~2k feat)",
            "value": value,
            "unit": "iterations/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed_max / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64 state / f32 points",
            "data": "synthetic",
            "config": {
                "workload": f"configs[3]: batch of {args.batch} independent scan pairs per GPU, "
                            f"{args.iters} IESKF iterations each (fixed), 2 scans resident per CU; a step queued behind another runs as two launches of "
                            "<= 512 scans on the context's two streams, a step issued into an idle context as one launch whose updates hand "
                            "over between workgroups every four iterations; "
                            "inputs resident in HBM before the timed region (PCIe-inclusive rates: see e2e), the target clouds' search "
                            "index built with them (see search_index)",
                "scans_per_gpu": len(pairs),
                "iters_per_scan": args.iters,
                "search": args.search,
                "mean_sizes": {"n_sharp": float(sizes[:, 0].mean()), "n_flat": float(sizes[:, 1].mean()),
                               "n_less_sharp_last": float(sizes[:, 2].mean()),
                               "n_less_flat_last": float(sizes[:, 3].mean())},
                "data_note": "round-3 scan generator (no firing on a range-image column edge: VERDICT r02 item 10): 8.7 k target points per "
                             "scan, 144 KB algorithmic per iteration; rounds 1-2 timed 7.7 k / 127.5 KB scans — iterations/s of different "
                             "rounds compare through roofline.frac (bytes per launch follow the scans), and DESIGN.md section 5.1 has the "
                             "round-2 kernel on these scans (11.9 M it/s)",
                "diverged_scans": n_div,
                "parallelism": f"scan-sharded x{world}" + ((", RCCL all-gather of 192 B pose records through the C ABI (lins_pose_allgather)" if c_abi_gather
                                                           else ", RCCL all-gather of 192 B pose records through torch.distributed (fallback)") if use_dist else ""),
                "gen_seconds": round(gen_s, 2),
            },
            "per_rank": per_rank,
            "roofline": {
                "bound": "hbm",
                "kernel": {"auto": "lds_mr::ieskf_lds_kernel<512,1>" if len(pairs) > 256 else "lds_full::ieskf_lds_kernel<1024,3>",
                           "mr": "lds_mr::ieskf_lds_kernel<512,1>", "lds": "lds_full::ieskf_lds_kernel<1024,3>",
                           "lds1": "lds_full::ieskf_lds_kernel<384,1>"}.get(args.search, "ieskf_persistent_kernel"),
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                "traffic": traffic[0]["bytes_hi"] if traffic[0] else None,  # per step (the counter runs take a step as ONE launch); fabric-side upper bound, see traffic_detail
                "traffic_detail": {k: v for k, v in traffic[0].items() if k != "valu"} if traffic[0] else None,
                # VALU side ("report both the HBM fraction and the VALU fraction"): SQ counters of the
                # same PMC record — busy_frac of the 1024 SIMDs' issue cycles, active lanes per VALU instruction (of 64)
                "valu": ({k: traffic[0]["valu"].get(k) for k in ("busy_frac", "lanes_per_inst", "insts_valu_per_launch", "wave_wait_frac", "lds_conflict_per_active",
                                                                    "insts_lds_per_launch", "insts_salu_per_launch")}
                         if traffic[0] and traffic[0].get("valu") else None),
                "traffic_source": traffic[1],
                "copy_ceiling_GBs": copy_gbs,  # measured stream-copy rate (read + write) on this box
                "frac_of_copy_ceiling": (achieved / copy_gbs) if copy_gbs else None,
                "alg_bytes_per_step": alg_bytes,
                "alg_bytes_per_launch": alg_bytes,  # (per step; kept under the name the earlier rounds' records use: see launches for the bytes of one launch)
                "kernel_ms": k_ms,
                "kernel_ms_meaning": "device time of the timed steps (HIP events: first launch's start to last launch's end, both launch queues) / steps",
                # the launches behind it: a step issued into a busy context is two launches of <= 512 scans (whole updates) on the
                # context's two streams; their own durations (events of each queue; = what rocprofv3 --kernel-trace lists per launch)
                # include the time a launch's workgroups wait for slots the other launch holds, so bytes / launch duration is
                # NOT the device's rate — the span above is
                "launches": {"per_step": float(np.mean([1 + (b > 0) for _, b in launches])),
                             "mean_launch_ms": float(np.mean([t for ab in launches for t in ab if t > 0])),
                             "step_bracket_ms_mean": float(np.mean(kernel_ms)),
                             "alg_bytes_per_launch_mean": alg_bytes / float(np.mean([1 + (b > 0) for _, b in launches])),
                             "note": "two launch queues when runs are queued (lins_set_launch_queues 2, the default): the first timed step finds the context idle and is ONE launch with several-part updates"},
                "bytes_per_iter_mean": bytes_iter_local / len(pairs),
            },
        }
        # Where the search index is built.  The reference builds its kd-trees where it produces the target clouds
        # (setInputCloud in updatePointCloud, SE:1156-1160), not in performIESKF (SE:465-600), and the cpu_baseline below
        # times performIESKF on estimators whose kd-trees exist (oracle/ref_driver.cpp: "Rigs ... built outside the timed
        # region").  The device path has the same split since the end of round 3: grid_index_kernel at lins_batch_upload,
        # the timed step = lins_batch_run = the iterated update.  with_build_each_step adds the build's own kernel time to
        # every step: the rate of a pipeline that searches each index once (and what rounds 1-3 timed, the build then
        # being the update kernel's first phase).
        if index_ms is not None:
            step_ms = elapsed_max / args.steps * 1e3
            out["search_index"] = {
                "built_at": "lins_batch_upload (outside the timed region): the reference's kd-tree build is in updatePointCloud "
                            "(SE:1156-1160), outside performIESKF, and outside the timed region of cpu_baseline kind \"reference\" too "
                            "(oracle/ref_driver.cpp ref_bench builds the estimators' kd-trees first; the port's figures include its own tree build)",
                "kernel": "grid_index_kernel", "kernel_ms": index_ms,
                "with_build_each_step": {"ms_per_step": step_ms + index_ms, "value": iters_all / ((step_ms + index_ms) * 1e-3),
                                         "frac": alg_bytes / ((k_ms + index_ms) * 1e-3) / 1e9 / HBM_PEAK_GBS}}
        if args.full and not args.no_cpu and args.cpu_sample > 0 and world == 1:  # (the CPU leg: single-GPU runs only)
            out.update(cpu_leg(pkg, args, prm, pairs, res))
        if args.full and world == 1 and not args.no_extras:
            out["reference_stop_rule"] = reference_stop_rule_rate(pkg, ieskf, pairs, args, max_targets)
            out["single_scan"] = single_scan_latency(pkg, ieskf, pairs[0])
            out["two_batches_in_flight"] = two_batches_in_flight(pkg, ieskf, pairs, args, max_targets)
            out["e2e"] = e2e_rates(pkg, ieskf, host, pairs, args)
            workers = min(16, os.cpu_count() or 1)
            out["scene_b"] = scene_b_block(pkg, ieskf, host, args, workers)
            out["rotating_inputs"] = rotating_inputs_block(pkg, ieskf, host, pairs, args, workers, max_targets)
    else:
        out = None
    ctx.close()
    if use_dist:
        # every rank drains its C stdout (RCCL's banner) before rank 0 prints the result line
        import ctypes

        ctypes.CDLL(None).fflush(None)
        sys.stdout.flush()
        dist.barrier()
        dist.destroy_process_group()
    if out is not None and out.get("parity_checked") and not out["parity_checked"]["ok"]:
        print(json.dumps(out), flush=True)
        raise SystemExit("bench.py: the GPU results of the timed batch do not match the CPU checker (parity_checked)")
    if use_dist and world > 1 and not c_abi_gather:
        # A run whose exchange step fell back to torch.distributed (a host wait per step) is not a scaling point of THIS
        # path: the line is printed for diagnosis, the exit code says so.
        if out is not None:
            print(json.dumps(out), flush=True)
        raise SystemExit(3)
    if out is not None:
        # RCCL writes its version banner to the C stdout buffer, which would otherwise be flushed at exit — after a
        # line printed from Python.  Drain it first: the JSON line is the last thing on stdout.
        import ctypes

        ctypes.CDLL(None).fflush(None)
        sys.stdout.flush()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
