"""Shared by tests/golden/make_streams_step_golden.py (the recipe) and tests/test_gpu_streams_step_golden.py: five
scenarios that between them pass through every mode of the device-resident streams step — prior given by the caller
(segmented scans under each kernel family, raw clouds), prior from the device filter (with a gated scan), the state
machine (INIT, FIRST_SCAN, RUNNING, gated first scans, back to INIT) and the divergence fall-back — and what each call
leaves, as integer arrays (floats by their bits, so that NaN compares like any other value).

Per call and stream: state and covariance, iters / converged / diverged / m_surf / m_corner / reserved[0], residual and
update norm, the four feature counts, the global state and the status where the call returns them, the stream's filter
and globalState_ where it has one, the outlier count of streams_map_cloud(.., 2) and a SHA-256 of each streams_peek
cloud (-1 / zeros while the stream has no resident scan)."""
import hashlib

import numpy as np

import boot_common as bc
import filter_common as fc


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _short_arc(raw):
    """a few rings' short arc of a raw cloud: too few features for processScan (SE:436-440; as tests/test_gpu_filter.py)"""
    raw = np.asarray(raw, np.float32).reshape(-1, 4)
    ring = np.rint((np.degrees(np.arctan2(raw[:, 2], np.hypot(raw[:, 0], raw[:, 1]))) + 15.0) / 2.0)
    az = np.arctan2(raw[:, 1], raw[:, 0])
    return np.ascontiguousarray(raw[(ring >= 6) & (ring <= 8) & (np.abs(az) < 0.08)])


class Recorder:
    def __init__(self, ieskf):
        self.out, self.ieskf = {}, ieskf

    def call(self, key, ctx, n, res, counts, g=None, status=None, filters=()):
        """filters: the streams whose filter is read back"""
        o = self.out
        o[key + "/state"] = np.stack([_bits(r.state).reshape(19) for r in res])
        o[key + "/cov"] = np.stack([_bits(r.cov).reshape(324) for r in res])
        o[key + "/flags"] = np.array([[r.iters, r.converged, r.diverged, r.m_surf, r.m_corner, r.reserved[0]] for r in res], np.int32)
        o[key + "/norms"] = np.stack([_bits([r.residual_norm, r.update_norm]) for r in res])
        o[key + "/counts"] = np.asarray(counts, np.int32).copy()
        if g is not None:
            o[key + "/global"] = _bits(g).reshape(n, 19).copy()
        if status is not None:
            o[key + "/status"] = np.asarray(status, np.int32).copy()
        filt = np.zeros((n, 351 + 19), np.int64)
        for k in filters:
            f, gs = ctx.streams_filter_get(k)
            filt[k] = _bits(np.concatenate(list(fc.filter_arrays(f)) + [gs]))
        if len(filters):
            o[key + "/filter"] = filt
        outl, peek = np.full(n, -1, np.int32), np.zeros((n, 2, 32), np.uint8)
        for k in range(n):
            try:
                clouds = [ctx.streams_peek(k, w) for w in (0, 1)]
            except self.ieskf.LinsError:  # no resident scan yet
                continue
            outl[k] = len(ctx.streams_map_cloud(k, 2))
            for w in (0, 1):
                peek[k, w] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(clouds[w]).tobytes()).digest(), np.uint8)
        o[key + "/outliers"], o[key + "/peek"] = outl, peek


def _given_priors(host, n, start):
    pairs = host.synth_batch(n, start=start)
    boot = np.zeros((n, 19))
    for i, p in enumerate(pairs):
        boot[i, 0:3], boot[i, 6:10] = p.meta["true_t"], p.meta["true_q"]
    return boot, np.stack([p.state for p in pairs]), np.stack([p.cov for p in pairs])


def given_segmented(pkg, host, ieskf):
    """three streams, three steps (first scan, two matched ones: the slots swap back) under each kernel family"""
    n, rec = 3, Recorder(ieskf)
    segs = [[host.frontend_segment(host.synth_raw_scan(40 + i, k)) for i in range(n)] for k in (0, 1)]
    boot, prior, cov = _given_priors(host, n, 40)
    cov0 = np.tile(np.eye(18)[None] * 1e-4, (n, 1, 1))
    for search in ("auto", "lds1", "mr", "binned"):
        with ieskf.IeskfContext(pkg.default_params(num_iter=12), max_batch=n, max_targets=16384, search=search) as c:
            c.streams_init(n)
            for step, (sg, ps, pc) in enumerate(((segs[0], boot, cov0), (segs[1], prior, cov), (segs[0], prior, cov))):
                res, counts = c.streams_step(sg, ps, pc)
                rec.call(f"{search}/{step}", c, n, res, counts)
    return rec.out


def given_raw(pkg, host, ieskf):
    """the same three streams from raw clouds"""
    n, rec = 3, Recorder(ieskf)
    raws = [[host.synth_raw_scan(40 + i, k) for i in range(n)] for k in (0, 1)]
    boot, prior, cov = _given_priors(host, n, 40)
    cov0 = np.tile(np.eye(18)[None] * 1e-4, (n, 1, 1))
    with ieskf.IeskfContext(pkg.default_params(num_iter=12), max_batch=n, max_targets=16384) as c:
        c.streams_init(n)
        for step, (rw, ps, pc) in enumerate(((raws[0], boot, cov0), (raws[1], prior, cov), (raws[0], prior, cov))):
            res, counts = c.streams_step_raw(rw, ps, pc)
            rec.call(f"{step}", c, n, res, counts)
    return rec.out


def _context30(pkg, ieskf, n):
    return ieskf.IeskfContext(pkg.default_params(num_iter=30), max_batch=n, max_targets=16 * 1800)


def device_filter(pkg, host, ieskf):
    """sequence 11: a stream brought to RUNNING by the state machine hands its linState_ and filter to a twin, which
    takes one raw step, the filter, three filter steps, a gated one (a short arc of the next sweep) and that sweep whole"""
    rec, s = Recorder(ieskf), bc.load(host, 11)
    with _context30(pkg, ieskf, 1) as X, _context30(pkg, ieskf, 1) as Y:
        X.streams_init(1)
        X.streams_machine_init()
        for call in (0, 1):
            res, counts, g, status = X.streams_process_raw([s["raws"][call]], [s["rows"][call]], [bc.scan_time(call)])
            rec.call(f"machine/{call}", X, 1, res, counts, g, status, filters=[0] if status[0] != 0 else [])
        Y.streams_init(1)
        res, counts = Y.streams_step_raw([s["raws"][1]], X.streams_lin_state(), np.eye(18)[None] * 1e-4)
        rec.call("twin/first", Y, 1, res, counts)
        Y.streams_filter_set(0, *X.streams_filter_get(0))
        clouds = [s["raws"][2], s["raws"][3], s["raws"][4], _short_arc(s["raws"][5]), s["raws"][5]]
        rows = [s["rows"][2], s["rows"][3], s["rows"][4], s["rows"][5], s["rows"][5]]
        for step, (cl, rw) in enumerate(zip(clouds, rows)):
            res, counts, g = Y.streams_step_imu_raw([cl], [rw])
            rec.call(f"twin/{step}", Y, 1, res, counts, g, filters=[0])
    return rec.out


def state_machine(pkg, host, ieskf):
    """four streams of sequence 11, five calls (the mixed batch of tests/test_gpu_boot.py): undisturbed; scan 0 sparse;
    scan 1 sparse (back to INIT); a sparse sweep for its first call"""
    rec, s, n = Recorder(ieskf), bc.load(host, 11), 4
    sp = [bc.sparse(r) for r in s["raws"][:2]]
    plans = [s["raws"][:5], [sp[0]] + s["raws"][1:5], [s["raws"][0], sp[1]] + s["raws"][2:5], [sp[0]] + s["raws"][1:5]]
    with _context30(pkg, ieskf, n) as c:
        c.streams_init(n)
        c.streams_machine_init()
        for call in range(5):
            res, counts, g, status = c.streams_process_raw([p[call] for p in plans], [s["rows"][call]] * n, [bc.scan_time(call)] * n)
            rec.call(f"{call}", c, n, res, counts, g, status, filters=[k for k in range(n) if status[k] != 0])
    return rec.out


def divergence_fallback(pkg, host, ieskf):
    """ICP_FREQ = 2 and a NaN prior covariance: the diverged stream cannot take the device fall-back, the others step"""
    n, rec = 3, Recorder(ieskf)
    segs = [[host.frontend_segment(host.synth_raw_scan(60 + i, k)) for i in range(n)] for k in (0, 1)]
    boot, prior, cov = _given_priors(host, n, 60)
    bad_cov = cov.copy()
    bad_cov[1] = np.nan
    with ieskf.IeskfContext(pkg.default_params(num_iter=12, icp_freq=2), max_batch=n, max_targets=16384) as c:
        c.streams_init(n)
        for step, (sg, ps, pc) in enumerate(((segs[0], boot, cov), (segs[1], prior, bad_cov), (segs[0], prior, cov))):
            res, counts = c.streams_step(sg, ps, pc)
            rec.call(f"{step}", c, n, res, counts)
    return rec.out


SCENARIOS = dict(given_segmented=given_segmented, given_raw=given_raw, device_filter=device_filter, state_machine=state_machine,
                 divergence_fallback=divergence_fallback)
