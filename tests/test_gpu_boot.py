"""The streams' state machine (include/lins_streams_filter.h: lins_streams_machine_init, lins_streams_process*;
csrc/boot_kernels.hip, csrc/lins_capi_boot.hip): the IMU pre-integration kernel against its CPU restatement, the two-scan
bootstrap against the reference's records, the hand-over to the running filter, the sequence over the join against the
reference, mixed batches with gated scans, and the interface's edges."""
import os

import numpy as np
import pytest

import boot_common as bc
import filter_common as fc
import seq_common

pytestmark = pytest.mark.gpu

SEQS = bc.SEQS
N = bc.N_SCANS
NONE = np.zeros((0, 7))


@pytest.fixture(scope="module")
def ref():
    from oracle import ref as r

    if not r.available():
        if os.environ.get("LINS_REQUIRE_REF") == "1":
            pytest.fail("LINS_REQUIRE_REF=1 and oracle/_ref/liblins_ref.so did not travel with the snapshot")
        pytest.skip("oracle/_ref/liblins_ref.so did not travel and the reference is not here to build it")
    return r


@pytest.fixture(scope="module")
def ref_seq(ref):
    from oracle import ref_seq as r

    if not r.available():
        if os.environ.get("LINS_REQUIRE_REF") == "1":
            pytest.fail("LINS_REQUIRE_REF=1 and oracle/_ref/liblins_ref_seq.so did not travel with the snapshot")
        pytest.skip("oracle/_ref/liblins_ref_seq.so did not travel and the reference is not here to build it")
    r.lib()
    return r


@pytest.fixture(scope="module")
def data(host):
    """raw clouds and IMU rows of the first N sweeps of the three sequences (no reference needed)"""
    return {s: bc.load(host, s) for s in SEQS}


@pytest.fixture(scope="module")
def seqs(pkg, data, ref, ref_seq):
    """... with the reference's records (NUM_ITER = 30), computed once"""
    prm = pkg.default_params(num_iter=30)
    return {s: dict(data[s], recs=bc.records(ref, ref_seq, prm, data[s])) for s in SEQS}


def flags(r):
    return (r.iters, r.converged, r.diverged, r.m_surf, r.m_corner)


def result_bits(r):
    return (r.state.tobytes(), r.cov.tobytes(), flags(r), r.reserved[0], r.residual_norm, r.update_norm)


def context(ieskf, pkg, n):
    return ieskf.IeskfContext(pkg.default_params(num_iter=30), max_batch=n, max_targets=16 * 1800)


def machine(ctx, n):
    ctx.streams_init(n)
    ctx.streams_machine_init()


def step(ctx, streams, k, raws=None):
    """scan k of every stream's sequence through lins_streams_process_raw (raws: replacement clouds per stream or None)"""
    clouds = [s["raws"][k] if raws is None or raws[i] is None else raws[i] for i, s in enumerate(streams)]
    return ctx.streams_process_raw(clouds, [s["rows"][k] for s in streams], [bc.scan_time(k)] * len(streams))


# ---- 1 ------------------------------------------------------------------------------------------------------------
def test_preintegration_kernel_against_its_cpu_restatement(pkg, host, ieskf, defs, data):
    """8 streams in FIRST_SCAN (each with an imu_last_ of its own) take 0, 1, 2, 7, 39, 40, 41 and LINS_STREAMS_IMU_MAX
    rows in ONE call.  Against lins_host_preintegrate BIT FOR BIT: the row step is +, -, x, / and sqrt only, correctly
    rounded on both sides, no contraction.  The 0-row stream keeps its bits; 13 + 27 rows in two calls are the bits of 40;
    the filter's time_ advances by the rows' dt; the rows given to a stream in INIT are dropped (SE:244-245)."""
    cap = defs.STREAMS_IMU_MAX
    counts = [0, 1, 2, 7, 39, 40, 41, cap]
    rng = np.random.default_rng(7)
    raw = data[11]["raws"][0]
    il = rng.normal(size=(8, 6)) * 0.2 + [0, 0, 9.81, 0, 0, 0]
    rows = [fc.imu_rows(rng.normal(size=(m, 3)) * 0.3 + [0, 0, 9.81], rng.normal(size=(m, 3)) * 0.05, dt=0.0025) for m in counts]
    want = []
    for k in range(8):
        _, _, pre = host.boot_first(il[k], 0.1)
        want.append((pre.array(), host.preintegrate(pre, rows[k]).array()))
    with context(ieskf, pkg, 8) as ctx:
        machine(ctx, 8)
        _, _, _, status = ctx.streams_process_raw([raw] * 8, [NONE] * 8, [0.1] * 8, scan_imu=il)
        assert list(status) == [defs.STREAM_FIRST_SCAN] * 8
        for k in range(8):
            assert np.array_equal(ctx.streams_preintegration_get(k).array(), want[k][0]), k
        ctx.streams_filter_predict(rows)
        got = [ctx.streams_preintegration_get(k).array() for k in range(8)]
        for k, m in enumerate(counts):
            d = np.abs(got[k] - want[k][1]).max()
            print(f"pre-integration, {m} rows: kernel - host restatement {d:.2e}, sum_dt {got[k][0]!r}")
            assert np.array_equal(got[k], want[k][1]), (m, d)
            t = 0.1
            for dt in rows[k][:, 0]:
                t += dt
            assert ctx.streams_filter_get(k)[0].time == t, m
        assert np.array_equal(got[0], want[0][0])  # no rows: the record as processFirstScan left it
        pm, _, _ = ctx.streams_boot_stats()
        assert pm > 0.0
        # anew: rows given in INIT are dropped; then the 40-row stream as 13 + 27 rows, the others none
        ctx.streams_machine_init()
        ctx.streams_filter_predict(rows)
        assert list(ctx.streams_status()) == [defs.STREAM_INIT] * 8
        ctx.streams_process_raw([raw] * 8, [NONE] * 8, [0.1] * 8, scan_imu=il)
        for k in range(8):
            assert np.array_equal(ctx.streams_preintegration_get(k).array(), want[k][0]), k
        ctx.streams_filter_predict([rows[5][:13] if k == 5 else NONE for k in range(8)])
        ctx.streams_filter_predict([rows[5][13:] if k == 5 else NONE for k in range(8)])
        assert np.array_equal(ctx.streams_preintegration_get(5).array(), got[5])
        assert np.array_equal(ctx.streams_preintegration_get(6).array(), want[6][0])


# ---- 2 ------------------------------------------------------------------------------------------------------------
def test_bootstrap_against_the_references_records(pkg, host, ieskf, defs, seqs):
    """Sequences 11, 12, 13 as three streams of one context, raw scans 0 and 1.  Bars: the device ICP's existing contract
    ("device ICP kernel = reference": 1e-6 m / 1e-7) for what the ICP's pose reaches — linState_, the
    filter's position; its velocity is that over sum_dt = 0.1: 1e-5 —, 1e-12 for what it does not; against
    lins_host_boot_second fed the device's own ICP pose 1e-12 (ocml against glibc asin / sin / cos is the only admitted
    difference)."""
    streams = [seqs[s] for s in SEQS]
    with context(ieskf, pkg, 3) as ctx:
        machine(ctx, 3)
        seg = ctx.segment_batch([s["raws"][0] for s in streams])
        feats = ctx.extract_features_batch(seg)
        machine(ctx, 3)
        res, counts, _, status = step(ctx, streams, 0)
        assert list(status) == [defs.STREAM_FIRST_SCAN] * 3
        for k, s in enumerate(streams):
            w, r = s["recs"][0], res[k]
            assert w.status == 1 and r.reserved[0] == defs.STREAMS_FIRST and r.iters == 0
            assert tuple(counts[k]) == (w.n_corner_sharp, w.n_corner_less_sharp, w.n_surf_flat, w.n_surf_less_flat)
            # the targets are the front-end's clouds as extracted: updatePointCloud is not called on a first scan
            assert np.array_equal(ctx.streams_peek(k, 0), feats[k]["corner_less_sharp"]), k
            assert np.array_equal(ctx.streams_peek(k, 1), feats[k]["surf_less_flat"]), k
            f, _ = ctx.streams_filter_get(k)
            pw = np.array(w.filter_cov[:])
            assert np.array_equal(np.array(f.state[:]), np.array(w.filter_state[:])) and np.array_equal(r.state, np.array(f.state[:]))
            assert np.abs(np.array(f.cov[:]) - pw).max() <= 1e-12 * np.abs(pw).max() and np.array_equal(r.cov.reshape(324), np.array(f.cov[:]))
            assert np.array_equal(np.array(list(f.acc_last[:]) + list(f.gyr_last[:])), np.array(w.imu_last[:])) and f.time == bc.scan_time(0)
        assert np.array_equal(ctx.streams_lin_state(), np.stack([np.array(s["recs"][0].lin_state[:]) for s in streams]))
        res, counts, g, status = step(ctx, streams, 1)
        assert list(status) == [defs.STREAM_RUNNING] * 3
        lin = ctx.streams_lin_state()
        pm, im, fm = ctx.streams_boot_stats()
        assert pm > 0.0 and im > 0.0 and fm > 0.0
        worst = dict(lin_p=0.0, lin_q=0.0, pos=0.0, vel=0.0, att=0.0, cov=0.0, host=0.0)
        for k, s in enumerate(streams):
            w, r = s["recs"][1], res[k]
            assert w.status == 3 and r.reserved[0] == defs.STREAMS_BOOTED and r.iters > 0 and not r.diverged
            assert tuple(counts[k]) == (w.n_corner_sharp, w.n_corner_less_sharp, w.n_surf_flat, w.n_surf_less_flat)
            f, g1 = ctx.streams_filter_get(k)
            assert np.array_equal(g1, g[k]) and np.array_equal(r.state, np.array(f.state[:]))
            lw, fw, gw, pw = (np.array(x[:]) for x in (w.lin_state, w.filter_state, w.global_state, w.filter_cov))
            fs = np.array(f.state[:])
            d = dict(lin_p=np.abs(lin[k][:3] - lw[:3]).max(), lin_q=np.abs(lin[k][6:10] - lw[6:10]).max(),
                     pos=np.abs(fs[:3] - fw[:3]).max(), vel=np.abs(fs[3:6] - fw[3:6]).max(), att=np.abs(g1[6:10] - gw[6:10]).max(),
                     cov=np.abs(np.array(f.cov[:]) - pw).max() / np.abs(pw).max())
            # the finish kernel alone: lins_host_boot_second on the device's own ICP pose
            b = bc.host_bootstrap(host, s, icp_pose=(lin[k][:3], lin[k][6:10]))
            hf, hg, hl = b["second"]
            d["host"] = max(np.abs(fs - np.array(hf.state[:])).max(), np.abs(g1 - hg).max())
            print(f"bootstrap, sequence {SEQS[k]}: ICP rounds {r.iters}, converged {r.converged};", {key: f"{v:.2e}" for key, v in d.items()})
            for key in worst:
                worst[key] = max(worst[key], float(d[key]))
            assert d["lin_p"] <= 1e-6 and d["lin_q"] <= 1e-7 and d["pos"] <= 1e-6 and d["vel"] <= 1e-5, (k, d)
            assert d["att"] <= 1e-12 and d["cov"] <= 1e-12 and d["host"] <= 1e-12, (k, d)
            assert np.array_equal(g1[10:16], gw[10:16]) and np.array_equal(fs[10:16], fw[10:16])  # ba, bw
            assert np.array_equal(fs[6:10], [1.0, 0.0, 0.0, 0.0]) and np.array_equal(fs[:3], lin[k][:3]) and np.array_equal(lin[k], hl)
            assert np.array_equal(np.array(list(f.acc_last[:]) + list(f.gyr_last[:])), np.array(w.imu_last[:])) and f.time == bc.scan_time(1)
        print("bootstrap, worst:", {key: f"{v:.2e}" for key, v in worst.items()})


# ---- 3 ------------------------------------------------------------------------------------------------------------
def test_hand_over_to_the_running_filter_bit_for_bit(pkg, host, ieskf, data):
    """Context X bootstraps on the device (scans 0, 1) and runs scans 2 - 5 through lins_streams_process_raw.  Context Y
    is started the established way from X's own state after scan 1 — lins_streams_step_raw on scan 1 with X's linState_,
    lins_streams_filter_set with X's filter and globalState_ — and runs scans 2 - 5 through lins_streams_step_imu_raw.
    Everything a scan leaves is the same bits."""
    streams = [data[s] for s in SEQS]
    with context(ieskf, pkg, 3) as X, context(ieskf, pkg, 3) as Y:
        machine(X, 3)
        step(X, streams, 0)
        step(X, streams, 1)
        Y.streams_init(3)
        Y.streams_step_raw([s["raws"][1] for s in streams], X.streams_lin_state(), np.tile(np.eye(18)[None] * 1e-4, (3, 1, 1)))
        for k in range(3):
            Y.streams_filter_set(k, *X.streams_filter_get(k))
            assert all(np.array_equal(X.streams_peek(k, w), Y.streams_peek(k, w)) for w in (0, 1)), k
        for scan in range(2, N):
            rx, cx, gx, status = step(X, streams, scan)
            ry, cy, gy = Y.streams_step_imu_raw([s["raws"][scan] for s in streams], [s["rows"][scan] for s in streams])
            assert list(status) == [3, 3, 3]
            assert np.array_equal(cx, cy) and np.array_equal(gx, gy), scan
            for k in range(3):
                assert rx[k].iters > 0 and result_bits(rx[k]) == result_bits(ry[k]), (scan, k)
                assert all(np.array_equal(X.streams_peek(k, w), Y.streams_peek(k, w)) for w in (0, 1)), (scan, k)
                fx, fy = X.streams_filter_get(k), Y.streams_filter_get(k)
                assert fc.filters_bitwise_equal(fx[0], fy[0]) and np.array_equal(fx[1], fy[1]), (scan, k)


# ---- 4 ------------------------------------------------------------------------------------------------------------
def test_scans_over_the_join_against_the_reference(pkg, host, ieskf, seqs):
    """The same three streams from their first scan on; scans 2 - 5 against the reference's records: flags equal, linState_
    within 1e-5 m / 1e-6 rad and the filter after reset(1) within 1e-5 (the bars of tests/test_gpu_sequence.py)."""
    streams = [seqs[s] for s in SEQS]
    worst = dict(lin_p=0.0, lin_a=0.0, filt=0.0)
    with context(ieskf, pkg, 3) as ctx:
        machine(ctx, 3)
        step(ctx, streams, 0)
        step(ctx, streams, 1)
        for scan in range(2, N):
            res, counts, g, status = step(ctx, streams, scan)
            for k, s in enumerate(streams):
                w, r = s["recs"][scan], res[k]
                assert w.status == 3 and w.ran_update and status[k] == 3 and r.reserved[0] == 0, (scan, k)
                assert flags(r) == (w.iters, w.converged, w.diverged, w.m_surf, w.m_corner), (scan, k)
                assert tuple(counts[k]) == (w.n_corner_sharp, w.n_corner_less_sharp, w.n_surf_flat, w.n_surf_less_flat), (scan, k)
                lw = np.array(w.lin_state[:])
                f, _ = ctx.streams_filter_get(k)
                d = dict(lin_p=np.abs(r.state[:3] - lw[:3]).max(), lin_a=seq_common.quat_angle(r.state[6:10], lw[6:10]),
                         filt=np.abs(np.array(f.state[:]) - np.array(w.filter_state[:])).max())
                for key in worst:
                    worst[key] = max(worst[key], float(d[key]))
                assert d["lin_p"] <= 1e-5 and d["lin_a"] <= 1e-6 and d["filt"] <= 1e-5, (scan, k, d)
    print("over the join, scans 2 - 5, largest differences to the reference:", {k: f"{v:.2e}" for k, v in worst.items()})


# ---- 5 ------------------------------------------------------------------------------------------------------------
def _plans(s):
    """per stream of the mixed batch: the cloud of each of the five calls — (a) undisturbed, (b) scan 0 sparse, (c) scan 1
    sparse, (d) a sparse sweep for its first call: it idles in INIT and starts one call late"""
    sp = [bc.sparse(r) for r in s["raws"][:2]]
    return [s["raws"][:5], [sp[0]] + s["raws"][1:5], [s["raws"][0], sp[1]] + s["raws"][2:5], [sp[0]] + s["raws"][1:5]]


def _peek_or_none(ctx, k):
    """the resident last scan's two clouds, or None while the stream has none"""
    try:
        return ctx.streams_peek(k, 0), ctx.streams_peek(k, 1)
    except Exception:
        return None


def test_mixed_batch_and_gates(pkg, host, ieskf, defs, ref, ref_seq, data):
    """Four streams of sequence 11 in one context, five calls.  Per call the statuses are the reference's for the same
    single-stream sequence; every accepted scan's result, and what the call leaves of the stream, is bit for bit that of
    the same stream run alone in a context of one; a RUNNING stream's result is that of lins_streams_step_imu_raw on a
    twin context."""
    s = data[11]
    plans = _plans(s)
    prm = pkg.default_params(num_iter=30)
    want_status = [[r.status for r in bc.records(ref, ref_seq, prm, s, raws=p)] for p in plans[:3]]
    assert want_status == [[1, 3, 3, 3, 3], [0, 1, 3, 3, 3], [1, 0, 1, 3, 3]]
    want_status.append(want_status[1])

    def run(ctx, which):
        n = len(which)
        machine(ctx, n)
        out = []
        for call in range(5):
            res, counts, g, status = ctx.streams_process_raw([plans[i][call] for i in which], [s["rows"][call]] * n, [bc.scan_time(call)] * n)
            left = [_peek_or_none(ctx, k) for k in range(n)]
            filt = [ctx.streams_filter_get(k) if status[k] != 0 else None for k in range(n)]
            out.append((res, counts, g, status, left, filt))
        return out

    with context(ieskf, pkg, 4) as ctx:
        batch = run(ctx, [0, 1, 2, 3])
    for call in range(5):
        assert [int(v) for v in batch[call][3]] == [want_status[i][call] for i in range(4)], call
    # the codes of the first two calls: accepted first / second scans, gated scans
    D = defs
    assert [r.reserved[0] for r in batch[0][0]] == [D.STREAMS_FIRST, D.STREAMS_GATED, D.STREAMS_FIRST, D.STREAMS_GATED]
    assert [r.reserved[0] for r in batch[1][0]] == [D.STREAMS_BOOTED, D.STREAMS_FIRST, D.STREAMS_GATED, D.STREAMS_FIRST]
    assert [r.reserved[0] for r in batch[2][0]] == [0, D.STREAMS_BOOTED, D.STREAMS_FIRST, D.STREAMS_BOOTED]
    for i in range(3):  # (stream 3 has stream 1's plan)
        with context(ieskf, pkg, 1) as c1:
            alone = run(c1, [i])
        for k in ([i] if i != 1 else [1, 3]):
            for call in range(5):
                (res, counts, g, status, left, filt), (res1, counts1, g1, status1, left1, filt1) = batch[call], alone[call]
                assert result_bits(res[k]) == result_bits(res1[0]), (k, call)
                assert np.array_equal(counts[k], counts1[0]) and status[k] == status1[0], (k, call)
                if status[k] == D.STREAM_RUNNING:
                    assert np.array_equal(g[k], g1[0]), (k, call)
                assert (left[k] is None) == (left1[0] is None) and (filt[k] is None) == (filt1[0] is None), (k, call)
                if left[k] is not None:
                    assert all(np.array_equal(a, b) for a, b in zip(left[k], left1[0])), (k, call)
                if filt[k] is not None:
                    assert fc.filters_bitwise_equal(filt[k][0], filt1[0][0]) and np.array_equal(filt[k][1], filt1[0][1]), (k, call)
    # stream (c) keeps the first scan's clouds while back in INIT (call 1), as the reference's record does
    assert all(np.array_equal(a, b) for a, b in zip(batch[1][4][2], batch[0][4][2]))
    # a RUNNING stream's rows of `out`: lins_streams_step_imu_raw on a twin started from stream (a)'s state after call 1
    with context(ieskf, pkg, 1) as X, context(ieskf, pkg, 1) as Y:
        machine(X, 1)
        for call in (0, 1):
            X.streams_process_raw([s["raws"][call]], [s["rows"][call]], [bc.scan_time(call)])
        Y.streams_init(1)
        Y.streams_step_raw([s["raws"][1]], X.streams_lin_state(), np.eye(18)[None] * 1e-4)
        Y.streams_filter_set(0, *X.streams_filter_get(0))
        for call in (2, 3, 4):
            ry, cy, gy = Y.streams_step_imu_raw([s["raws"][call]], [s["rows"][call]])
            assert result_bits(ry[0]) == result_bits(batch[call][0][0]) and np.array_equal(gy[0], batch[call][2][0]), call


# ---- 6 ------------------------------------------------------------------------------------------------------------
def test_interface_edges(pkg, host, ieskf, defs, data):
    s = data[11]
    raw, rows = s["raws"][0], s["rows"][0]

    def code(fn):
        with pytest.raises(ieskf.LinsError) as e:
            fn()
        return int(str(e.value).split("error ")[1].split(":")[0])

    with context(ieskf, pkg, 1) as ctx:
        ctx.streams_init(1)
        # without lins_streams_machine_init the new calls are call-sequence errors ...
        assert code(lambda: ctx.streams_process_raw([raw], [rows], [0.1])) == defs.E_STATE
        assert code(ctx.streams_status) == defs.E_STATE
        assert code(lambda: ctx.streams_preintegration_get(0)) == defs.E_STATE
        # ... and an existing-path call's bits do not depend on a machine-mode context having lived beside it
        lin = np.zeros((1, 19))
        lin[0, 6], lin[0, 18] = 1.0, -9.81
        before = ctx.streams_step_raw([raw], lin, np.eye(18)[None] * 1e-4)
        with context(ieskf, pkg, 1) as m:
            machine(m, 1)
            m.streams_process_raw([raw], [rows], [0.1])
        ctx.streams_init(1)
        after = ctx.streams_step_raw([raw], lin, np.eye(18)[None] * 1e-4)
        assert result_bits(before[0][0]) == result_bits(after[0][0]) and np.array_equal(before[1], after[1])
    with context(ieskf, pkg, 1) as ctx:
        machine(ctx, 1)
        assert code(lambda: ctx.streams_preintegration_get(0)) == defs.E_STATE  # INIT
        # no imu_last_: scan_imu = NULL and the stream has never been given a row — nothing advanced
        assert code(lambda: ctx.streams_process_raw([raw], [NONE], [0.1])) == -1
        assert list(ctx.streams_status()) == [defs.STREAM_INIT]
        # lins_streams_step_imu_raw still needs every stream RUNNING
        assert code(lambda: ctx.streams_step_imu_raw([raw], [rows])) == defs.E_STATE
        res, _, _, status = ctx.streams_process_raw([raw], [rows], [0.1])
        assert list(status) == [defs.STREAM_FIRST_SCAN] and res[0].reserved[0] == defs.STREAMS_FIRST
        assert code(lambda: ctx.streams_step_imu_raw([s["raws"][1]], [s["rows"][1]])) == defs.E_STATE  # FIRST_SCAN
        pre = ctx.streams_preintegration_get(0)
        assert pre.sum_dt == 0.0 and np.array_equal(np.array(list(pre.acc_0[:]) + list(pre.gyr_0[:])), rows[-1, 1:7])
        # the last row the stream has SEEN serves a later call that brings none
        ctx.streams_filter_predict([s["rows"][1]])
        res, _, _, status = ctx.streams_process_raw([s["raws"][1]], [NONE], [0.2])
        assert list(status) == [defs.STREAM_RUNNING] and res[0].reserved[0] == defs.STREAMS_BOOTED
        f, _ = ctx.streams_filter_get(0)
        assert np.array_equal(np.array(list(f.acc_last[:]) + list(f.gyr_last[:])), s["rows"][1][-1, 1:7])
        assert code(lambda: ctx.streams_preintegration_get(0)) == defs.E_STATE  # RUNNING
        res, _, _ = ctx.streams_step_imu_raw([s["raws"][2]], [s["rows"][2]])  # every stream RUNNING: the old call serves
        assert res[0].iters > 0
