"""The streams' device-resident filter (include/lins_streams_filter.h lins_streams_filter_*, lins_streams_step_imu*;
csrc/filter_kernels.hip): IMU propagation against the reference's StatePredictor, the finish kernel against its CPU
restatement, the reference's whole state machine over a raw scan sequence with no host filter call in the loop, batch
independence, the feature gate (SE:436-440) and the old and new entry points mixed on one context."""
import ctypes as C
import os

import numpy as np
import pytest

import filter_common as fc
import seq_common

pytestmark = pytest.mark.gpu

SEQS = (11, 12, 13)
N_BOOT = 9  # scans of each sequence the shared reference runs cover (test 3 runs sequence 11 further on its own)


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
def seqs(pkg, host, ref, ref_seq):
    """per sequence: raw clouds, IMU rows and the reference's records of the first N_BOOT scans (computed once)"""
    prm = pkg.default_params(num_iter=30)
    out = {}
    for s in SEQS:
        raws = [host.synth_seq_raw_scan(s, k) for k in range(N_BOOT)]
        imus = [host.synth_seq_imu(s, k) for k in range(N_BOOT)]
        inputs = [(0.1 * (k + 1), imus[k][0], imus[k][1], ref.segment(raws[k])) for k in range(N_BOOT)]
        out[s] = dict(raws=raws, rows=[fc.imu_rows(a, g) for a, g in imus], recs=seq_common.run(ref_seq, prm, inputs))
    return out


def boot(ctx, host, streams):
    """streams: [(sequence dict, scan index b >= 1)] — each stream starts where the reference stands after its scan b:
    scan b through the old entry point (its first scan: clouds re-projected with the reference's relative pose), the
    reference's filter and globalState_ through lins_streams_filter_set."""
    n = len(streams)
    ctx.streams_init(n)
    ctx.streams_step_raw([s["raws"][b] for s, b in streams], np.stack([np.array(s["recs"][b].lin_state[:]) for s, b in streams]),
                         np.tile(np.eye(18)[None] * 1e-4, (n, 1, 1)))
    for k, (s, b) in enumerate(streams):
        ctx.streams_filter_set(k, fc.filter_from_record(host, s["recs"][b]), s["recs"][b].global_state[:])


def flags(r):
    return (r.iters, r.converged, r.diverged, r.m_surf, r.m_corner)


def result_bits(r):
    return (r.state.tobytes(), r.cov.tobytes(), flags(r), r.reserved[0], r.residual_norm, r.update_norm)


# ---- 1 ------------------------------------------------------------------------------------------------------------
def test_predict_kernel_against_the_references_state_predictor(pkg, host, ieskf, defs, ref):
    """8 streams seeded as tests/test_ref.py's StatePredictor test (vn, ba, bw, noisy IMU; one with non-zero init_pos_std /
    init_att_std), 0, 1, 2, 7, 39, 40, 41 and LINS_STREAMS_IMU_MAX rows in ONE call, against filter::StatePredictor
    itself: state 1e-12, covariance 1e-12 max|P|; the host mirror's distance to the kernel is
    printed beside it.  No rows: bitwise unchanged.  13 + 27 rows in two calls: the bits of the 40-row call."""
    cap = defs.STREAMS_IMU_MAX
    counts = [0, 1, 2, 7, 39, 40, 41, cap]
    rng = np.random.default_rng(5)
    filts, seeds, rows = [], [], []
    for k, m in enumerate(counts):
        vn, ba, bw = rng.normal(size=3) * 3, rng.normal(size=3) * 0.05, rng.normal(size=3) * 0.003
        f, fp = fc.new_filter(host, vn, ba, bw, pos_std=[0.02, 0.03, 0.01] if k == 3 else None, att_std=[0.5, 0.4, 0.3] if k == 3 else None)
        filts.append(f), seeds.append((fp, vn, ba, bw))
        rows.append(fc.imu_rows(rng.normal(size=(m, 3)) * 0.3 + [0, 0, 9.81], rng.normal(size=(m, 3)) * 0.05, dt=0.0025))
    g0 = np.zeros(19)
    g0[6] = 1.0
    worst = dict(ref_state=0.0, ref_cov=0.0, host_state=0.0, host_cov=0.0)
    with ieskf.IeskfContext(pkg.default_params(num_iter=30), max_batch=8, max_targets=16384) as ctx:
        ctx.streams_init(8)
        for k in range(8):
            ctx.streams_filter_set(k, filts[k], g0)
        ctx.streams_filter_predict(rows)
        got = [ctx.streams_filter_get(k)[0] for k in range(8)]
        assert fc.filters_bitwise_equal(got[0], filts[0]) and got[0].has_imu == 0
        for k, m in enumerate(counts):
            if m == 0:
                continue
            fp, vn, ba, bw = seeds[k]
            st, cov = ref.filter_run(fp, vn, ba, bw, rows[k])
            h = fc.copy_filter(host, filts[k])
            fc.host_predict(host, h, rows[k])
            gs, gc = np.array(got[k].state[:]), np.array(got[k].cov[:]).reshape(18, 18)
            d = dict(ref_state=np.abs(gs - st).max(), ref_cov=np.abs(gc - cov).max() / np.abs(cov).max(),
                     host_state=np.abs(gs - np.array(h.state[:])).max(),
                     host_cov=np.abs(gc - np.array(h.cov[:]).reshape(18, 18)).max() / np.abs(cov).max())
            print(f"predict, {m} rows: kernel - reference state {d['ref_state']:.2e} cov {d['ref_cov']:.2e} (of max|P|); "
                  f"kernel - host mirror state {d['host_state']:.2e} cov {d['host_cov']:.2e}")
            for key in worst:
                worst[key] = max(worst[key], float(d[key]))
            assert d["ref_state"] <= 1e-12 and d["ref_cov"] <= 1e-12, (m, d)
            assert got[k].has_imu == 1 and np.array_equal(np.array(got[k].acc_last[:]), rows[k][-1, 1:4]) and \
                np.array_equal(np.array(got[k].gyr_last[:]), rows[k][-1, 4:7])
            assert abs(got[k].time - 0.0025 * m) <= 1e-15 * m
        print("predict, worst:", {k: f"{v:.2e}" for k, v in worst.items()})
        # the 40-row stream again, as 13 + 27 rows (the other streams get none)
        ctx.streams_filter_set(5, filts[5], g0)
        none = np.zeros((0, 7))
        ctx.streams_filter_predict([rows[5][:13] if k == 5 else none for k in range(8)])
        ctx.streams_filter_predict([rows[5][13:] if k == 5 else none for k in range(8)])
        assert fc.filters_bitwise_equal(ctx.streams_filter_get(5)[0], got[5])
        assert fc.filters_bitwise_equal(ctx.streams_filter_get(6)[0], got[6])
        pm, _ = ctx.streams_filter_stats()
        assert pm > 0.0


# ---- 2 ------------------------------------------------------------------------------------------------------------
def test_finish_kernel_against_its_cpu_restatement(pkg, host, ieskf, seqs):
    """Four streams on scan 2 of sequence 11, against the resident scan 1: (0) the reference's filter, 40 IMU rows —
    gravity z < 0; (1) no IMU rows and a filter whose gravity points UP (the other sign of SE:603-604; without rows the
    gravity only reaches the update's prior); (2) no IMU rows and a NaN position variance — the first iteration produces NaN, the update
    is flagged diverged (SE:552-563) and the ICP fallback's pose is handed over with the PRIOR covariance, whose position
    block reset(1) then replaces; (3) as (0) with non-zero init_pos_std /
    init_att_std.  Per stream lins_filter_finish on the predicted filter (read back from a twin context that only
    predicts) and the returned posterior must give the device's filter and globalState_: reset(1)'s zeros and identity
    quaternion exact, everything else within 1e-14 of the array's scale (the unshared arithmetic is ocml's asin / atan2
    / sin / cos against libm's)."""
    s = seqs[11]
    prm = pkg.default_params(num_iter=30)
    rows, none = s["rows"][2], np.zeros((0, 7))
    imu = [rows, none, none, rows]

    def load(ctx):
        boot(ctx, host, [(s, 1)] * 4)
        f1, g1 = ctx.streams_filter_get(1)
        f1.state[16:19] = [0.3, -0.2, 9.8]
        ctx.streams_filter_set(1, f1, g1)
        f2, g2 = ctx.streams_filter_get(2)
        f2.cov[0] = float("nan")
        ctx.streams_filter_set(2, f2, g2)
        f3, g3 = ctx.streams_filter_get(3)
        f3.prm.init_pos_std[:] = [0.02, 0.03, 0.01]
        f3.prm.init_att_std[:] = [0.5, 0.4, 0.3]
        ctx.streams_filter_set(3, f3, g3)

    with ieskf.IeskfContext(prm, max_batch=4, max_targets=16 * 1800) as twin:
        load(twin)
        twin.streams_filter_predict(imu)
        pred = [twin.streams_filter_get(k) for k in range(4)]
    with ieskf.IeskfContext(prm, max_batch=4, max_targets=16 * 1800) as ctx:
        load(ctx)
        res, _, gs = ctx.streams_step_imu_raw([s["raws"][2]] * 4, imu)
        got = [ctx.streams_filter_get(k) for k in range(4)]
        _, fm = ctx.streams_filter_stats()
        assert fm > 0.0
    print("finish: diverged flags", [r.diverged for r in res], "iters", [r.iters for r in res])
    assert not res[0].diverged and not res[1].diverged and not res[3].diverged
    assert res[2].diverged and res[2].reserved[0] == 0  # the branch this test is about: ICP pose + prior covariance
    assert np.array_equal(res[2].cov.reshape(324), np.array(pred[2][0].cov[:]), equal_nan=True)
    worst = 0.0
    for k in range(4):
        f, g = pred[k]
        gw = host.filter_finish(f, g, res[k].state, res[k].cov, used_prior_cov=bool(res[k].diverged))
        gf, gg = got[k]
        assert np.array_equal(gg, gs[k])
        st = np.array(gf.state[:])
        assert np.array_equal(st[0:3], np.zeros(3)) and np.array_equal(st[6:10], [1.0, 0.0, 0.0, 0.0]), k
        cw, cg = np.array(f.cov[:]), np.array(gf.cov[:])
        assert np.array_equal(cg[cw == 0.0], np.zeros(int((cw == 0.0).sum()))), k
        for a, b in ((st, np.array(f.state[:])), (cg, cw), (gg, gw)):
            d = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
            worst = max(worst, d)
            assert d <= 1e-14, (k, d)
        assert np.array_equal(np.array(gf.acc_last[:]), np.array(f.acc_last[:])) and gf.time == f.time
    print(f"finish kernel - lins_filter_finish, largest relative difference {worst:.2e}")


# ---- 3 ------------------------------------------------------------------------------------------------------------
def test_twenty_raw_scans_with_the_filter_on_the_device_against_the_references_state_machine(pkg, host, ieskf, ref, ref_seq):
    """Bootstrap as tests/test_gpu_sequence.py; from scan 2 on ONLY lins_streams_step_imu_raw with the scan's 40 IMU rows —
    no host filter call in the loop.  Bars: the existing device-chain test's (linState_ 1e-5 m / 1e-6 rad, filter state
    1e-5), seq_common.compare's for globalState_, DESIGN.md section 3's for a covariance that may end at NUM_ITER
    (1e-6 max|P|)."""
    seq, n_scans = 11, 20
    prm = pkg.default_params(num_iter=30)
    raws = [host.synth_seq_raw_scan(seq, k) for k in range(n_scans)]
    imus = [host.synth_seq_imu(seq, k) for k in range(n_scans)]
    inputs = [(0.1 * (k + 1), imus[k][0], imus[k][1], ref.segment(raws[k])) for k in range(n_scans)]
    want = seq_common.run(ref_seq, prm, inputs)
    s = dict(raws=raws, recs=want)
    worst = dict(lin_p=0.0, lin_a=0.0, filt=0.0, cov=0.0, g_p=0.0, g_a=0.0, g_rest=0.0)
    with ieskf.IeskfContext(prm, max_batch=1, max_targets=16 * 1800) as ctx:
        boot(ctx, host, [(s, 1)])
        for k in range(2, n_scans):
            res, counts, g = ctx.streams_step_imu_raw([raws[k]], [fc.imu_rows(*imus[k])])
            r, w = res[0], want[k]
            assert w.ran_update and r.reserved[0] == 0, k
            assert flags(r) == (w.iters, w.converged, w.diverged, w.m_surf, w.m_corner), k
            assert tuple(counts[0]) == (w.n_corner_sharp, w.n_corner_less_sharp, w.n_surf_flat, w.n_surf_less_flat), k
            lw, gw = np.array(w.lin_state[:]), np.array(w.global_state[:])
            f, g1 = ctx.streams_filter_get(0)
            assert np.array_equal(g1, g[0])
            pw = np.array(w.filter_cov[:])
            d = dict(lin_p=np.abs(r.state[:3] - lw[:3]).max(), lin_a=seq_common.quat_angle(r.state[6:10], lw[6:10]),
                     filt=np.abs(np.array(f.state[:]) - np.array(w.filter_state[:])).max(),
                     cov=np.abs(np.array(f.cov[:]) - pw).max() / np.abs(pw).max(),
                     g_p=np.abs(g1[:3] - gw[:3]).max(), g_a=seq_common.quat_angle(g1[6:10], gw[6:10]),
                     g_rest=max(np.abs(g1[3:6] - gw[3:6]).max(), np.abs(g1[10:] - gw[10:]).max()))
            for key in worst:
                worst[key] = max(worst[key], float(d[key]))
            assert d["lin_p"] <= 1e-5 and d["lin_a"] <= 1e-6 and d["filt"] <= 1e-5, (k, d)
            assert d["g_p"] <= 1e-5 and d["g_a"] <= 1e-6 and d["g_rest"] <= 1e-4, (k, d)
            assert d["cov"] <= 1e-6, (k, d)
            assert np.array_equal(np.array(list(f.acc_last[:]) + list(f.gyr_last[:])), np.array(w.imu_last[:])), k
    print("device filter, 18 scans, largest differences to the reference:", {k: f"{v:.2e}" for k, v in worst.items()})


# ---- 4 ------------------------------------------------------------------------------------------------------------
def _stream_plan(seqs, i):
    """stream i: sequence, first scan, and how many of each scan's 40 IMU rows arrive BEFORE the step (through
    lins_streams_filter_predict) — the step itself then takes 40 - early rows: the counts differ between streams"""
    return seqs[SEQS[i % 3]], 1 + (i // 3) % 4, 3 * (i % 7)


def _run_plan(ctx, host, plans, n_steps=4):
    boot(ctx, host, [(s, b) for s, b, _ in plans])
    out = []
    for step in range(1, n_steps + 1):
        ctx.streams_filter_predict([s["rows"][b + step][:e] for s, b, e in plans])
        res, counts, g = ctx.streams_step_imu_raw([s["raws"][b + step] for s, b, _ in plans], [s["rows"][b + step][e:] for s, b, e in plans])
        out.append((res, counts, g))
    return out, [ctx.streams_filter_get(k) for k in range(len(plans))]


def test_a_streams_result_does_not_depend_on_its_batch(pkg, host, ieskf, seqs):
    """70 streams (more than one wave of workgroups, no multiple of 64): sequences 11 - 13 from different scans, different
    IMU row counts per stream.  After 4 steps every stream's results, filter and globalState_ are the bits of the same
    stream run alone in a fresh context."""
    n = 70
    prm = pkg.default_params(num_iter=30)
    plans = [_stream_plan(seqs, i) for i in range(n)]
    with ieskf.IeskfContext(prm, max_batch=n, max_targets=16 * 1800) as ctx:
        steps, filts = _run_plan(ctx, host, plans)
    assert all(r.iters > 0 for res, _, _ in steps for r in res)
    alone = {}
    for i in range(n):
        key = (i % 3, (i // 3) % 4, i % 7)  # (streams with one plan are one stream)
        if key not in alone:
            with ieskf.IeskfContext(prm, max_batch=1, max_targets=16 * 1800) as c1:
                alone[key] = _run_plan(c1, host, [plans[i]])
        s1, f1 = alone[key]
        for (res, counts, g), (res1, counts1, g1) in zip(steps, s1):
            assert result_bits(res[i]) == result_bits(res1[0]), i
            assert np.array_equal(counts[i], counts1[0]) and np.array_equal(g[i], g1[0]), i
        assert fc.filters_bitwise_equal(filts[i][0], f1[0][0]) and np.array_equal(filts[i][1], f1[0][1]), i


# ---- 5 ------------------------------------------------------------------------------------------------------------
def _short_arc(raw):
    """a few rings' short arc of a raw cloud: too few features for processScan (SE:436-440)"""
    raw = np.asarray(raw, np.float32).reshape(-1, 4)
    ring = np.rint((np.degrees(np.arctan2(raw[:, 2], np.hypot(raw[:, 0], raw[:, 1]))) + 15.0) / 2.0)
    az = np.arctan2(raw[:, 1], raw[:, 0])
    keep = (ring >= 6) & (ring <= 8) & (np.abs(az) < 0.08)
    return np.ascontiguousarray(raw[keep])


def test_the_feature_gate_keeps_the_old_targets_and_the_predicted_filter(pkg, host, ieskf, defs, seqs):
    prm = pkg.default_params(num_iter=30)
    plans = [(seqs[s], 1, 0) for s in SEQS]
    bad = _short_arc(seqs[12]["raws"][4])
    fb = host.frontend_extract(bad)
    assert len(bad) >= 2 and (len(fb["corner_less_sharp"]) <= 5 or len(fb["surf_less_flat"]) <= 10)
    for s in (11, 13):
        fg = host.frontend_extract(seqs[s]["raws"][4])
        assert len(fg["corner_less_sharp"]) > 5 and len(fg["surf_less_flat"]) > 10

    def scans(step, with_bad):
        return [bad if (with_bad and step == 3 and k == 1) else s["raws"][1 + step] for k, (s, _, _) in enumerate(plans)]

    def imu(step):
        return [s["rows"][1 + step] for s, _, _ in plans]

    with ieskf.IeskfContext(prm, max_batch=3, max_targets=16 * 1800) as ctx:
        boot(ctx, host, [(s, b) for s, b, _ in plans])
        a = [ctx.streams_step_imu_raw(scans(step, True), imu(step)) for step in (1, 2)]
        f_before, g_before = ctx.streams_filter_get(1)
        old = [ctx.streams_peek(1, w) for w in (0, 1)]
        a.append(ctx.streams_step_imu_raw(scans(3, True), imu(3)))
        r = a[2][0][1]
        assert r.reserved[0] == defs.STREAMS_GATED and r.iters == 0 and not r.diverged
        f_gated, g_gated = ctx.streams_filter_get(1)
        assert np.array_equal(g_gated, g_before) and np.array_equal(a[2][2][1], g_before)
        assert all(np.array_equal(ctx.streams_peek(1, w), old[w]) for w in (0, 1))
        a.append(ctx.streams_step_imu_raw(scans(4, True), imu(4)))
        f_end = [ctx.streams_filter_get(k) for k in range(3)]
    # predict-only twin: the same filter, the same rows, no scan
    with ieskf.IeskfContext(prm, max_batch=1, max_targets=16 * 1800) as twin:
        twin.streams_init(1)
        twin.streams_filter_set(0, f_before, g_before)
        twin.streams_filter_predict([imu(3)[1]])
        f_pred, _ = twin.streams_filter_get(0)
    assert fc.filters_bitwise_equal(f_gated, f_pred)
    assert np.array_equal(r.state, np.array(f_pred.state[:])) and np.array_equal(r.cov.reshape(324), np.array(f_pred.cov[:]))
    # the other streams: as in a run where stream 1's scan was fine
    with ieskf.IeskfContext(prm, max_batch=3, max_targets=16 * 1800) as ctx:
        boot(ctx, host, [(s, b) for s, b, _ in plans])
        b = [ctx.streams_step_imu_raw(scans(step, False), imu(step)) for step in (1, 2, 3, 4)]
        f_good = [ctx.streams_filter_get(k) for k in range(3)]
    for k in (0, 2):
        for (res, counts, g), (res1, counts1, g1) in zip(a, b):
            assert result_bits(res[k]) == result_bits(res1[k]) and np.array_equal(g[k], g1[k]), k
        assert fc.filters_bitwise_equal(f_end[k][0], f_good[k][0]) and np.array_equal(f_end[k][1], f_good[k][1])
    # step 4 of stream 1 matched the OLD targets (scan 3's clouds): flags of the host chain that skips the bad scan
    s = seqs[12]
    with ieskf.IeskfContext(prm, max_batch=1, max_targets=16 * 1800) as hc:
        hc.streams_init(1)
        hc.streams_step_raw([s["raws"][1]], np.array(s["recs"][1].lin_state[:])[None], np.eye(18)[None] * 1e-4)
        f, g = fc.filter_from_record(host, s["recs"][1]), np.array(s["recs"][1].global_state[:])
        for step in (1, 2, 3, 4):
            fc.host_predict(host, f, s["rows"][1 + step])
            if step == 3:
                continue
            res, _ = hc.streams_step_raw([s["raws"][1 + step]], np.array(f.state[:])[None], np.array(f.cov[:]).reshape(1, 18, 18))
            g = host.filter_finish(f, g, res[0].state, res[0].cov, used_prior_cov=bool(res[0].diverged))
    got = a[3][0][1]
    assert got.iters > 0 and flags(got) == flags(res[0])
    assert np.abs(got.state - res[0].state).max() <= 1e-9


# ---- 6 ------------------------------------------------------------------------------------------------------------
def test_old_and_new_entry_points_mixed_on_one_context(pkg, host, ieskf, seqs):
    """IMU step, then the same scan step done by hand — lins_streams_filter_predict, priors from lins_streams_filter_get,
    lins_streams_step_raw, lins_filter_finish on the host, lins_streams_filter_set — then an IMU step again, against three
    IMU steps.  The update of the middle step reads the same bits either way; what may differ is the host finish against
    the device's (test 2's bar, 1e-14) and what the last step makes of it (test 1's bar, 1e-12)."""
    s = seqs[11]
    prm = pkg.default_params(num_iter=30)
    with ieskf.IeskfContext(prm, max_batch=1, max_targets=16 * 1800) as ctx:
        boot(ctx, host, [(s, 1)])
        a = [ctx.streams_step_imu_raw([s["raws"][k]], [s["rows"][k]]) for k in (2, 3, 4)]
        fa, ga = ctx.streams_filter_get(0)
    with ieskf.IeskfContext(prm, max_batch=1, max_targets=16 * 1800) as ctx:
        boot(ctx, host, [(s, 1)])
        b0 = ctx.streams_step_imu_raw([s["raws"][2]], [s["rows"][2]])
        ctx.streams_filter_predict([s["rows"][3]])
        f, g = ctx.streams_filter_get(0)
        res, counts = ctx.streams_step_raw([s["raws"][3]], np.array(f.state[:])[None], np.array(f.cov[:]).reshape(1, 18, 18))
        f_same, g_same = ctx.streams_filter_get(0)  # the old entry point left the device filter alone
        assert fc.filters_bitwise_equal(f_same, f) and np.array_equal(g_same, g)
        g = host.filter_finish(f, g, res[0].state, res[0].cov, used_prior_cov=bool(res[0].diverged))
        ctx.streams_filter_set(0, f, g)
        b2 = ctx.streams_step_imu_raw([s["raws"][4]], [s["rows"][4]])
        fb, gb = ctx.streams_filter_get(0)
    assert result_bits(a[0][0][0]) == result_bits(b0[0][0]) and np.array_equal(a[0][2], b0[2])
    assert result_bits(a[1][0][0]) == result_bits(res[0]) and np.array_equal(a[1][1], counts)
    assert np.abs(g - a[1][2][0]).max() <= 1e-14 * np.abs(g).max()
    assert flags(a[2][0][0]) == flags(b2[0][0])
    assert np.abs(a[2][0][0].state - b2[0][0].state).max() <= 1e-12
    assert np.abs(a[2][0][0].cov - b2[0][0].cov).max() <= 1e-12 * np.abs(b2[0][0].cov).max()
    assert np.abs(np.array(fa.state[:]) - np.array(fb.state[:])).max() <= 1e-12
    assert np.abs(np.array(fa.cov[:]) - np.array(fb.cov[:])).max() <= 1e-12 * np.abs(np.array(fb.cov[:])).max()
    assert np.abs(ga - gb).max() <= 1e-12 * np.abs(gb).max()


def test_imu_step_needs_a_filter_and_a_resident_scan(pkg, host, ieskf, seqs):
    s = seqs[11]
    with ieskf.IeskfContext(pkg.default_params(num_iter=30), max_batch=1, max_targets=16 * 1800) as ctx:
        ctx.streams_init(1)
        with pytest.raises(ieskf.LinsError):  # no filter
            ctx.streams_step_imu_raw([s["raws"][2]], [s["rows"][2]])
        f = fc.filter_from_record(host, s["recs"][1])
        ctx.streams_filter_set(0, f, s["recs"][1].global_state[:])
        with pytest.raises(ieskf.LinsError):  # no resident last scan
            ctx.streams_step_imu_raw([s["raws"][2]], [s["rows"][2]])
        with pytest.raises(ieskf.LinsError):  # more rows than a call takes
            ctx.streams_filter_predict([np.zeros((65, 7))])
        boot(ctx, host, [(s, 1)])
        res, _, _ = ctx.streams_step_imu_raw([s["raws"][2]], [s["rows"][2]])
        assert res[0].iters > 0
