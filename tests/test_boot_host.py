"""The CPU restatement of the two-scan bootstrap (lins_host_preintegrate, lins_host_boot_first / _second;
csrc/host/boot.cpp, csrc/boot_math.h) against the reference's own state machine (oracle/ref_seq.py)."""
import os

import numpy as np
import pytest

import boot_common as bc
import filter_common as fc
import seq_common


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
def seqs(host):
    return {s: bc.load(host, s, 2) for s in bc.SEQS}


# ---- 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seq", bc.SEQS)
def test_preintegration_against_the_reference(pkg, host, ref, ref_seq, seqs, seq):
    """With NUM_ITER = 0 estimateTransform's loop runs no round: record 1's linState_ is (pl, ql) of SE:392-396 and the
    filter's velocity pl / sum_dt.  Exactly two scans are fed (a third would run performIESKF with NUM_ITER = 0).  Bar:
    1e-12 absolute, the StatePredictor kernel's (tests/test_gpu_filter.py test 1) — 40 rows of the same arithmetic."""
    s = seqs[seq]
    recs = bc.records(ref, ref_seq, pkg.default_params(num_iter=0), s, n=2)
    assert [r.status for r in recs] == [1, 3]
    b = bc.host_bootstrap(host, s)
    pl, ql = b["start"]
    lw, fw = np.array(recs[1].lin_state[:]), np.array(recs[1].filter_state[:])
    d = dict(pl=np.abs(pl - lw[0:3]).max(), ql=np.abs(ql - lw[6:10]).max(), v=np.abs(pl / b["pre"].sum_dt - fw[3:6]).max())
    print(f"sequence {seq}: pl {pl}, q_w {ql[0]:.10f}, sum_dt {b['pre'].sum_dt!r}; host - reference", {k: f"{v:.2e}" for k, v in d.items()})
    assert np.abs(pl).max() > 1e-6 and ql[0] < 1.0  # (the sequence moves: the comparison is not one of zeros)
    assert d["pl"] <= 1e-12 and d["ql"] <= 1e-12 and d["v"] <= 1e-12, d
    # 13 + 27 rows over two calls: the bits of one call
    _, _, pre2 = host.boot_first(bc.imu_last(s, 0), bc.scan_time(0))
    host.preintegrate(pre2, s["rows"][1][:13])
    host.preintegrate(pre2, s["rows"][1][13:])
    assert np.array_equal(pre2.array(), b["pre"].array())
    host.preintegrate(pre2, np.zeros((0, 7)))
    assert np.array_equal(pre2.array(), b["pre"].array())


# ---- 2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seq", bc.SEQS)
def test_first_and_second_scan_against_the_references_records(pkg, host, ref, ref_seq, seqs, seq):
    """Records 0 and 1 of the NUM_ITER = 30 run; the ICP's pose is taken from record 1's linState_, so the ICP is out of
    the comparison."""
    s = seqs[seq]
    recs = bc.records(ref, ref_seq, pkg.default_params(num_iter=30), s, n=2)
    assert [r.status for r in recs] == [1, 3]
    lw = np.array(recs[1].lin_state[:])
    b = bc.host_bootstrap(host, s, icp_pose=(lw[0:3], lw[6:10]))
    # first scan: the zero initialisation, the offline covariance, identity linState_
    f0, lin0 = b["first"]
    pw = np.array(recs[0].filter_cov[:])
    assert np.abs(np.array(f0.state[:]) - np.array(recs[0].filter_state[:])).max() <= 1e-12
    assert np.abs(np.array(f0.cov[:]) - pw).max() <= 1e-12 * np.abs(pw).max()
    assert np.array_equal(lin0, np.array(recs[0].lin_state[:]))
    assert np.array_equal(np.array(list(f0.acc_last[:]) + list(f0.gyr_last[:])), np.array(recs[0].imu_last[:]))
    assert f0.time == bc.scan_time(0) and f0.has_imu == 1
    # second scan
    f1, g1, lin1 = b["second"]
    pw = np.array(recs[1].filter_cov[:])
    d = dict(filt=np.abs(np.array(f1.state[:]) - np.array(recs[1].filter_state[:])).max(),
             glob=np.abs(g1 - np.array(recs[1].global_state[:])).max(),
             cov=np.abs(np.array(f1.cov[:]) - pw).max() / np.abs(pw).max(), lin=np.abs(lin1 - lw).max())
    print(f"sequence {seq}: host bootstrap - reference", {k: f"{v:.2e}" for k, v in d.items()})
    assert d["filt"] <= 1e-12 and d["glob"] <= 1e-12 and d["cov"] <= 1e-12 and d["lin"] <= 1e-12, d
    assert np.array_equal(np.array(list(f1.acc_last[:]) + list(f1.gyr_last[:])), np.array(recs[1].imu_last[:]))
    assert np.array_equal(np.array(f1.state[0:3]), lw[0:3])  # position pl, not zero (SE:404-405)
    assert f1.time == bc.scan_time(1)


def _rp_quat_long_double(acc, ba):
    """calculateRPfromGravity (SE:602-605) + rpy2Quat (yaw 0) in long double"""
    L = np.longdouble
    f = np.asarray(acc, L) - np.asarray(ba, L)
    sg = L(1) if f[2] >= 0 else L(-1)
    pitch, roll = -sg * np.arcsin(f[0] / L(9.81)), sg * np.arcsin(f[1] / L(9.81))
    cr, sr, cp, sp = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2)
    return np.array([cr * cp, sr * cp, cr * sp, -sr * sp], L)  # w x y z with cy = 1, sy = 0


@pytest.mark.parametrize("acc", [(0.31, -0.27, 9.7), (0.31, -0.27, -9.7), (-1.2, 0.8, 9.5)])
def test_roll_and_pitch_from_gravity_both_signs(host, acc):
    """the gravity sample's z > 0 takes the other sign of SE:603-604 than every synthetic sequence does"""
    prm = host.boot_default_params()
    _, _, pre = host.boot_first(np.zeros(6), 0.1)
    pre.sum_dt = 0.1
    il = np.array(list(acc) + [0.0, 0.0, 0.0])
    f, g, _ = host.boot_second(pre, [0.01, -0.02, 0.003], [1.0, 0.0, 0.0, 0.0], il, 0.2, prm)
    want = _rp_quat_long_double(acc, prm.init_ba[:])
    assert np.abs(g[6:10] - want.astype(np.float64)).max() <= 1e-15
    assert np.array_equal(g[0:3], [0.01, -0.02, 0.003]) and np.array_equal(g[10:16], list(prm.init_ba[:]) + list(prm.init_bw[:]))
    assert np.array_equal(np.array(f.state[6:10]), [1.0, 0.0, 0.0, 0.0]) and np.array_equal(g[16:19], [0.0, 0.0, -9.81])


# ---- 3 ------------------------------------------------------------------------------------------------------------
def test_reference_sequence_continued_from_the_host_bootstrap(pkg, host, defs, oracle, ref, ref_seq):
    """Sequence 11 with no line of the reference's filter code: host bootstrap (the ICP by the CPU oracle's
    estimateTransform from the restatement's start pose), then scans 2 - 4 through the lins_filter_* mirror, the oracle's
    performIESKF and lins_filter_finish, the targets re-projected by lins_transform_to_end.  Against the unmodified
    reference's records: flags equal, linState_ 1e-5 m / 1e-6 rad, the filter after reset(1) 1e-5, globalState_ as
    seq_common.compare — the bars of tests/test_sequence.py's swapped chain."""
    s = bc.load(host, 11, 5)
    prm = pkg.default_params(num_iter=30)
    recs = bc.records(ref, ref_seq, prm, s)
    fe = [host.frontend_extract(r) for r in s["raws"]]
    b = bc.host_bootstrap(host, s)
    ident = np.array(b["first"][1])

    def pair(k, last, state, cov):
        return defs.ScanPair(fe[k]["surf_flat"], fe[k]["corner_sharp"], last[1], last[0], state, cov)

    last = (fe[0]["corner_less_sharp"], fe[0]["surf_less_flat"])  # a first scan's targets: as extracted
    t, q, rounds = oracle.icp(prm, pair(1, last, ident, np.eye(18) * 1e-4), *b["start"])
    f, g, lin = host.boot_second(b["pre"], t, q, bc.imu_last(s, 1), bc.scan_time(1))
    w = recs[1]
    assert w.status == 3 and np.abs(lin - np.array(w.lin_state[:])).max() <= 1e-6
    assert np.abs(np.array(f.state[:]) - np.array(w.filter_state[:])).max() <= 1e-5 and np.abs(g - np.array(w.global_state[:])).max() <= 1e-5
    worst = dict(lin_p=0.0, lin_a=0.0, filt=0.0, g_p=0.0, g_a=0.0)
    for k in (2, 3, 4):
        last = tuple(host.transform_to_end(lin[0:3], lin[6:10], fe[k - 1][name]) for name in ("corner_less_sharp", "surf_less_flat"))
        fc.host_predict(host, f, s["rows"][k])
        r = oracle.perform_ieskf(prm, pair(k, last, np.array(f.state[:]), np.array(f.cov[:]).reshape(18, 18)))
        g = host.filter_finish(f, g, r.state, r.cov, used_prior_cov=bool(r.diverged))
        lin, w = r.state, recs[k]
        assert w.ran_update and (r.iters, r.converged, r.diverged, r.m_surf, r.m_corner) == (w.iters, w.converged, w.diverged, w.m_surf, w.m_corner), k
        lw, gw = np.array(w.lin_state[:]), np.array(w.global_state[:])
        d = dict(lin_p=np.abs(lin[:3] - lw[:3]).max(), lin_a=seq_common.quat_angle(lin[6:10], lw[6:10]),
                 filt=np.abs(np.array(f.state[:]) - np.array(w.filter_state[:])).max(),
                 g_p=np.abs(g[:3] - gw[:3]).max(), g_a=seq_common.quat_angle(g[6:10], gw[6:10]))
        for key in worst:
            worst[key] = max(worst[key], float(d[key]))
        assert d["lin_p"] <= 1e-5 and d["lin_a"] <= 1e-6 and d["filt"] <= 1e-5 and d["g_p"] <= 1e-5 and d["g_a"] <= 1e-6, (k, d)
    print(f"host chain from the host bootstrap (ICP rounds {rounds}), scans 2 - 4, largest differences:", {k: f"{v:.2e}" for k, v in worst.items()})
