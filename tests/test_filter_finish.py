"""lins_filter_finish (csrc/host/filter_finish.cpp, arithmetic: csrc/filter_math.h) against the reference's own state
machine: what processScan does to the filter and to globalState_ after performIESKF — filter_->update,
integrateTransformation, reset(1), calculateRPfromGravity + correctRollPitch (SE:443-453) — must reproduce the
records of oracle/ref_seq.py from one scan to the next."""
import os

import numpy as np
import pytest

import filter_common as fc
import seq_common


@pytest.fixture(scope="module")
def ref_seq():
    from oracle import ref_seq as r

    if not r.available():
        if os.environ.get("LINS_REQUIRE_REF") == "1":
            pytest.fail("LINS_REQUIRE_REF=1 and oracle/_ref/liblins_ref_seq.so is neither built nor buildable here")
        pytest.skip("oracle/_ref/liblins_ref_seq.so not built and /root/reference not present")
    r.lib()
    return r


def test_finish_reproduces_the_references_global_state_and_reset_filter(pkg, host, ref_seq):
    """20 scans of synthetic sequence 11.  For every scan k >= 2 that ran an update: from globalState_ of scan k - 1, the
    posterior linState_ of scan k and the host filter chain's covariance (the records keep Pk_ only after reset(1): the
    covariance handed over is the host StatePredictor mirror's prior over the scan's 40 IMU rows, from the reference's
    filter of scan k - 1 — the state half of the check does not read it), lins_filter_finish must give globalState_ and
    the filter state of scan k to 1e-12, with the zeros and the identity quaternion of reset(1) exact, and the covariance
    structure reset(1) leaves: zero outside the six diagonal blocks, the bias blocks carried over bit for bit."""
    prm = pkg.default_params(num_iter=30)
    n_scans = 20
    inputs = seq_common.sequence_inputs(host, 11, n_scans)
    recs = seq_common.run(ref_seq, prm, inputs)
    worst_g = worst_f = 0.0
    checked = 0
    for k in range(2, n_scans):
        w = recs[k]
        if not w.ran_update:
            continue
        f = fc.filter_from_record(host, recs[k - 1])
        fc.host_predict(host, f, fc.imu_rows(inputs[k][1], inputs[k][2]))
        prior_cov = np.array(f.cov[:]).reshape(18, 18)
        g = host.filter_finish(f, recs[k - 1].global_state[:], w.lin_state[:], prior_cov, used_prior_cov=bool(w.used_icp))
        dg = float(np.abs(g - np.array(w.global_state[:])).max())
        st = np.array(f.state[:])
        df = float(np.abs(st - np.array(w.filter_state[:])).max())
        worst_g, worst_f = max(worst_g, dg), max(worst_f, df)
        assert dg <= 1e-12 and df <= 1e-12, (k, dg, df)
        assert np.array_equal(st[0:3], np.zeros(3)) and np.array_equal(st[6:10], [1.0, 0.0, 0.0, 0.0]), k
        cov = np.array(f.cov[:]).reshape(18, 18)
        mask = np.zeros((18, 18), bool)
        for b in range(0, 18, 3):
            mask[b:b + 3, b:b + 3] = True
        assert np.array_equal(cov[~mask], np.zeros((~mask).sum())), k
        assert np.array_equal(cov[0:3, 0:3], np.zeros((3, 3))) and np.array_equal(cov[6:9, 6:9], np.zeros((3, 3))), k  # init_*_std = 0
        assert np.array_equal(cov[9:15, 9:15][mask[9:15, 9:15]], prior_cov[9:15, 9:15][mask[9:15, 9:15]]), k
        # the same blocks reset(1) of the mirror leaves, from the same covariance
        checked += 1
    assert checked >= 17
    print(f"lins_filter_finish against the reference's records, {checked} scans: globalState_ {worst_g:.2e}, filter state {worst_f:.2e}")


def test_finish_equals_update_then_the_mirrors_reset1(host):
    """the filter half of lins_filter_finish is filter_->update + lins_filter_reset1 (pinned to the reference's reset(1) to
    1e-14 by tests/test_ref.py), bit for bit — also with non-zero init_pos_std / init_att_std and with the prior
    covariance kept (the diverged branch)."""
    import ctypes as C

    rng = np.random.default_rng(11)
    for trial in range(4):
        f, _ = fc.new_filter(host, vn=rng.normal(size=3), ba=rng.normal(size=3) * 0.05, bw=rng.normal(size=3) * 0.003,
                             pos_std=[0.02, 0.03, 0.01] if trial % 2 else None, att_std=[0.5, 0.4, 0.3] if trial % 2 else None)
        rows = fc.imu_rows(rng.normal(size=(7, 3)) * 0.3 + [0, 0, 9.81], rng.normal(size=(7, 3)) * 0.05)
        fc.host_predict(host, f, rows)
        post = np.array(f.state[:])
        post[0:3] += rng.normal(size=3) * 0.1
        q = post[6:10] + rng.normal(size=4) * 0.05
        post[6:10] = q / np.linalg.norm(q)
        a = rng.normal(size=(18, 18)) * 1e-2
        pcov = a @ a.T
        keep_prior = trial >= 2
        want = fc.copy_filter(host, f)
        want.state[:] = post
        if not keep_prior:
            want.cov[:] = pcov.reshape(324)
        host.lib().lins_filter_reset1(C.byref(want))
        g0 = np.array([1, 2, 3, 0.1, 0.2, 0.3, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -9.81], dtype=np.float64)
        host.filter_finish(f, g0, post, pcov, used_prior_cov=keep_prior)
        assert fc.filters_bitwise_equal(f, want), trial
