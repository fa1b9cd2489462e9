"""What tests/cov_cases.py claims of its cases, asserted with its model, and the conditions its reference is held to — on
the CPU, before any kernel is compared with it (tests/test_gpu_cov_update.py):
  the textbook form in f64 within 8 eps of the long-double one in e (the reference does not depend on the path to it);
  the rank-6 form in plain numpy f64 within 4 eps / shrink + 4 eps (the error model the kernels' bar is eight times of);
  the reference's smallest eigenvalue in correlation form, recorded per case;
and the oracle's joseph_reduced through the checks the device paths go through."""
import numpy as np
import pytest

import cov_cases as cc


def test_long_double_is_wider_than_f64():
    assert np.finfo(cc.LD).eps <= 2.0 ** -63


def test_every_claim_of_every_case():
    names = [c["name"] for c in cc.cases()]
    assert 24 <= len(names) <= 48
    for c in cc.cases():
        P, H = c["P"], c["H"]
        assert P.shape == (18, 18) and H.shape[1] == 18 and not H[:, [k for k in range(18) if k not in cc.S]].any(), c["name"]
        assert P.tobytes() == P.T.copy().tobytes() or c["diverged"], c["name"]
        # the 21 sums are H^T H exactly: the long-double product (64-bit significand, exact for entries on the grid) rounds to them
        A = H[:, cc.S].astype(cc.LD).T @ H[:, cc.S].astype(cc.LD)
        assert np.array_equal(A, cc.A_of(c["sums"]).astype(cc.LD)), c["name"]
        assert c["r2"] == c["lidar_std"] * c["lidar_std"]
        if c["diverged"]:
            continue
        d = np.sqrt(np.diag(P))
        live = d > 0
        assert np.linalg.eigvalsh(P[np.ix_(live, live)] / np.outer(d[live], d[live])).min() > 1e-4, c["name"]  # a covariance
        if c["shrink_target"]:
            assert 0.5 <= c["shrink"] / c["shrink_target"] <= 2.0, (c["name"], c["shrink"])
        if c["rank"] is not None:
            assert np.linalg.matrix_rank(H) == c["rank"], c["name"]
        order, tie = cc.pivot_order(P, c["sums"], c["r2"])
        if c["pivot"] == "k0":
            assert order[0] != 0, (c["name"], order)
        if c["pivot"] == "later":
            assert order[0] == 0 and order != list(range(6)), (c["name"], order)
        assert tie == c["tie"] or not c["pivot"], (c["name"], order, tie)
        if c["rho"]:
            C = P / np.outer(d, d)
            assert abs(C[0, 6] - c["rho"]) < 1e-14 and abs(C[1, 7] + c["rho"]) < 1e-14 and abs(C[2, 8] - c["rho"]) < 1e-14, c["name"]
        for r in c["zero_rows"]:
            assert not P[r].any() and not P[:, r].any() and c["ref"][r, r] == 0, (c["name"], r)
        if c["kept_rows"]:
            k = list(c["kept_rows"])
            assert not P[np.ix_(k, cc.S)].any() and np.abs(P[np.ix_(k, [3, 4, 5, 9, 10, 11, 15, 16, 17])]).min() > 0, c["name"]
            assert np.array_equal(c["ref"][k].astype(np.float64), P[k]), c["name"]  # (the reference keeps them exactly too)
        if c["returns_prior"]:
            assert np.array_equal(c["ref"].astype(np.float64), P), c["name"]
    # the ladder: every decade from 1e-2 to 1e-10 by the prior's scale and by |A| from 1e2 to 2e6; another r2
    for way in ("prior", "info"):
        got = sorted(c["shrink_target"] for c in cc.cases() if c["name"].startswith(f"ladder/{way}/"))
        assert np.allclose(got, sorted(cc.LADDER), rtol=1e-12), way
    sizes = [c["A_size"] for c in cc.cases() if c["name"].startswith("ladder/info/")]
    assert 1e2 <= min(sizes) < 2e2 and 1e6 <= max(sizes) <= 2e6
    assert any(c["r2"] != cc.LIDAR_STD ** 2 for c in cc.cases())
    stds = np.sqrt(np.diag(cc.by_name("blocks/all_correlated")["P"]))
    assert stds.max() / stds.min() >= 1e8
    C = cc.by_name("blocks/all_correlated")["P"] / np.outer(stds, stds)
    assert np.abs(C[np.ix_(cc.S, [k for k in range(18) if k not in cc.S])]).reshape(6, 4, 3).max(axis=(0, 2)).min() > 0.01  # S with every block
    assert np.isnan(cc.by_name("diverged/nan")["P"]).any()


def test_the_reference_does_not_depend_on_the_path_and_the_rank6_model_holds():
    worst_tb, worst_r6 = (0.0, ""), (0.0, "")
    for c in cc.cases():
        if c["diverged"]:
            continue
        tb = cc.err(cc.reference(c["P"], c["H"], c["r2"], np.float64), c["ref"])
        r6 = cc.err(cc.rank6_f64(c["P"], c["sums"], c["r2"]), c["ref"])
        model = cc.EPS / c["shrink"] + cc.EPS
        print(f"{c['name']:32s} shrink {c['shrink']:.3e}  textbook f64 e = {tb / cc.EPS:5.2f} eps  rank-6 f64 e = {r6:.2e} = {r6 / model:5.2f} (eps / shrink + eps)"
              f"  min eig (correlation form) {c['min_eig']:.3e}")
        assert tb <= 8 * cc.EPS, (c["name"], tb / cc.EPS)
        assert r6 <= 4 * model, (c["name"], r6 / model)
        assert c["min_eig"] > 0
        worst_tb, worst_r6 = max(worst_tb, (tb / cc.EPS, c["name"])), max(worst_r6, (r6 / model, c["name"]))
    print(f"textbook f64 against long double: worst {worst_tb[0]:.2f} eps at {worst_tb[1]}")
    print(f"rank-6 f64: worst constant {worst_r6[0]:.2f} at {worst_r6[1]}")


def test_the_metric_sees_what_max_norm_cannot():
    """an error of 1e-9 max|P| — what the whole-update tests allow — in the gyro bias block is far outside the bar"""
    c = cc.by_name("blocks/all_correlated")
    got = c["ref"].astype(np.float64)
    got[13, 13] += 1e-9 * np.abs(got).max()
    assert np.abs(got - c["ref"].astype(np.float64)).max() <= 1e-9 * np.abs(got).max() and cc.err(got, c["ref"]) > 1e6 * c["bar"]


def test_the_oracles_joseph_reduced(pkg, oracle):
    worst = (0.0, "")
    for c in cc.cases():
        if c["diverged"]:
            continue  # (the divergence branch is performIESKF's, not joseph_reduced's)
        prm = pkg.default_params()
        prm.lidar_std = c["lidar_std"]
        got = oracle.joseph_reduced(prm, c["P"], c["sums"])
        e = cc.check_output(c, got, "oracle")
        print(f"{c['name']:32s} oracle e = {e:.2e}  bar {c['bar']:.2e}")
        worst = max(worst, (e / c["bar"], c["name"]))
    print(f"oracle: worst e / bar = {worst[0]:.3f} at {worst[1]}")
