"""The loop-closure ICP's fit and stop step on built sums, on the CPU: what every case of tests/loop_fit_cases.py claims,
asserted from its exact reference alone; the calibration of the bar; and the CPU restatement's step
(lins_host_loop_icp_step over csrc/loop_icp_math.h: the text the device compiles too) against the reference within each
case's bar, with the properties that need no bar and every stop comparison at equality.  tests/test_gpu_loop_fit.py runs
the same cases through the device's step kernel."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import loop_fit_cases as fc
import loop_icp_np as lnp


def angle_of(R):
    return np.rad2deg(np.arccos(np.clip(0.5 * (np.trace(R) - 1.0), -1.0, 1.0)))


def test_every_case_is_what_it_claims():
    perms = set()
    for c in fc.fit_cases():
        r, name = c["ref"], c["name"]
        assert r["rank"] == c["rank"], name
        g = fc.gap(r)
        if c["rank"] == 3:
            assert (r["det_sign"], r["d"]) == ((-1, -1.0) if c["mirror"] else (1, 1.0)), name
        if fc.well_posed(c):
            assert g >= 1e-3, (name, g)
        if "want_gap" in c:  # the ladder: gap = e^2 / 4 by construction
            assert abs(g - c["want_gap"]) <= 1e-6 * c["want_gap"] and abs(c["want_gap"] / float(name.split("/")[1]) - 1) < 1e-6, (name, g)
        if name == "mirror":  # the stated gap: (sigma2 - sigma3) / sigma1 = (S y~^2 - S z^2) / S x~^2 = (40 - 0.125) / 168
            assert abs(g - 39.875 / 168.0) < 1e-3 and angle_of(r["R"]) < 1.0, (name, g)
        if c["perm"] is not None:  # which axis the k-th largest singular value belongs to
            assert tuple(int(k) for k in np.argmax(np.abs(r["V"]), 0)) == c["perm"], name
            perms.add(c["perm"])
        if c.get("plane") is not None:  # s and g in one plane of normal n: cof(H) = det(H2) n n^T / |n|^2, H2 the in-plane 2 x 2 H
            n, Hx = [Fraction(float(v)) for v in c["plane"]], r["Hx"]
            cof = [[Hx[(i + 1) % 3][(j + 1) % 3] * Hx[(i + 2) % 3][(j + 2) % 3] - Hx[(i + 1) % 3][(j + 2) % 3] * Hx[(i + 2) % 3][(j + 1) % 3]
                    for j in range(3)] for i in range(3)]
            det2 = sum(n[i] * cof[i][j] * n[j] for i in range(3) for j in range(3))
            nn = np.asarray(c["plane"]) / np.linalg.norm(c["plane"])
            if c["flips_plane"]:  # the in-plane optimum is a reflection: the proper rotation turns the plane over
                assert det2 < 0 and np.linalg.norm(r["R"] @ nn + nn) < 1e-12 and abs(angle_of(r["R"]) - 180.0) < 1e-5, name
            else:
                assert det2 > 0 and np.linalg.norm(r["R"] @ nn - nn) < 1e-12, name
        if "angle" in c:  # the f32 rounding of the points moves the fitted angle by 1e-6 degrees at most
            assert abs(angle_of(r["R"]) - c["angle"]) < 1e-4, (name, angle_of(r["R"]))
        if c["identity"] and fc.determined(c):
            assert np.array_equal(r["R"], np.eye(3)), name
        if c["dyadic"]:  # every sum exact: equal to the rational sum, in any order and over any tiling; the means exact
            x, y = fc._fr(c["X"]), fc._fr(c["G"])
            exact = [Fraction(len(x))] + [sum(p[i] for p in x) for i in range(3)] + [sum(p[i] for p in y) for i in range(3)]
            exact += [sum(p[i] * q[j] for p, q in zip(x, y)) for i in range(3) for j in range(3)]
            assert [Fraction(float(v)) for v in c["sums"][:16]] == exact, name
            assert np.array_equal(fc.sums(c["X"][::-1], c["G"][::-1])[:16], c["sums"][:16]), name
            for tiles in (2, 5):
                assert np.array_equal(fc.split(c["X"], c["G"], tiles).sum(0)[:16], c["sums"][:16]), (name, tiles)
            if c["exact"]:
                assert all(Fraction(float(c["sums"][k] / len(x))) == exact[k] / len(x) for k in range(1, 7)), name
    assert perms == set(itertools.permutations(range(3)))
    assert {c["rank"] for c in fc.fit_cases()} == {0, 1, 2, 3}


def test_the_end_to_end_clouds_pair_up_in_order():
    """mirror and planar as clouds: 1 m spacing, 1/8 m resp. 0.1 m displacement — nearest-neighbour pairing at T = I is the
    identity pairing, and the moved source is the source, so the search's sums are the built ones"""
    for pairs in (fc.mirror_pairs, fc.planar_pairs):
        for n in (31, 32, 33):
            X, G = pairs(n)
            S, T = np.concatenate([X, np.zeros((n, 1), np.float32)], 1), np.concatenate([G, np.zeros((n, 1), np.float32)], 1)
            idx, d, moved = lnp.correspondences(S, T, np.eye(4), 100.0)
            assert np.array_equal(idx, np.arange(n)) and np.array_equal(moved, X) and np.array_equal(d, fc.sqd(X, G))


def test_the_bars_constants_come_from_the_references():
    ratio, where = fc.calibrate()
    floor = fc.collinear_floor()
    print(f"raw moments + LAPACK against the exact reference: worst |dR| / (bar_R / K) = {ratio:.3f} at {where}; K = {fc.K}")
    print(f"exactly collinear points, raw moments + LAPACK: sigma2 / sigma1 <= {floor:.0f} x 2^-53; C_RANK = {fc.C_RANK:.0f}")
    assert ratio <= fc.K / 4 and 4 * floor <= fc.C_RANK  # (K and C_RANK are 8 x what was measured; half of that margin is asserted)


def test_host_step_is_the_reference_within_each_cases_bar(host):
    worst, worst_ortho = (0.0, ""), 0.0
    for c in fc.fit_cases():
        st, D, q = host.loop_icp_step(c["sums"])
        assert np.array_equal(D, st["T"]), c["name"]  # T_in = I: the composition returns the fit's bits
        ratio, ortho = fc.check_fit(c, st, "host")
        want = fc.numpy_round(c)
        if fc.determined(c):  # (the numpy statement's own fit is within the bar too)
            lim = 2 * (fc.bar_R(c["ref"]) + fc.bar_t(c["ref"]) * (1 + np.linalg.norm(D[:3, 3])))
            assert abs(q[0] - want["stop"][0]) <= lim and abs(q[1] - want["stop"][1]) <= lim, (c["name"], q, want["stop"])
        else:
            assert q[0] == 1.0 and q[1] == (D[0, 3] * D[0, 3] + D[1, 3] * D[1, 3]) + D[2, 3] * D[2, 3], (c["name"], q)
        assert q[2] == want["stop"][2] and q[3] == want["stop"][3], (c["name"], q, want["stop"])
        worst, worst_ortho = max(worst, (ratio, c["name"])), max(worst_ortho, ortho)
    print(f"host against the reference: worst |dR| / bar_R = {worst[0]:.3f} at {worst[1]}; |R^T R - I| <= {worst_ortho:.2e} (bar {fc.ORTHO:.2e})")


def test_far_origin_reports_what_raw_moments_cost(host):
    for c in fc.fit_cases():
        if "far" in c:
            st, D, _ = host.loop_icp_step(c["sums"])
            r = c["ref"]
            print(f"{c['name']}: |dR| = {np.linalg.norm(D[:3, :3] - r['R']):.2e} (bar {fc.bar_R(r):.2e}), |dt| = {np.linalg.norm(D[:3, 3] - r['t']):.2e} "
                  f"(bar {fc.bar_t(r):.2e}), m / sigma1 = {r['m'] / r['sig'][0]:.2e}")


def test_the_fits_residual_is_the_minimum(host):
    """independent of R: S |R x' + t - g|^2 of the returned fit, in rational arithmetic, against the reference's.  Two fits
    within (bR, bt) of the optimum differ in every residual vector by at most 2 bR |x~_k| + 2 bt, so the roots of the two
    sums differ by at most 2 bR sqrt(P) + 2 bt sqrt(n), P = S |x~_k|^2: a wrong branch (a reflection, a turn about the
    wrong axis) misses this by orders of magnitude even where the forward bar is loose."""
    for c in fc.fit_cases():
        if not fc.well_posed(c) or c.get("far", 0) > 0:  # (far_origin: the Fraction sums are the same work; the forward bar is tight enough)
            continue
        r = c["ref"]
        st, D, _ = host.loop_icp_step(c["sums"])
        Dref = np.eye(4)
        Dref[:3, :3], Dref[:3, 3] = r["R"], r["t"]
        got, want = float(fc.residual_exact(D, c["X"], c["G"])), float(fc.residual_exact(Dref, c["X"], c["G"]))
        xc = c["X"].astype(np.float64) - r["mu_s"]
        slack = 2 * fc.bar_R(r) * np.sqrt((xc * xc).sum()) + 2 * fc.bar_t(r) * np.sqrt(len(xc))
        assert np.sqrt(got) <= np.sqrt(want) + slack, (c["name"], got, want, slack)


def test_composition_with_a_running_transform(host):
    """T_out = Delta T_in entry by entry in the contract's order, bottom row (0, 0, 0, 1) exactly"""
    for name in ("rotations/generic120", "mirror", "planar/generic", "three_points"):
        c = fc.by_name(name)
        st, D, q = host.loop_icp_step(c["sums"], state=dict(T=fc.T_IN, mse_prev=0.5, iterations=3))
        st0, D0, _ = host.loop_icp_step(c["sums"])
        assert np.array_equal(D, D0) and st["iterations"] == 4
        want = np.array([[((D[i, 0] * fc.T_IN[0, j] + D[i, 1] * fc.T_IN[1, j]) + D[i, 2] * fc.T_IN[2, j]) + D[i, 3] * fc.T_IN[3, j] for j in range(4)]
                         for i in range(4)])
        assert np.array_equal(st["T"], want) and np.array_equal(st["T"][3], [0, 0, 0, 1]), name
        assert np.abs(st["T"] - D @ fc.T_IN).max() <= 4 * fc.U53 * (np.abs(D) @ np.abs(fc.T_IN)).max()
        mse = c["sums"][16] / c["sums"][0]
        assert q[2] == abs(mse - 0.5) and q[3] == abs(mse - 0.5) / 0.5


def test_every_stop_comparison_at_equality(host):
    for edge in fc.stop_edges():
        name, v, kw, st_in, reason = edge
        st, D, q = host.loop_icp_step(v, host.loop_icp_params(**kw), state=st_in)
        fc.check_stop_edge(edge, st, "host")
        if reason != lnp.NO_CORRESPONDENCES:
            assert q[0] == 1.0 and q[1] == fc.STOP_T2, (name, q)
            if "mse_prev" in st_in:
                assert q[2] == abs(v[16] / 8 - 0.5) and q[3] == q[2] / 0.5, (name, q)
            else:
                assert q[2] == lnp.DBL_MAX and q[3] == 1.0, (name, q)
        else:
            assert np.array_equal(D, np.eye(4)) and np.array_equal(q, np.zeros(4)), name
    assert {e[4] for e in fc.stop_edges()} == set(range(6))


def test_fitness_mode_and_an_inactive_problem(host):
    v = fc.stop_sums(0.25)
    st, _, _ = host.loop_icp_step(v, mode=1, state=dict(T=fc.T_IN, active=0, iterations=7, mse=0.125, mse_prev=0.125))
    assert (st["fitness"], st["n_fitness"], st["iterations"], st["active"]) == (0.25, 8, 7, 0) and st["T"].tobytes() == fc.T_IN.tobytes()
    v3 = v.copy()
    v3[0], v3[16] = 3.0, 1.0
    assert host.loop_icp_step(v3, mode=1)[0]["fitness"] == 1.0 / 3.0
    st, _, _ = host.loop_icp_step(np.zeros(17), mode=1)
    assert (st["fitness"], st["n_fitness"]) == (lnp.DBL_MAX, 0)
    gone = dict(T=fc.T_IN, active=0, iterations=7, mse=0.125, mse_prev=0.375, reason=lnp.ABS_MSE, converged=1, n_corr=5)
    st, D, q = host.loop_icp_step(v, state=gone)  # a stopped problem is not stepped
    assert all(st[k] == gone[k] for k in gone if k != "T") and st["T"].tobytes() == fc.T_IN.tobytes()
    with pytest.raises(RuntimeError, match="-1"):
        host.loop_icp_step(v, mode=2)
