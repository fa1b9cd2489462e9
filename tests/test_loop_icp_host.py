"""The CPU restatement of the loop-closure ICP (csrc/host/loop_icp.cpp over csrc/loop_icp_math.h: the text the device
compiles too) against the independent numpy statement tests/loop_icp_np.py: correspondences and d bit for bit, the same
stop round / reason / counts, T, mse and fitness within the bar that summation order and SVD algorithm explain
(loop_icp_cases.BAR_*: measured here, printed, used with a x10 margin), both sides of every stop rule, and the
camera / lidar frame shuffle of LM:1156-1166."""
import numpy as np
import pytest

import loop_icp_cases as cases
import loop_icp_np as lnp


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def prm(host, **kw):
    return host.loop_icp_params(**kw)


def same_outcome(got, want):
    return all(got[k] == want[k] for k in ("iterations", "converged", "reason", "n_corr", "n_fitness"))


def test_correspondences_are_the_numpy_statements_bit_for_bit(host):
    probs = [(n, s, t, np.eye(4), 0.0) for n, s, t in cases.search_cases()]
    s, t = cases.beyond_cap_case()
    probs += [("beyond cap", s, t, np.eye(4), 100.0), ("beyond cap, none", s, t, np.eye(4), 0.0)]
    for k, (s, t) in enumerate(cases.all_whole_loop_clouds()):
        rounds, _ = host.loop_icp_trace(s, t)
        probs += [(f"loop {k} round {r}", s, t, rounds[r]["T_in"], 100.0) for r in (0, len(rounds) // 2, len(rounds) - 1)]
    for name, s, t, T, cap in probs:
        idx, d = host.loop_icp_correspondences(s, t, T, cap)
        widx, wd, _ = lnp.correspondences(s, t, T, cap)
        assert np.array_equal(idx, widx), name
        assert np.array_equal(bits(d), bits(wd)), name
    s, t = cases.beyond_cap_case()
    assert host.loop_icp_correspondences(s, t, np.eye(4), 100.0)[0][0] == -1 and host.loop_icp_correspondences(s, t, np.eye(4), 0.0)[0][0] >= 0


def test_every_round_is_the_numpy_statements_within_the_bar(host):
    worst = dict(T=0.0, mse=0.0, fitness=0.0)
    for k, (s, t) in enumerate(cases.all_whole_loop_clouds()):
        rounds, res = host.loop_icp_trace(s, t)
        wrounds, wres = lnp.icp(s, t)
        assert len(rounds) == len(wrounds) and same_outcome(res, wres), (k, res, wres)
        assert same_outcome(host.loop_icp(s, t), wres)
        for r, (a, b) in enumerate(zip(rounds, wrounds)):
            assert (a["n_corr"], a["reason"]) == (b["n_corr"], b["reason"]), (k, r)
            assert np.array_equal(a["T_in"], rounds[r - 1]["T_out"] if r else np.eye(4))
            worst["T"] = max(worst["T"], np.abs(a["T_out"] - b["T_out"]).max(), np.abs(a["delta"] - b["delta"]).max())
            worst["mse"] = max(worst["mse"], abs(a["mse"] - b["mse"]))
            assert np.allclose(a["stop"][:2], b["stop"][:2], rtol=0, atol=cases.BAR_T * 10), (k, r)
        assert np.array_equal(res["transform"], rounds[-1]["T_out"])
        worst["fitness"] = max(worst["fitness"], abs(res["fitness"] - wres["fitness"]))
        worst["T"] = max(worst["T"], np.abs(res["transform"] - wres["transform"]).max())
    print("host against numpy, largest difference:", worst)
    assert worst["T"] <= cases.BAR_T and worst["mse"] <= cases.BAR_MSE and worst["fitness"] <= cases.BAR_MSE, worst


def test_rounds_limit_reports_the_last_round_run(host):
    s, t = cases.all_whole_loop_clouds()[0]
    rounds, _ = host.loop_icp_trace(s, t)
    for r in (1, 3, len(rounds)):
        got = host.loop_icp(s, t, max_rounds=r)
        assert (got["iterations"], got["reason"], got["n_corr"]) == (r, rounds[r - 1]["reason"], rounds[r - 1]["n_corr"])
        assert np.array_equal(got["transform"], rounds[r - 1]["T_out"]) and got["mse"] == rounds[r - 1]["mse"]
        assert got["converged"] == (rounds[r - 1]["reason"] != lnp.NONE)


def test_both_sides_of_every_stop_rule(host):
    """each rule fires where its quantity is on the stopping side of its threshold and not where it is on the other —
    thresholds placed a factor 2 either side of the quantities the default run's trace shows, no debug hook involved"""
    s, t = cases.all_whole_loop_clouds()[0]
    rounds, res = host.loop_icp_trace(s, t)
    assert res["reason"] == lnp.TRANSFORM and len(rounds) > 5
    never_b = dict(rotation_threshold=2.0)  # 0.5 (trace - 1) <= 1: rule (b) cannot fire
    at = 3
    ad, rel = rounds[at]["stop"][2], rounds[at]["stop"][3]

    def first(col, thr):  # the round count at which a rule with this threshold stops, as far as the trace tells
        hits = [r for r, rd in enumerate(rounds) if rd["stop"][col] < thr]
        return (hits[0] + 1, None) if hits else None

    variants = [
        (dict(max_iterations=3), (3, lnp.ITERATIONS)),
        (dict(max_iterations=4), (4, lnp.ITERATIONS)),
        (dict(), (len(rounds), lnp.TRANSFORM)),
        (dict(never_b, fitness_epsilon=2 * ad, rel_mse=0.0), first(2, 2 * ad) + (lnp.ABS_MSE, at + 1)),
        (dict(never_b, fitness_epsilon=0.5 * ad, rel_mse=0.0), first(2, 0.5 * ad)),  # not at `at`
        (dict(never_b, fitness_epsilon=0.0, rel_mse=2 * rel), first(3, 2 * rel) + (lnp.REL_MSE, at + 1)),
        (dict(never_b, fitness_epsilon=0.0, rel_mse=0.5 * rel), first(3, 0.5 * rel)),
        (dict(min_correspondences=len(s) + 1), (0, lnp.NO_CORRESPONDENCES)),
        (dict(min_correspondences=len(s), max_iterations=2), (2, lnp.ITERATIONS)),
        (dict(max_corr_dist=1e-4), (0, lnp.NO_CORRESPONDENCES)),
    ]
    # rule (b) needs both halves: with either threshold out of reach the default run goes on past its stop round
    last = rounds[-1]["stop"]
    variants += [(dict(transformation_epsilon=0.5 * last[1], max_iterations=len(rounds) + 1), (len(rounds) + 1, None)),
                 (dict(rotation_threshold=1.5, max_iterations=len(rounds) + 1), (len(rounds) + 1, None))]
    for kw, want in variants:
        got = host.loop_icp(s, t, prm(host, **kw))
        _, wres = lnp.icp(s, t, **kw)
        assert same_outcome(got, wres), (kw, got, wres)
        assert got["converged"] == (got["reason"] != lnp.NO_CORRESPONDENCES)
        if want is None:  # the trace never has the quantity below this threshold: the run goes on past it
            assert got["iterations"] > len(rounds), (kw, got)
        elif len(want) == 4:  # (round count by the trace, -, reason, the latest round it may be)
            assert got["iterations"] == want[0] <= want[3] and got["reason"] == want[2], (kw, got, want)
        else:
            assert got["iterations"] == want[0] and (want[1] is None or got["reason"] == want[1]), (kw, got)
            assert got["iterations"] != at + 1 or "max_iterations" in kw or kw == {} or "transformation_epsilon" in kw or "rotation_threshold" in kw, (kw, got)
    # too few correspondences keeps T
    got = host.loop_icp(s, t, prm(host, min_correspondences=len(s) + 1))
    assert np.array_equal(got["transform"], np.eye(4)) and got["n_corr"] == len(s) and got["n_fitness"] == len(s)


def test_empty_clouds_stop_at_round_0(host):
    s, t = cases.all_whole_loop_clouds()[0]
    e = np.zeros((0, 4), np.float32)
    for a, b in ((e, t), (s, e), (e, e)):
        got = host.loop_icp(a, b)
        assert (got["iterations"], got["converged"], got["reason"], got["n_corr"], got["n_fitness"]) == (0, 0, lnp.NO_CORRESPONDENCES, 0, 0 if len(a) == 0 or len(b) == 0 else len(a))
        assert got["fitness"] == lnp.DBL_MAX
    bad = s.copy()
    bad[3, 1] = np.nan
    with pytest.raises(RuntimeError, match="-4"):
        host.loop_icp(bad, t)


def test_pose_from_is_the_numpy_restatement_to_f32_rounding(host):
    rng = np.random.default_rng(3)
    for (s, t), wrong in zip(cases.all_whole_loop_clouds(), [p[2] for p in cases.whole_loop_problems()] + [cases.archive_case()[2]]):
        T = host.loop_icp(s, t)["transform"]
        for w in (wrong, (wrong + rng.normal(0, 0.3, 6)).astype(np.float32)):
            got, want = host.loop_pose_from(T, w), lnp.pose_from(T, w)
            # a dozen f32 operations on values of magnitude max(1, |v|): 64 units in the last place
            assert np.all(np.abs(got - want) <= 64 * 2.0 ** -24 * np.maximum(1.0, np.abs(want))), (got, want)
    # no correction: tWrong itself, whose extraction carries the camera-to-lidar shuffle (z, x, y, yaw, roll, pitch)
    ident = host.loop_pose_from(np.eye(4), (1.0, 2.0, 3.0, 0.1, 0.2, 0.3))
    assert np.allclose(ident, [3.0, 1.0, 2.0, 0.3, 0.1, 0.2], atol=1e-6)
