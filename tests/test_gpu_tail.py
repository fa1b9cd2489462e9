"""The serial tail of an iteration of the LDS IESKF kernels (csrc/ieskf_lds_tail.h) in every kernel shape, on inputs chosen
with the CPU oracle so that the oracle itself shows each branch of the tail: the stop rule met late, early and in the
first iteration (the convergence flag and |dx| come from another wave than the solve), divergence by residual growth
and by a NaN increment (the state and |dx| that are kept), rotations outside the short-series range of the rotation maps
(the libm fall-backs, taken by some of the waves that share the next iteration's constants and not by others), and an
update cut after every iteration (the tail's state handed over through global memory).

Bars: flags, iteration and row counts equal to the oracle's; state, covariance and residual within TIGHT_STATE /
TIGHT_COV / 1e-12 of tests/test_gpu_parity.py.  update_norm is |dx| of the last accepted step, a norm of quantities of
the state's size: the residual's form of bar, TIGHT_STATE relative to max(1, |dx|).  tests/golden/tail_parent_bits.npz
holds what the library gave for the fixed-iteration batch in the batch shape BEFORE the tail was reorganised (written
by this project's own library on an MI355X): the reorganisation moved work between waves, no operation of the
arithmetic, so the bits must be those.
"""
import os

import numpy as np
import pytest

from test_gpu_parity import TIGHT_COV, TIGHT_STATE, _max_parts, _run_cut, _same_bits

pytestmark = pytest.mark.gpu

SHAPES = ["mr", "lds1", "lds"]
START = 31000  # first synthetic pair of the batch the golden file was recorded on
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tail_parent_bits.npz")
FAST_QUAT2AXIS_ANGLE = 2 * np.arctan(1.0 / 8.0)  # lins_math.h kFastTanSq: tan(angle / 2) <= 1 / 8 (0.2487 rad)


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def _yawed(host, oracle, index, yaw, att_var=None):
    """Synthetic pair `index` with the prior attitude turned by `yaw` about z (and, optionally, a loose attitude prior)."""
    p = host.synth_pair(index)
    p.state[6:10] = _qmul(p.state[6:10], oracle.axis2quat(np.array([0.0, 0.0, yaw])))
    if att_var is not None:
        c = p.cov.reshape(18, 18)
        for k in (6, 7, 8):
            c[k, k] = att_var
    return p


def _big_turn_pair(pkg, lever=0.3, off=0.4):
    """A hand-built pair (after tests/diverging.py) whose increments turn by more than 1 rad: ONE plane query, `off` above
    a horizontal plane and `lever` beside the x axis, and a prior covariance that leaves only the rotation about x free —
    the one row is explained by dth_x = off / lever = 1.33 rad.  The turned query then lies far from the plane, no row is
    accepted, and the next increment is x_filter (-) x_lin: 1.33 rad back.  Ring-sorted targets with ring ids 0 / 1."""
    f = np.float32
    a, b, d = np.array([0.0, 0.0, -1.5]), np.array([-0.4, 0.35, -1.5]), np.array([0.45, 0.3, -1.5])
    surf_last = np.zeros((3, 4), dtype=f)
    surf_last[0, :3], surf_last[0, 3] = d, 0.05  # ring 0: the third point
    surf_last[1, :3], surf_last[2, :3] = b, a  # ring 1: second, first (backward walk)
    surf_last[1:, 3] = 1.05
    surf_flat = np.zeros((1, 4), dtype=f)
    surf_flat[0, :3] = a + np.array([0.03, lever, off])
    surf_flat[0, 3] = f(1.0) + f(0.1)  # ring 1, relative time 1: the whole transform applies
    state = np.zeros(19)
    state[6] = 1.0
    state[18] = -9.81
    cov = np.zeros((18, 18))
    cov[6, 6] = 1e6
    empty = np.zeros((0, 4), dtype=f)
    return pkg.ScanPair(surf_flat, empty, surf_last, empty, state, cov)


@pytest.fixture(scope="module")
def cases(pkg, host, oracle):
    """name -> (params, pairs, the oracle's results, the oracle's traces); computed once, never modified."""
    from diverging import make_diverging_pair

    fixed = pkg.default_params(num_iter=10, fixed_iters=1)
    stop = pkg.default_params(num_iter=30)
    inputs = {"fixed": (fixed, host.synth_batch(8, start=START)),
              "stop": (stop, host.synth_batch(4, start=START))}
    tight = host.synth_batch(3, start=START)  # (b) a prior that hardly moves: the covariance scaled down
    for p in tight:
        p.cov *= 1e-4
    inputs["first"] = (stop, tight)
    inputs["growth"] = (stop, [make_diverging_pair(pkg), host.synth_pair(START)])  # (c), next to an ordinary scan
    nan = host.synth_batch(2, start=START)  # (d) one NaN in the prior covariance of the first scan
    nan[0].cov.reshape(18, 18)[0, 0] = np.nan
    inputs["nan"] = (stop, nan)
    # (e) the prior attitude 0.6 / 0.3 rad off.  With the tight attitude prior of the generator q stays there: phi, Rinvleft of
    # EVERY iteration take the libm path (wave 1) while x_filter (-) x_lin stays small (wave 2: short series).  With a
    # loose attitude prior q returns to the truth: phi in range, x_filter (-) x_lin grows past the range on the way.
    # (Attitude variance 1e-3: an input is admitted only where the oracle's own two algebraic forms of the update agree
    # three orders inside TIGHT_STATE, see the test.  With 1e-2 the same scans take 18 iterations along which the accepted
    # rows flip, and the oracle's dense and reduced forms — equal algebra, different rounding — end 2.3e-8 apart: such an
    # input measures the conditioning of the update, not the device.)
    inputs["far"] = (stop, [_yawed(host, oracle, START + 1, 0.6), _yawed(host, oracle, START + 1, 0.3, att_var=1e-3),
                            _yawed(host, oracle, START + 2, 0.3, att_var=1e-3)])
    inputs["turn"] = (stop, [_big_turn_pair(pkg), host.synth_pair(START)])  # (e) dth beyond 1 rad, next to an ordinary scan
    out = {}
    for name, (prm, pairs) in inputs.items():
        res, traces = [], []
        for p in pairs:
            r, tr = oracle.ieskf(prm, p, oracle.FORM_DENSE, oracle.NN_KDTREE, trace=True)
            res.append(r), traces.append(tr)
        out[name] = (prm, pairs, res, traces)
    return out


def _run(ieskf, prm, pairs, search):
    with ieskf.IeskfContext(prm, max_batch=len(pairs), max_targets=16384, search=search) as c:
        res = c.update_batch(pairs)
        assert c.last_search() == search
    return res


def _assert_tight(got, want, what):
    assert (got.iters, got.converged, got.diverged) == (want.iters, want.converged, want.diverged), (what, got, want)
    assert (got.m_surf, got.m_corner) == (want.m_surf, want.m_corner), (what, got, want)
    gc, wc = np.asarray(got.cov).ravel(), np.asarray(want.cov).ravel()
    assert np.array_equal(np.isnan(gc), np.isnan(wc)) and not np.isnan(got.state).any(), what
    ok = ~np.isnan(wc)
    ds = np.abs(got.state - want.state).max()
    dc = np.abs(gc[ok] - wc[ok]).max() / np.abs(wc[ok]).max()
    dr = abs(got.residual_norm - want.residual_norm) / max(1.0, want.residual_norm)
    du = abs(got.update_norm - want.update_norm) / max(1.0, want.update_norm)
    print(f"{what}: state {ds:.2e}, covariance {dc:.2e} (rel), residual {dr:.2e}, update_norm {du:.2e}")
    assert ds <= TIGHT_STATE and dc <= TIGHT_COV and dr <= 1e-12 and du <= TIGHT_STATE, what


def _check(ieskf, cases, name, search):
    prm, pairs, want, _ = cases[name]
    got = _run(ieskf, prm, pairs, search)
    for k, (g, w) in enumerate(zip(got, want)):
        _assert_tight(g, w, f"{name}[{k}] {search}")
    return got


@pytest.mark.parametrize("search", SHAPES)
def test_fixed_iterations_and_the_stop_rule_met_late(ieskf, cases, search):
    """(a) ten fixed iterations, and the reference's stop rule met after several: the loop ends on the flag wave 3 wrote."""
    assert all((w.iters, w.converged, w.diverged) == (10, 0, 0) for w in cases["fixed"][2])
    assert all(w.converged and not w.diverged and 1 < w.iters < 30 for w in cases["stop"][2])
    assert any(w.iters < 10 for w in cases["stop"][2])
    _check(ieskf, cases, "fixed", search)
    _check(ieskf, cases, "stop", search)


def test_fixed_iterations_reproduce_the_bits_recorded_before_the_tail_was_reorganised(ieskf, cases):
    """The batch shape on the 8 scans of (a) against tests/golden/tail_parent_bits.npz, bit for bit."""
    prm, pairs, _, _ = cases["fixed"]
    got = _run(ieskf, prm, pairs, "mr")
    g = np.load(GOLDEN)
    assert np.array_equal(np.array([r.state for r in got]), g["state"])
    assert np.array_equal(np.array([np.asarray(r.cov).reshape(324) for r in got]), g["cov"])
    assert np.array_equal(np.array([r.residual_norm for r in got]), g["residual_norm"])
    assert np.array_equal(np.array([r.update_norm for r in got]), g["update_norm"])
    assert np.array_equal(np.array([[r.iters, r.converged, r.diverged, r.m_surf, r.m_corner] for r in got], dtype=np.int32), g["counts"])


@pytest.mark.parametrize("search", SHAPES)
def test_stop_rule_met_in_the_first_iteration(ieskf, cases, search):
    """(b) a prior within the stop rule: one iteration, converged."""
    assert all((w.iters, w.converged, w.diverged) == (1, 1, 0) for w in cases["first"][2])
    _check(ieskf, cases, "first", search)


@pytest.mark.parametrize("search", SHAPES)
def test_residual_growth_keeps_the_filter_state_and_the_previous_update_norm(ieskf, cases, search):
    """(c) tests/diverging.py: |r| of the second iteration is more than ten times the first's.  diverged == 1, the state is
    the filter's, update_norm is the FIRST iteration's |dx| (the trace's), the covariance is the prior."""
    prm, pairs, want, traces = cases["growth"]
    assert (want[0].iters, want[0].diverged) == (2, 1) and want[1].diverged == 0
    assert abs(want[0].update_norm - np.linalg.norm(traces[0]["dx"][0])) <= 1e-12 * want[0].update_norm
    got = _check(ieskf, cases, "growth", search)
    assert np.array_equal(got[0].state, pairs[0].state) and np.array_equal(np.asarray(got[0].cov).ravel(), pairs[0].cov.ravel())


@pytest.mark.parametrize("search", SHAPES)
def test_nan_increment_diverges_in_the_first_iteration(ieskf, cases, search):
    """(d) a NaN entry of the prior covariance (the input contract checks clouds, not priors) makes dx NaN: diverged == 2
    after one iteration, the filter state returned, update_norm as it was set up (0), the prior passed through."""
    prm, pairs, want, _ = cases["nan"]
    assert (want[0].iters, want[0].converged, want[0].diverged, want[0].update_norm) == (1, 0, 2, 0.0) and want[1].diverged == 0
    got = _check(ieskf, cases, "nan", search)
    assert np.array_equal(got[0].state, pairs[0].state) and got[0].update_norm == 0.0


@pytest.mark.parametrize("search", SHAPES)
def test_rotations_outside_the_short_series_range(ieskf, oracle, cases, search):
    """(e) the accumulated q, or x_filter (-) x_lin, beyond tan(angle / 2) = 1 / 8: the libm forms of phi / Rinvleft
    (wave 1) and of boxMinus (wave 2) run, in some iterations and in one of the waves only.  (An increment dth beyond
    the range of axis2quat_fast, 1 rad in one step, is not something the oracle produces on these scans — the largest
    |dth| of its traces is 0.16 rad: the test below builds one.)"""
    prm, pairs, want, traces = cases["far"]
    q_ang, d_ang = [], []
    for p, w, tr in zip(pairs, want, traces):
        lin = tr["lin_state"][1:w.iters]  # the states the tail formed constants for
        q_ang.append(np.array([np.linalg.norm(oracle.quat2axis(s[6:10])) for s in lin]))
        d_ang.append(np.array([np.linalg.norm(oracle.box_minus(p.state, s)[6:9]) for s in lin]))
    assert q_ang[0].min() > FAST_QUAT2AXIS_ANGLE and d_ang[0].max() < FAST_QUAT2AXIS_ANGLE  # wave 1 libm, wave 2 series, always
    for k in (1, 2):  # wave 1 series; wave 2 series first, libm later
        assert q_ang[k].max() < FAST_QUAT2AXIS_ANGLE
        assert d_ang[k][0] < FAST_QUAT2AXIS_ANGLE < d_ang[k][-1]
    assert all(w.converged and not w.diverged for w in want)
    for p, w in zip(pairs, want):  # the reference's own error on these inputs: its two forms agree to 1e-12
        other = oracle.ieskf(prm, p, oracle.FORM_REDUCED, oracle.NN_KDTREE)
        assert other.iters == w.iters and np.abs(other.state - w.state).max() <= 1e-3 * TIGHT_STATE
    _check(ieskf, cases, "far", search)


@pytest.mark.parametrize("search", SHAPES)
def test_an_increment_beyond_one_radian_takes_the_libm_form_of_axis2quat(ieskf, oracle, cases, search):
    """(e) |dth| = 1.33 rad in every iteration of a hand-built pair: boxPlus on wave 0 leaves the range of axis2quat_fast
    (kFastHalfAngleSq: |dth| <= 1 rad) and takes libm's form; so do, from the q it gives, phi / Rinvleft and boxMinus.  The
    second increment is x_filter (-) x_lin of that q and is what update_norm reports: the update ends diverged by residual
    growth in its third iteration (|r| 0 -> 0.13) with the filter state."""
    prm, pairs, want, traces = cases["turn"]
    dth = np.linalg.norm(traces[0]["dx"][:want[0].iters, 6:9], axis=1)
    assert (want[0].iters, want[0].converged, want[0].diverged) == (3, 0, 1) and dth.min() > 1.0 and want[1].diverged == 0
    assert abs(want[0].update_norm - np.linalg.norm(traces[0]["dx"][1])) <= 1e-12 * want[0].update_norm
    other = oracle.ieskf(prm, pairs[0], oracle.FORM_REDUCED, oracle.NN_KDTREE)  # (the reference's own error on this input)
    assert other.iters == 3 and abs(other.update_norm - want[0].update_norm) <= 1e-3 * TIGHT_STATE
    got = _check(ieskf, cases, "turn", search)
    assert np.array_equal(got[0].state, pairs[0].state)


def test_an_update_cut_after_every_iteration_returns_the_whole_updates_bits(ieskf, cases, monkeypatch):
    """(f) the batch of (a) with a hand-over after every iteration (ten parts): the tail's results cross global memory nine
    times and come out as the uncut update's, and as the recorded ones."""
    prm, pairs, want, _ = cases["fixed"]
    whole, cut0 = _run_cut(ieskf, monkeypatch, prm, pairs, 0)
    assert cut0 == (1, 0)
    parts, cut = _run_cut(ieskf, monkeypatch, prm, pairs, 1, LINS_RELAY_CUTS=14, LINS_QUEUE_GRID=4)
    assert cut == (10, 0), cut
    for k, (a, b, w) in enumerate(zip(whole, parts, want)):
        _same_bits(a, b)
        _assert_tight(b, w, f"cut[{k}]")
    assert np.array_equal(np.array([r.state for r in parts]), np.load(GOLDEN)["state"])


def test_a_stop_rule_update_cut_after_every_iteration_ends_where_the_oracle_ends(ieskf, cases, monkeypatch):
    """(f) the stop-rule batch of (a) with a hand-over after every iteration: the launch has a part for each of the first
    fourteen iterations and one for the rest; after every hand-over the loop head decides on the convergence flag wave 3
    wrote whether this part finished the scan.  Every scan of the batch ends, by the oracle, before the last cut — so each
    of its iterations, the converging one included, is a part of its own — and comes out with the uncut update's bits and
    the oracle's iteration count."""
    prm, pairs, want, _ = cases["stop"]
    whole, cut0 = _run_cut(ieskf, monkeypatch, prm, pairs, 0)
    assert cut0 == (1, 0)
    parts, cut = _run_cut(ieskf, monkeypatch, prm, pairs, 1, LINS_RELAY_CUTS=14, LINS_QUEUE_GRID=2)
    assert cut == (_max_parts(prm.num_iter, 1, 14), 0) == (15, 0), cut
    assert all(w.converged and 1 < w.iters < cut[0] for w in want) and len({w.iters for w in want}) > 1
    for k, (a, b, w) in enumerate(zip(whole, parts, want)):
        _same_bits(a, b)
        assert b.iters == w.iters  # the part that met the stop rule was the scan's last
        _assert_tight(b, w, f"stop cut[{k}]")
