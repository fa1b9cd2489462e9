"""Scan-to-map on the device against the CPU oracle (oracle/map_oracle.cpp) round by round, in batches of any shape, at
the edges of the 27-cell search, for far and non-finite associated points, on both sides of the fits' thresholds, and
for what LINS_MAP_REUSE finds resident.  What the inputs are is asserted on the CPU (tests/test_map_rounds_inputs.py).

No number here comes from the device: records are compared bit for bit, transforms under the project's bar of 2e-5 (f64
sums added in another order, tests/test_gpu_map.py).  The per-round trace is the oracle's; the oracle's per-round
transforms are in turn held against the reference's own text on the CPU (they agree to the bit on these problems), and
the end result stays pinned to both as before."""
import importlib

import numpy as np
import pytest

import map_synth as ms

pytestmark = pytest.mark.gpu
defs = importlib.import_module("lins---lidar-inertial-slam_amd._ctypes_defs")
BAR = ms.SCAN2MAP_BAR


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def assert_records(g, w, what):
    """lins_map_corr records bit for bit; a rejected record of a rank-deficient fit carries NaN coefficients on both
    sides, and only there — and in the associated point of a query whose rotation overflowed — may the bits (a NaN's
    sign and payload) differ"""
    assert np.array_equal(g["ind"], w["ind"]), what
    assert np.array_equal(g["accepted"], w["accepted"]), what
    assert ((bits(g["sel"]) == bits(w["sel"])) | (np.isnan(g["sel"]) & np.isnan(w["sel"]))).all(), what  # (a NaN is a NaN)
    assert np.array_equal(bits(g["sq5"]), bits(w["sq5"])), what
    same = bits(g["coeff"]) == bits(w["coeff"])
    both_nan = np.isnan(g["coeff"]) & np.isnan(w["coeff"]) & (w["accepted"] == 0)[:, None]
    assert (same | both_nan).all(), what


def assert_result(g, w, what, exact=False):
    assert (g["iters"], g["converged"], g["degenerate"], g["n_sel"]) == (w["iters"], w["converged"], w["degenerate"], w["n_sel"]), (what, g, w)
    if exact:
        assert np.array_equal(bits(g["transform"]), bits(w["transform"])), (what, g, w)
    else:
        assert np.abs(g["transform"] - w["transform"]).max() <= BAR, (what, g, w)


def new_ctx(pkg, ieskf):
    return ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)


@pytest.fixture(scope="module")
def ctx(pkg, ieskf):
    c = new_ctx(pkg, ieskf)
    yield c
    c.close()


def at(p, transform):
    return defs.MapProblem(p.map_corner, p.map_surf, p.scan_corner, p.scan_surf, transform)


@pytest.fixture(scope="module")
def traces(oracle):
    return {name: (p,) + oracle.scan2map_trace(p) for name, p in ms.rounds_problems(defs).items()}


# ---- A. round by round --------------------------------------------------------------------------------------------
ROUND_PROBLEMS = ("room0", "room1", "room2", "room3", "room4", "room5", "corridor", "quick", "slow", "far", "far2", "floor", "floor50",
                  "below49", "few")


@pytest.mark.parametrize("name", ROUND_PROBLEMS)
def test_records_of_every_round_match_the_oracle(oracle, ctx, traces, name):
    """at the transform entering every round of the oracle's trace: the device's records bit for bit, and their rows
    summed on the host in f64 by the oracle's row formula are the oracle's 21 + 6 sums of that round"""
    p, _, rounds = traces[name]
    for r, tr in enumerate(rounds):
        pr = at(p, tr["t_in"])
        wc, ws = oracle.map_correspondences(pr)
        gc, gs = ctx.map_correspondences(pr)
        assert_records(gc, wc, (name, r, "corner"))
        assert_records(gs, ws, (name, r, "surf"))
        sums, n = oracle.map_sums(pr, gc, gs)
        assert n == tr["n_sel"] and np.array_equal(sums, tr["sums"]), (name, r)


def test_the_devices_own_rounds_match_the_trace(pkg, ieskf, traces):
    """lins_scan2map_batch stopped after r = 0 .. 10 rounds (lins_debug_map_rounds): transform, iters, converged,
    degenerate and n_sel are those of the trace's round min(r, rounds run).  Bar: 2e-5.  Measured on an MI355X: see
    1.06e-6 at most after any round of any of the fifteen problems (printed below)."""
    names = list(traces)
    assert tuple(names) == ROUND_PROBLEMS
    probs = [traces[n][0] for n in names]
    worst = (0.0, None)
    with new_ctx(pkg, ieskf) as c:
        for r in range(0, 11):
            c.debug_map_rounds(r)
            got = c.scan2map_batch(probs)
            for n, g in zip(names, got):
                p, _, rounds = traces[n]
                k = min(r, len(rounds))
                if k == 0:
                    w = dict(transform=p.transform, iters=0, converged=0, degenerate=0, n_sel=0)
                else:
                    t = rounds[k - 1]
                    w = dict(transform=t["t_out"], iters=k, converged=t["converged"], degenerate=t["degenerate"], n_sel=t["n_sel"])
                d = float(np.abs(g["transform"] - w["transform"]).max())
                if d > worst[0]:
                    worst = (d, (n, r))
                print("rounds=%d %s: |dT| = %.3g" % (r, n, d))
                assert_result(g, w, (n, r))
            assert c.map_stats()[1] == sum(g["iters"] * (len(p.scan_corner) + len(p.scan_surf)) for g, p in zip(got, probs))
        print("largest per-round transform difference: %.3g at %s" % worst)
        c.debug_map_rounds(10)
        for n, g in zip(names, c.scan2map_batch(probs)):
            assert_result(g, traces[n][1], n)
        with pytest.raises(ieskf.LinsError):
            c.debug_map_rounds(11)


# ---- B. batch shape and independence --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(pkg, ieskf, oracle):
    """kind -> (problem, the problem run alone in a fresh context, the oracle's result)"""
    out = {}
    for kind, p in ms.batch_pool(defs).items():
        with new_ctx(pkg, ieskf) as c:
            out[kind] = (p, c.scan2map_batch([p])[0], oracle.scan2map(p))
    return out


@pytest.mark.parametrize("order", ["first", "second"])
def test_a_problems_bits_do_not_depend_on_its_batch(pkg, ieskf, pool, order):
    """batches of 1, 7, 8, 9, 16, 19 and 33 problems of very uneven query counts, inactive and early-converging ones
    interleaved: every problem's result is, bit for bit, that of the problem alone in a fresh context, whatever its
    position and its batch mates, and the oracle's under the bar; the query count is rounds x queries"""
    for kind, (p, alone, want) in pool.items():
        assert_result(alone, want, kind)
    with new_ctx(pkg, ieskf) as c:
        for kinds in ms.batch_orders()[order]:
            got = c.scan2map_batch([pool[k][0] for k in kinds])
            assert len(got) == len(kinds)
            for i, (k, g) in enumerate(zip(kinds, got)):
                assert_result(g, pool[k][1], (order, len(kinds), i, k), exact=True)
                assert_result(g, pool[k][2], (order, len(kinds), i, k))
            nq = c.map_stats()[1]
            assert nq == sum(g["iters"] * (len(pool[k][0].scan_corner) + len(pool[k][0].scan_surf)) for k, g in zip(kinds, got))


# ---- C. lattice and box edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform", [None, ms.LATTICE_T], ids=["identity", "moved"])
def test_lattice_and_box_edges_match_the_oracle(oracle, ctx, transform):
    """hand-built maps at the edges of the 27-cell search (tests/map_synth.py lattice_cases): the oracle's search is
    exhaustive and knows no grid; its records say the case is what it claims, the device's are the same bits"""
    for name, (p, claims) in ms.lattice_cases(defs, transform).items():
        wc, ws = oracle.map_correspondences(p)
        ms.check_lattice_claims(p, claims, ws, exact=transform is None)
        gc, gs = ctx.map_correspondences(p)
        assert_records(gc, wc, (name, "corner"))
        assert_records(gs, ws, (name, "surf"))


# ---- D. far and non-finite associated points -----------------------------------------------------------------------
FAR = (1e3, 1e6, 1e10, 3e38)


def test_far_queries_get_no_neighbours_and_leave_the_others_alone(oracle, ctx):
    """queries 1e3 .. 3e38 m from the map (the device clamps the associated point before it takes its cell,
    include/lins_map.h): ind = -1, accepted = 0, sq5 = inf like the oracle, the other queries' records unchanged"""
    p, _ = ms.make_problem(defs, 64, n_map_surf=6000, n_map_corner=900, n_scan_surf=400, n_scan_corner=120)
    bc, bs = ctx.map_correspondences(p)
    sc, ss = p.scan_corner.copy(), p.scan_surf.copy()
    moved_c, moved_s = [], []
    for k, far in enumerate(FAR):
        for axis in range(3):
            for sign in (-1.0, 1.0):
                i = 6 * k + 2 * axis + int(sign > 0)
                ss[i, axis], sc[i, axis] = sign * far, sign * far
                moved_s.append(i), moved_c.append(i)
    ss[30, :3], sc[30, :3] = 3e38, -3e38  # (every coordinate: the rotation overflows, the associated point is inf or NaN)
    moved_s.append(30), moved_c.append(30)
    q = defs.MapProblem(p.map_corner, p.map_surf, sc, ss, p.transform)
    wc, ws = oracle.map_correspondences(q)
    gc, gs = ctx.map_correspondences(q)
    for g, w, b, moved, what in ((gc, wc, bc, moved_c, "corner"), (gs, ws, bs, moved_s, "surf")):
        assert_records(g, w, what)
        assert (g["ind"][moved] == -1).all() and not g["accepted"][moved].any() and np.isinf(g["sq5"][moved]).all()
        keep = np.setdiff1d(np.arange(len(g)), moved)
        assert g[keep].tobytes() == b[keep].tobytes()
    # the same through the rounds, in a batch with an untouched neighbour on either side
    got = ctx.scan2map_batch([p, q, p])
    assert_result(got[0], oracle.scan2map(p), "neighbour")
    assert_result(got[1], oracle.scan2map(q), "far queries")
    assert_result(got[2], got[0], "neighbours agree", exact=True)
    # a huge but finite transform: every associated point is far away
    t = p.transform.copy()
    t[3] = 1e30
    far_t = at(p, t)
    wc, ws = oracle.map_correspondences(far_t)
    gc, gs = ctx.map_correspondences(far_t)
    assert_records(gc, wc, "corner, far transform"), assert_records(gs, ws, "surf, far transform")
    assert (gs["ind"] == -1).all() and (gc["ind"] == -1).all()
    assert_result(ctx.scan2map_batch([far_t])[0], oracle.scan2map(far_t), "far transform")


def test_inputs_outside_the_contract_are_input_errors(ieskf, oracle, ctx):
    """a non-finite transform or scan point is LINS_E_INPUT (-4) from both calls, in any position of a batch; the context
    is usable afterwards and gives the answers it gave before"""
    p, _ = ms.make_problem(defs, 65, n_map_surf=6000, n_map_corner=900, n_scan_surf=300, n_scan_corner=80)
    before = ctx.scan2map_batch([p])[0]
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        for i in (0, 5):
            t = p.transform.copy()
            t[i] = v
            bad.append(at(p, t))
        s = p.scan_surf.copy()
        s[7, 2] = v
        bad.append(defs.MapProblem(p.map_corner, p.map_surf, p.scan_corner, s, p.transform))
        s = p.scan_corner.copy()
        s[3, 0] = v
        bad.append(defs.MapProblem(p.map_corner, p.map_surf, s, p.scan_surf, p.transform))
    for b in bad:
        with pytest.raises(ieskf.LinsError, match="-4"):
            ctx.map_correspondences(b)
        with pytest.raises(ieskf.LinsError, match="-4"):
            ctx.scan2map_batch([p, b])
        with pytest.raises(ieskf.LinsError, match="-4"):
            ctx.scan2map_batch([b, p, p])
    assert_result(ctx.scan2map_batch([p])[0], before, "after the errors", exact=True)
    assert_result(before, oracle.scan2map(p), "oracle")


# ---- E. fit thresholds -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sigma_0", "sigma_0.02", "sigma_0.05", "sigma_0.1", "sigma_0.2", "shapes"])
def test_both_sides_of_the_fit_thresholds_match_the_oracle(oracle, ctx, name):
    """the noise sweep and the shaped neighbourhoods whose branch populations tests/test_map_rounds_inputs.py asserts"""
    p = ms.threshold_sweep(defs)[name]
    wc, ws = oracle.map_correspondences(p)
    gc, gs = ctx.map_correspondences(p)
    assert_records(gc, wc, (name, "corner"))
    assert_records(gs, ws, (name, "surf"))


# ---- F. what is resident --------------------------------------------------------------------------------------------
def hide_maps(p):
    """the problem with LINS_MAP_REUSE set and map arrays that must not be read (NaN: an input error if they were)"""
    q = defs.MapProblem(np.full_like(p.map_corner, np.nan), np.full_like(p.map_surf, np.nan), p.scan_corner, p.scan_surf, p.transform)
    q.reuse_resident_map = True
    return q


def flag_only(p):
    q = at(p, p.transform)
    q.reuse_resident_map = True
    return q


def test_reuse_after_a_correspondence_call(pkg, ieskf):
    """lins_map_correspondences leaves its problem's maps resident as a batch of one: a LINS_MAP_REUSE batch of one runs
    on them; a LINS_MAP_REUSE batch of two does not fit what is resident and uploads afresh"""
    a, b = ms.make_problem(defs, 70)[0], ms.make_problem(defs, 71)[0]
    with new_ctx(pkg, ieskf) as c:
        fresh = c.scan2map_batch([a, b])
    with new_ctx(pkg, ieskf) as c:
        c.map_correspondences(a)
        assert_result(c.scan2map_batch([hide_maps(a)])[0], fresh[0], "reuse after correspondences", exact=True)
        rc, rs = c.map_correspondences(hide_maps(a))  # and the other way round
        with new_ctx(pkg, ieskf) as d:
            wc, ws = d.map_correspondences(a)
        assert rc.tobytes() == wc.tobytes() and rs.tobytes() == ws.tobytes()
        got = c.scan2map_batch([flag_only(a), flag_only(b)])  # one problem resident, two asked for: fallback
        assert_result(got[0], fresh[0], "fallback 0", exact=True), assert_result(got[1], fresh[1], "fallback 1", exact=True)
        # same count, maps of other sizes than the resident ones: fallback
        other = ms.make_problem(defs, 72, n_map_surf=5000)[0]
        with new_ctx(pkg, ieskf) as d:
            want = d.scan2map_batch([other, b])
        got = c.scan2map_batch([flag_only(other), flag_only(b)])
        assert_result(got[0], want[0], "fallback sizes 0", exact=True), assert_result(got[1], want[1], "fallback sizes 1", exact=True)


def test_reuse_after_a_failed_call(pkg, ieskf):
    """a call that returns LINS_E_INPUT — from a map cloud, from a scan cloud after the new maps went up or with the
    resident ones in use, from the transform — leaves nothing resident (include/lins_map.h), so it never leaves descriptors of maps that are not on the device: a LINS_MAP_REUSE call behind it gives the bits
    of a fresh upload of its own maps"""
    a, b = ms.make_problem(defs, 73)[0], ms.make_problem(defs, 74)[0]  # (same cloud sizes, other clouds)
    with new_ctx(pkg, ieskf) as c:
        fresh_a, fresh_b = c.scan2map_batch([a])[0], c.scan2map_batch([b])[0]
    assert not np.array_equal(fresh_a["transform"], fresh_b["transform"])
    bad_map = at(b, b.transform)
    bad_map.map_surf = b.map_surf.copy()
    bad_map.map_surf[11, 0] = np.nan
    bad_scan = at(b, b.transform)
    bad_scan.scan_surf = b.scan_surf.copy()
    bad_scan.scan_surf[11, 0] = np.nan
    bad_scan_reusing = at(b, b.transform)  # (sizes match what is resident: fails on the scan with a's maps in use)
    bad_scan_reusing.scan_surf, bad_scan_reusing.reuse_resident_map = bad_scan.scan_surf, True
    bad_t = at(b, np.full(6, np.nan, np.float32))
    for what, bad in (("map", bad_map), ("scan", bad_scan), ("scan, reusing", bad_scan_reusing), ("transform", bad_t)):
        with new_ctx(pkg, ieskf) as c:
            assert_result(c.scan2map_batch([a])[0], fresh_a, what, exact=True)  # a's maps are resident
            with pytest.raises(ieskf.LinsError, match="-4"):
                c.scan2map_batch([bad])
            # b's maps with the flag: whatever is resident now, the answer is b's (real arrays: a fallback may read them)
            assert_result(c.scan2map_batch([flag_only(b)])[0], fresh_b, (what, "b"), exact=True)
            with pytest.raises(ieskf.LinsError, match="-4"):
                c.scan2map_batch([bad])
            # and a's with the flag (the sizes match whatever a failed call left): a's answer, not b's
            assert_result(c.scan2map_batch([flag_only(a)])[0], fresh_a, (what, "a"), exact=True)
            assert_result(c.scan2map_batch([hide_maps(a)])[0], fresh_a, (what, "a, resident"), exact=True)


def test_reuse_after_a_local_map_batch(pkg, ieskf):
    """a LINS_MAP_LOCAL batch leaves the built maps resident: a LINS_MAP_REUSE batch of the same size with the downloaded
    clouds' sizes runs on them (map arrays not read); one of another size uploads afresh"""
    from local_map_synth import room_scan, trajectory

    poses = trajectory(12, seed=4)
    with new_ctx(pkg, ieskf) as c:
        c.local_map_init(2, 50, 8192)
        fills = [10, 4]
        for s, f in enumerate(fills):
            for i in range(f):
                c.local_map_push(s, *(room_scan(100 * s + i, poses[i], n_corner=300, n_surf=2500, n_outlier=100) + (poses[i],)))
        truth = [poses[f - 1] + np.array([0.05, 0.03, 0.0, 0.0, 0.0, 0.01], np.float32) for f in fills]
        scans = [room_scan(500 + s, truth[s], n_corner=470, n_surf=6000, n_outlier=200) for s in range(2)]
        sizes = c.local_map_build([0, 1], scans)
        assert all(s["status"] == 0 for s in sizes)
        t0 = [np.array([p[3], p[4], p[5], p[0], p[1], p[2]], np.float32) for p in poses[[f - 1 for f in fills]]]
        local = c.scan2map_batch([defs.MapProblem.local(t) for t in t0])
        explicit = []
        for k in range(2):
            cl = [c.local_map_download(k, w) for w in range(6)]
            explicit.append(defs.MapProblem(cl[0], cl[1], cl[2], cl[5], t0[k]))
        with new_ctx(pkg, ieskf) as d:
            fresh = d.scan2map_batch(explicit)
            fresh_one = d.scan2map_batch(explicit[1:])
        assert local[0]["iters"] > 0
        for k in range(2):
            assert_result(local[k], fresh[k], ("local", k), exact=True)
        got = c.scan2map_batch([hide_maps(p) for p in explicit])  # same size: the built maps, where they were gridded
        for k in range(2):
            assert_result(got[k], fresh[k], ("reuse after local", k), exact=True)
        c.scan2map_batch([defs.MapProblem.local(t) for t in t0])
        got = c.scan2map_batch([flag_only(explicit[1])])  # another size: problem 1 is not what lies at index 0
        assert_result(got[0], fresh_one[0], "another size after local", exact=True)
