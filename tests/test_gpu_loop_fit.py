"""The loop-closure ICP's fit and stop step on the device, on built sums (tests/loop_fit_cases.py): every case through the
real step kernel (lins_debug_loop_icp_step: caller-given tile partials, launch_loop_step, the states read back) against
the CPU restatement's step within 2 x bar_R — both are within bar_R of the exact reference — and against the reference
itself; bit for bit where the arithmetic is exact; every stop comparison at equality; batch and tile independence; and
two cases end to end through lins_loop_icp_batch, which ties the search kernel's sums to the built ones.
tests/test_loop_fit_inputs.py asserts what the cases claim and runs the same checks on the CPU."""
import importlib
import time

import numpy as np
import pytest

import loop_fit_cases as fc
import loop_icp_np as lnp

pytestmark = pytest.mark.gpu
host = importlib.import_module("lins---lidar-inertial-slam_amd.host")
PAD = 6  # tiles a batch: the widest case has 5, the rest is NaN no kernel may read
FIELDS = ("mse_prev", "mse", "fitness", "iterations", "converged", "reason", "n_corr", "n_fitness", "active")


def state_bits(st):
    return (st["T"].tobytes(), st["move"].tobytes()) + tuple(np.float64(st[k]).tobytes() if isinstance(st[k], float) else st[k] for k in FIELDS)


@pytest.fixture(scope="module")
def ctx(pkg, ieskf):
    t0 = time.perf_counter()
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    yield c
    c.close()
    print(f"\ntests/test_gpu_loop_fit.py: {time.perf_counter() - t0:.2f} s from context creation to the last test")


def partials_of(c, tiles=None):
    p = fc.split(c["X"], c["G"], tiles or c["tiles"], pad=PAD - (tiles or c["tiles"]))
    return p, tiles or c["tiles"]


def run_cases(ctx, cs, **kw):
    parts = [partials_of(c) for c in cs]
    return ctx.debug_loop_icp_step(np.stack([p for p, _ in parts]), n_tiles=[t for _, t in parts], **kw)


@pytest.fixture(scope="module")
def device_states(ctx):
    """every case in one call, each over its own tile count"""
    states, running = run_cases(ctx, fc.fit_cases())
    assert running == sum(s["active"] for s in states)
    return states


def test_every_case_against_the_host_and_the_reference(device_states):
    worst_host, worst_ref = (0.0, ""), (0.0, "")
    for c, st in zip(fc.fit_cases(), device_states):
        # the host's step over the same partials added in tile order, as the kernel adds them
        p, tiles = partials_of(c)
        v = np.zeros(17)
        for b in range(tiles):
            v = v + p[b]
        hs, _, _ = host.loop_icp_step(v)
        assert all(st[k] == hs[k] for k in ("iterations", "converged", "reason", "n_corr", "active")) and st["mse"] == hs["mse"], (c["name"], st, hs)
        diff = np.linalg.norm(st["T"][:3, :3] - hs["T"][:3, :3])
        if fc.determined(c):
            assert diff <= 2 * fc.bar_R(c["ref"]) and np.linalg.norm(st["T"][:3, 3] - hs["T"][:3, 3]) <= 2 * fc.bar_t(c["ref"]), (c["name"], diff)
            worst_host = max(worst_host, (diff / (2 * fc.bar_R(c["ref"])), c["name"]))
        if c["exact"] or not fc.determined(c):
            assert state_bits(st) == state_bits(hs), c["name"]
        print(f"{c['name']}: device - host |dR| = {diff:.2e}, |dt| = {np.linalg.norm(st['T'][:3, 3] - hs['T'][:3, 3]):.2e}")
        ratio, _ = fc.check_fit(dict(c, sums=v), st, "device")
        worst_ref = max(worst_ref, (ratio, c["name"]))
    print(f"device against the host: worst |dR| / (2 bar_R) = {worst_host[0]:.3f} at {worst_host[1]}")
    print(f"device against the reference: worst |dR| / bar_R = {worst_ref[0]:.3f} at {worst_ref[1]}")


def test_every_stop_comparison_at_equality(ctx):
    for edge in fc.stop_edges():
        name, v, kw, st_in, reason = edge
        p = np.stack([v / 2, v / 2] + [np.full(17, np.nan)] * 2)[None]  # (two tiles: halves of dyadic sums are exact)
        (st,), running = ctx.debug_loop_icp_step(p, host.loop_icp_params(**kw), states=[st_in], n_tiles=[2])
        fc.check_stop_edge(edge, st, "device")
        hs, _, _ = host.loop_icp_step(v, host.loop_icp_params(**kw), state=st_in)
        assert state_bits(st) == state_bits(hs) and running == st["active"], name


def test_fitness_mode(ctx):
    v, v3 = fc.stop_sums(0.25), fc.stop_sums(0.25)
    v3[0], v3[16] = 3.0, 1.0
    gone = dict(T=fc.T_IN, active=0, iterations=7, mse=0.125, mse_prev=0.125)
    states, _ = ctx.debug_loop_icp_step(np.stack([v, v3, np.zeros(17), v])[:, None, :], mode=1, states=[gone, None, None, None], status=[0, 0, 0, -3])
    assert (states[0]["fitness"], states[0]["n_fitness"], states[0]["iterations"], states[0]["active"]) == (0.25, 8, 7, 0)
    assert states[0]["T"].tobytes() == fc.T_IN.tobytes()
    assert states[1]["fitness"] == 1.0 / 3.0 and (states[2]["fitness"], states[2]["n_fitness"]) == (lnp.DBL_MAX, 0)
    assert (states[3]["fitness"], states[3]["n_fitness"]) == (lnp.DBL_MAX, 0)  # a problem with a status is not run


def test_a_cases_bits_do_not_depend_on_its_batch(ctx, device_states):
    cs = fc.fit_cases()
    alone = {c["name"]: state_bits(s) for c, s in zip(cs, device_states)}
    gone = dict(T=fc.T_IN, active=0, iterations=7, mse=0.125, mse_prev=0.375, fitness=0.5, reason=lnp.ABS_MSE, converged=1, n_corr=5, n_fitness=4)
    failed = dict(T=fc.T_IN, iterations=2, mse=0.25, mse_prev=0.25, n_corr=9)
    order_a = list(range(len(cs)))[::-1]
    order_b = list(np.random.default_rng(1).permutation(len(cs)))
    for order in (order_a, order_b):
        # the cases in this order, with a stopped problem and one with a status (live sums under both) put among them
        slots = [("case", k) for k in order]
        slots.insert(3, ("gone", order[0]))
        slots.insert(9, ("failed", order[1]))
        slots.append(("gone", order[2]))
        assert len(slots) > 8
        parts = [partials_of(cs[k]) for _, k in slots]
        states, running = ctx.debug_loop_icp_step(np.stack([p for p, _ in parts]), n_tiles=[t for _, t in parts],
                                                  states=[dict(case=None, gone=gone, failed=failed)[w] for w, _ in slots],
                                                  status=[-3 if w == "failed" else 0 for w, _ in slots])
        live = 0
        for (w, k), st in zip(slots, states):
            if w == "case":
                assert state_bits(st) == alone[cs[k]["name"]], (cs[k]["name"], w)
                live += st["active"]
            else:  # untouched
                src = gone if w == "gone" else failed
                assert st["T"].tobytes() == fc.T_IN.tobytes() and all(st[f] == src.get(f, dict(fitness=lnp.DBL_MAX, active=1).get(f, 0)) for f in FIELDS), (w, st)
        assert running == live


def test_the_tiling_of_the_sums(ctx):
    """the same pairs over 1, 2 and 5 tiles: the same counts and reason, T within the bar of the reference; the same bits
    where the sums are dyadic.  The tiles behind a problem's own are NaN: the kernel's tile loop ends where it should."""
    cs = [c for c in fc.fit_cases() if c["dyadic"] or c["name"] in ("rotations/yaw2", "rotations/generic120", "far_origin/1000", "three_points")]
    res = {}
    for tiles in (1, 2, 5):
        parts = [partials_of(c, min(tiles, len(c["X"]))) for c in cs]
        res[tiles], _ = ctx.debug_loop_icp_step(np.stack([p for p, _ in parts]), n_tiles=[t for _, t in parts])
    for k, c in enumerate(cs):
        for tiles in (1, 2, 5):
            st = res[tiles][k]
            assert np.isfinite(st["T"]).all() and (st["n_corr"], st["reason"]) == (res[1][k]["n_corr"], res[1][k]["reason"]), (c["name"], tiles)
            fc.check_fit(c, dict(st, mse=c["sums"][16] / c["sums"][0], mse_prev=c["sums"][16] / c["sums"][0]), f"{tiles} tiles")
            if c["dyadic"]:
                assert st["T"].tobytes() == res[1][k]["T"].tobytes(), (c["name"], tiles)


@pytest.mark.parametrize("pairs", [fc.mirror_pairs, fc.planar_pairs], ids=["mirror", "planar"])
def test_the_search_kernels_sums_are_the_built_ones(ctx, pairs):
    """one round of the public entry (nearest-neighbour pairing is the identity pairing, tests/test_loop_fit_inputs.py) at 31,
    32 and 33 source points — either side of one tile — against the step on the sums numpy forms of the same pairs"""
    ctx.debug_loop_icp_rounds(1)
    try:
        for n in (31, 32, 33):
            X, G = pairs(n)
            z = np.zeros((n, 1), np.float32)
            got = ctx.loop_icp([(np.concatenate([X, z], 1), np.concatenate([G, z], 1))])[0]
            c = fc.case(f"{pairs.__name__}/{n}", X, G, rank=3 if pairs is fc.mirror_pairs else 2)
            c.update(ref=fc.reference(X, G), sums=fc.sums(X, G))
            (st,), _ = ctx.debug_loop_icp_step(fc.split(X, G, 2 if n > 32 else 1)[None])
            assert (got["status"], got["iterations"], got["n_corr"], got["reason"], got["n_fitness"]) == (0, 1, n, st["reason"], n), got
            if pairs is fc.mirror_pairs:  # dyadic: every sum exact in any order
                assert got["transform"].tobytes() == st["T"].tobytes() and got["mse"] == st["mse"], n
            r = c["ref"]
            assert np.linalg.norm(got["transform"][:3, :3] - st["T"][:3, :3]) <= 2 * fc.bar_R(r)
            assert np.linalg.norm(got["transform"][:3, 3] - st["T"][:3, 3]) <= 2 * fc.bar_t(r)
            assert abs(got["mse"] - st["mse"]) <= 4 * fc.U53 * st["mse"]
            fc.check_fit(c, dict(st, T=got["transform"], move=got["transform"][:3].astype(np.float32)), "end to end")
    finally:
        ctx.debug_loop_icp_rounds(0)
