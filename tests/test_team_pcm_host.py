"""lins_host_team_factors_consistent and lins_host_team_pcm_clique (include/lins_host.h; the scalar text
csrc/host/team_pcm.h) against the independent checker of tests/team_pcm_np.py: every case of tests/team_pcm_cases.py —
mask, counts, exact, nodes_max —, seeded random graphs of 64 vertices, the mask's independence of a member's root, and
every refusal.

Nothing near a threshold is compared across the two arithmetics: the cases' pairs lie well inside or well outside the
bars, and for the planted case (and its rebased copy) the checker alone first shows every kept pair within HALF the bars and
every inlier-outlier pair beyond TWICE a bar.  The bar itself and one nextafter beyond it belong to the native program
(tests/test_team_pcm_sanitized.py), which uses the text's own arithmetic."""
import importlib

import numpy as np
import pytest

import pose_graph_cases as pgc
import pose_graph_np as pnp
import team_pcm_cases as tpc
import team_pcm_np as tpn

host = importlib.import_module("lins---lidar-inertial-slam_amd.host")
defs = importlib.import_module("lins---lidar-inertial-slam_amd._ctypes_defs")

E_ARG, E_CAPACITY, E_INPUT = -1, -3, -4  # include/lins_ieskf.h
CASES = tpc.cases()


def graphs(members):
    gs = [host.PoseGraph(len(c["aft"]), 1) for c in members]
    for g, c in zip(gs, members):
        pgc.fill(g, c)
    return gs


def poses_of(gs, factors):
    T = [g.poses_f64() for g in gs]
    Tb = np.array([T[f[0]][f[1]] for f in factors]).reshape(-1, 12)
    Ta = np.array([T[f[2]][f[3]] for f in factors]).reshape(-1, 12)
    return Tb, Ta


_CHECKED = {}


def checked(c):
    """the checker's record of a case, computed once"""
    if c["name"] not in _CHECKED:
        Tb, Ta = poses_of(graphs(c["members"]), c["factors"])
        _CHECKED[c["name"]] = tpn.evaluate(c["factors"], Tb, Ta, **c["params"])
    return _CHECKED[c["name"]]


def test_defaults_and_record_sizes():
    import ctypes as C

    p = host.team_pcm_params()
    assert (p.max_translation, p.min_cos_rotation, p.translation_per_frame, p.min_support, p.max_nodes) == (
        1.0, tpn.DEFAULTS["min_cos_rotation"], 0.0, 3, 65536)
    assert C.sizeof(defs.TeamPcmResultC) == 32 and C.sizeof(defs.TeamPcmParamsC) == 32 and defs.TEAM_PCM_MAX_FACTORS == 64
    assert abs(np.degrees(np.arccos(p.min_cos_rotation)) - 5.0) < 1e-12


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_case_against_the_checker(c):
    want = checked(c)
    for k, v in c["want"].items():  # what the issue states outright: the checker reproduces it, or the text is not the definition
        assert want[k] == v, (k, want[k], v)
    got = host.team_factors_consistent_graphs(graphs(c["members"]), c["factors"], **c["params"])
    assert got == want


def margins(recs, prm, inliers, outliers):
    """(the largest share of a bar among the inlier pairs, the smallest multiple of a bar that separates an inlier from an
    outlier): rotation as an angle against arccos(min_cos), translation against the pair's own t"""
    rot_bar = np.arccos(prm["min_cos_rotation"])
    inside, outside = 0.0, np.inf
    for i, l in enumerate(inliers):
        for m in inliers[i + 1:]:
            a, b = recs[l], recs[m]
            inside = max(inside, tpn.angle(a, b) / rot_bar, tpn.apart(a, b) / tpn.bar(a, b, prm))
        for m in outliers:
            a, b = recs[l], recs[m]
            outside = min(outside, max(tpn.angle(a, b) / rot_bar, tpn.apart(a, b) / tpn.bar(a, b, prm)))
    return inside, outside


def test_planted_outliers_and_root_independence():
    """11 and 10: exactly the inliers are kept; then member 1's graph is rebased by a 7 m / 26 degree X and the mask is the
    same.  First, by the checker alone, before and after the rebase: every kept pair within half the bars, every
    inlier-outlier pair beyond twice a bar."""
    c = tpc.planted()
    gs = graphs(c["members"])
    X = np.eye(4)
    X[:3, :3] = pnp.rot_axis(1, np.deg2rad(26.0))  # (the archive's vertical axis is 1)
    X[:3, 3] = [4.0, -1.0, 5.657]
    assert abs(np.linalg.norm(X[:3, 3]) - 7.0) < 0.01
    results = []
    for rebased in (False, True):
        if rebased:
            assert gs[1].rebase(X) == 0
        Tb, Ta = poses_of(gs, c["factors"])
        inside, outside = margins(tpn.records(c["factors"], Tb, Ta), tpn.DEFAULTS, tpc.PLANTED_INLIERS, tpc.PLANTED_OUTLIERS)
        print("planted%s: inlier pairs within %.3f of a bar, inlier-outlier pairs beyond %.2f of a bar" % (" (rebased)" if rebased else "", inside, outside))
        assert inside <= 0.5 and outside >= 2.0
        want = tpn.evaluate(c["factors"], Tb, Ta)
        got = host.team_factors_consistent(c["factors"], Tb, Ta)
        assert got == want and got["kept"] == tpc.PLANTED_INLIERS and (got["n_pairs"], got["n_pairs_kept"], got["exact"]) == (1, 1, 1)
        results.append(got)
    assert results[0] == results[1]
    moved = np.abs(gs[1].poses_f64() - graphs(c["members"])[1].poses_f64()).max()
    assert moved > 3.0  # (the rebase did move the member)


def rows(adj):
    return np.array(adj, np.uint64)


@pytest.mark.parametrize("seed,density", tpc.RANDOM_GRAPHS)
def test_clique_on_random_graphs(seed, density):
    adj = tpc.random_graph(seed, density)
    want = tpn.clique(adj, [0] * 64, dict(tpn.DEFAULTS, min_support=1))
    print("seed %d density %.1f: clique of %d, at most %d nodes a subproblem" % (seed, density, want["n_kept"], want["nodes_max"]))
    assert want["exact"] == 1 and want["nodes_max"] <= 65536
    assert host.team_pcm_clique(rows(adj), min_support=1) == want
    # a budget one node short of the costliest subproblem: both stop there with the same best so far
    short = tpn.clique(adj, [0] * 64, dict(tpn.DEFAULTS, min_support=1, max_nodes=want["nodes_max"] - 1))
    assert short["exact"] == 0 and host.team_pcm_clique(rows(adj), min_support=1, max_nodes=want["nodes_max"] - 1) == short


def test_clique_keeps_pairs_apart():
    """two keys: the even vertices a triangle plus a pendant, the odd ones a path — per key its own winner"""
    n = 9
    edges = [(0, 2), (0, 4), (2, 4), (4, 6), (1, 3), (3, 5), (5, 7)]
    adj = [0] * n
    for a, b in edges:
        adj[a] |= 1 << b
        adj[b] |= 1 << a
    pair = [7 if v % 2 == 0 else -3 for v in range(n)]
    want = tpn.clique(adj, pair, dict(tpn.DEFAULTS, min_support=2))
    assert want["kept"] == [0, 1, 2, 3, 4] and (want["n_pairs"], want["n_pairs_kept"]) == (2, 2)
    assert host.team_pcm_clique(rows(adj), pair, min_support=2) == want
    assert host.team_pcm_clique(rows(adj), pair)["kept"] == [0, 2, 4]


def untouched():
    out = defs.TeamPcmResultC(71, 72, 73, 74, 75, 76)
    out.kept[0], out.kept[1] = 77, 78
    return out


def is_untouched(out):
    return (out.n_factors, out.n_kept, out.n_pairs, out.n_pairs_kept, out.exact, out.nodes_max, out.kept[0], out.kept[1]) == (71, 72, 73, 74, 75, 76, 77, 78)


def test_refusals_write_nothing():
    import ctypes as C

    c = tpc.planted()
    Tb, Ta = poses_of(graphs(c["members"]), c["factors"])
    fs = c["factors"]
    out = untouched()

    def refused(factors=fs, tb=Tb, ta=Ta, **kw):
        rc = host.team_factors_consistent(factors, tb, ta, out=out, **kw)
        assert is_untouched(out), kw
        return rc

    def with_(i, **kw):
        f = dict(zip(("slot_b", "id_b", "slot_a", "id_a", "Z", "var"), fs[i]))
        f.update(kw)
        return list(fs[:i]) + [f] + list(fs[i + 1:])

    for kw in (dict(max_translation=-1.0), dict(max_translation=np.nan), dict(max_translation=np.inf), dict(min_cos_rotation=np.nan),
               dict(translation_per_frame=-1e-9), dict(translation_per_frame=np.nan), dict(translation_per_frame=np.inf), dict(min_support=0),
               dict(max_nodes=0), dict(max_nodes=-5)):
        assert refused(**kw) == E_ARG, kw
    for kw in (dict(slot_a=0), dict(slot_b=1, slot_a=1), dict(slot_b=-1), dict(slot_a=-2), dict(id_b=-1), dict(id_a=-1)):
        assert refused(with_(0, **kw)) == E_ARG, kw
    assert host.team_factors_consistent(fs, Tb, Ta, n_factors=-1, out=out) == E_ARG and is_untouched(out)
    # null pointers, through the C call itself
    L, prm = host.lib(), host.team_pcm_params()
    farr = (defs.TeamFactorC * len(fs))(*[defs.team_factor(f) for f in fs])
    for args in ((len(fs), None, Tb.ctypes.data, Ta.ctypes.data, C.byref(prm), C.byref(out)),
                 (len(fs), farr, None, Ta.ctypes.data, C.byref(prm), C.byref(out)),
                 (len(fs), farr, Tb.ctypes.data, None, C.byref(prm), C.byref(out)),
                 (len(fs), farr, Tb.ctypes.data, Ta.ctypes.data, None, C.byref(out)),
                 (len(fs), farr, Tb.ctypes.data, Ta.ctypes.data, C.byref(prm), None)):
        assert L.lins_host_team_factors_consistent(*args) == E_ARG and is_untouched(out)
    # inputs the solve would refuse, and poses that are not finite
    Z = np.array(fs[3][4])
    nan_z, inf_t, skew = Z.copy(), Z.copy(), Z.copy()
    nan_z[4], inf_t[10], skew[0] = np.nan, np.inf, Z[0] + 1e-6
    for kw in (dict(Z=nan_z), dict(Z=inf_t), dict(Z=skew), dict(var=0.0), dict(var=-1.0), dict(var=np.nan), dict(var=np.inf)):
        assert refused(with_(3, **kw)) == E_INPUT, kw
    for which, j, bad in ((0, 2, np.nan), (1, 11, np.inf), (0, 9, -np.inf)):
        T = [Tb.copy(), Ta.copy()]
        T[which][5, j] = bad
        assert refused(tb=T[0], ta=T[1]) == E_INPUT, (which, j)
    # 64 factors are taken, 65 are not
    m = tpc.pair_members(70)
    many = [tpc.near(m, i, i) for i in range(65)]
    tb, ta = poses_of(graphs(m), many)
    assert refused(many, tb, ta) == E_CAPACITY
    assert host.team_factors_consistent(many[:64], tb[:64], ta[:64])["n_kept"] == 64
    # usable behind the refusals
    assert host.team_factors_consistent(fs, Tb, Ta)["kept"] == tpc.PLANTED_INLIERS


def test_clique_refusals_write_nothing():
    out = untouched()
    tri = [0b110, 0b101, 0b011]
    assert host.team_pcm_clique(rows(tri), min_support=1)["kept"] == [0, 1, 2]
    for adj, pair in (([0b010, 0b000], None),         # not symmetric
                      ([0b011, 0b001], None),         # its own neighbour
                      ([0b110, 0b001, 0b000], None),  # a bit beyond n ... (row 0 names vertex 2, which names nobody)
                      ([0b1010, 0b0001], None),       # ... and at n
                      ([0b10, 0b01], [0, 1])):        # an edge between two keys
        assert host.team_pcm_clique(rows(adj), pair, out=out) == E_ARG and is_untouched(out), adj
    for kw in (dict(min_support=0), dict(max_nodes=0), dict(max_translation=-1.0)):
        assert host.team_pcm_clique(rows(tri), out=out, **kw) == E_ARG and is_untouched(out), kw
    assert host.team_pcm_clique(rows([]), min_support=1) == dict(n_factors=0, n_kept=0, n_pairs=0, n_pairs_kept=0, exact=1, nodes_max=0, kept=[])


def test_the_windows_hypotheses_on_the_cpu():
    """the fixture of tests/rendezvous_window_cases.py through host_window_chain(): the admissible hypotheses of slot 1 as
    factors keep all five at the defaults; slot 3's two aliases, which claim frames 3 m apart, keep nothing at
    min_support 2 — what tests/test_gpu_team_pcm.py asks of the device, confirmed without one"""
    import place_loop_cases as plc
    import rendezvous_window_cases as rwc

    fr = rwc.slots()
    gs = {}
    for s in (0, 1, 3):
        gs[s] = host.PoseGraph(len(fr[s]), 2)
        for i, f in enumerate(fr[s]):
            assert gs[s].push(plc.six_of_key(fr[s][i - 1][3]) if i else None, plc.six_of_key(f[3])) == i
    T = {s: g.poses_f64() for s, g in gs.items()}

    def groups(slot):
        """the admissible hypotheses of `slot`, one group per target slot named: target -> (factors over the members (target,
        slot), Tb, Ta)"""
        out = {}
        for h in rwc.host_window_chain(slot)["hyp"]:
            if not h["admissible"]:
                continue
            t = h["cand"]["slot"]
            f = host.team_factor(T[slot][h["frame"]], T[t][h["cand"]["id"]], np.asarray(h["icp"]["transform"], np.float64), h["icp"]["fitness"])
            assert not isinstance(f, int)
            f.slot_b, f.id_b, f.slot_a, f.id_a = 1, h["frame"], 0, h["cand"]["id"]
            fs, Tb, Ta = out.setdefault(t, ([], [], []))
            fs.append(f), Tb.append(T[slot][h["frame"]]), Ta.append(T[t][h["cand"]["id"]])
        return {t: (fs, np.array(Tb), np.array(Ta)) for t, (fs, Tb, Ta) in out.items()}

    as_tuples = lambda fs: [(f.slot_b, f.id_b, f.slot_a, f.id_a, np.array(f.Z[:]), f.var) for f in fs]
    g1 = groups(1)
    assert sorted(g1) == [0]
    fs, Tb, Ta = g1[0]
    r = host.team_factors_consistent(fs, Tb, Ta)
    assert len(fs) == 5 and r["kept"] == [0, 1, 2, 3, 4] and (r["n_pairs"], r["n_pairs_kept"], r["exact"]) == (1, 1, 1)
    assert r == tpn.evaluate(as_tuples(fs), Tb, Ta)
    g3 = groups(3)
    assert sorted(g3) == [0, 1]  # (slot 1 drove where slot 0 did: the aliases look like both)
    for t, (fs, Tb, Ta) in sorted(g3.items()):
        r = host.team_factors_consistent(fs, Tb, Ta, min_support=2)
        assert len(fs) == 2 and r["kept"] == [] and (r["n_pairs"], r["n_pairs_kept"]) == (1, 0)
        recs = tpn.records(as_tuples(fs), Tb, Ta)
        print("slot 3's two aliases in slot %d: %.2f m and %.2f degrees apart" % (t, tpn.apart(recs[0], recs[1]), np.degrees(tpn.angle(recs[0], recs[1]))))
        assert tpn.apart(recs[0], recs[1]) > 2.0  # (far from the bar of 1 m: nothing near a threshold crosses two arithmetics)
