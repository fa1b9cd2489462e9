"""Pairwise-consistent team factors on the device (include/lins_team.h lins_team_factors_consistent_batch) against their
definition on the CPU (lins_host_team_factors_consistent, itself pinned to the numpy checker by
tests/test_team_pcm_host.py): every bit of the 32-byte record on every case of tests/team_pcm_cases.py, the search stage
alone (lins_debug_team_pcm_clique) against its twin on seeded graphs, a group's independence of its batch, the refusals,
the planted case end to end through keep_factors and lins_team_graph_solve, and the rendezvous window's hypotheses as
factors before and after a rebase.

The kernel calls the host's scalar text (csrc/host/team_pcm.h) on its LDS copy of the group, f64 with contraction off and no
libm: equality is asked bit for bit, with no tolerance."""
import ctypes as C
import importlib

import numpy as np
import pytest

import pose_graph_cases as pgc
import team_pcm_cases as tpc

pytestmark = pytest.mark.gpu
host = importlib.import_module("lins---lidar-inertial-slam_amd.host")
team = importlib.import_module("lins---lidar-inertial-slam_amd.team")
defs = importlib.import_module("lins---lidar-inertial-slam_amd._ctypes_defs")

E_ARG, E_CAPACITY, E_INPUT, E_STATE = -1, -3, -4, -6
MAX_FRAMES, MAX_LOOPS = 130, 4
CASES = tpc.cases()


@pytest.fixture
def ctx(pkg, ieskf):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    yield c
    c.close()


class DevGraph:
    def __init__(self, ctx, slot):
        self.ctx, self.slot = ctx, slot

    def push(self, last6, aft6):
        return self.ctx.pose_graph_push(self.slot, last6, aft6)

    def add_loop(self, b, a, pf, var):
        return self.ctx.pose_graph_add_loop(self.slot, b, a, pf, var)


def fill(ctx, members, first=0):
    slots = list(range(first, first + len(members)))
    for s, c in zip(slots, members):
        pgc.fill(DevGraph(ctx, s), c)
    return slots


def on_slots(factors, slots):
    return [(slots[mb], ib, slots[ma], ia, Z, var) for mb, ib, ma, ia, Z, var in factors]


def host_record(ctx, slots, factors, **params):
    """the definition on the poses the context holds: the factors' slots are member indices here"""
    T = [ctx.debug_pose_graph_poses_f64(s) for s in slots]
    Tb = np.array([T[f[0]][f[1]] for f in factors]).reshape(-1, 12)
    Ta = np.array([T[f[2]][f[3]] for f in factors]).reshape(-1, 12)
    return host.team_factors_consistent(factors, Tb, Ta, **params)


def test_every_case_is_the_host_record(ctx):
    for c in CASES:
        ctx.pose_graph_init(len(c["members"]), MAX_FRAMES, MAX_LOOPS)
        slots = fill(ctx, c["members"])
        want = host_record(ctx, slots, c["factors"], **c["params"])
        got = team.factors_consistent(ctx, [(slots, on_slots(c["factors"], slots))], **c["params"])
        print("%-26s L %2d kept %2d pairs %d/%d exact %d nodes_max %6d  %.3f ms" % (
            c["name"], want["n_factors"], want["n_kept"], want["n_pairs_kept"], want["n_pairs"], want["exact"], want["nodes_max"], team.pcm_stats(ctx)))
        assert isinstance(got, list) and got[0] == want, c["name"]
        for k, v in c["want"].items():
            assert got[0][k] == v, (c["name"], k)


@pytest.mark.parametrize("seed,density", tpc.RANDOM_GRAPHS)
def test_the_search_stage_against_its_twin(ctx, seed, density):
    adj = np.array(tpc.random_graph(seed, density), np.uint64)
    want = host.team_pcm_clique(adj, min_support=1)
    assert want["exact"] == 1 and team.debug_pcm_clique(ctx, adj, min_support=1) == want
    short = host.team_pcm_clique(adj, min_support=1, max_nodes=want["nodes_max"] - 1)
    assert short["exact"] == 0 and team.debug_pcm_clique(ctx, adj, min_support=1, max_nodes=want["nodes_max"] - 1) == short
    # two keys: the graph's halves searched apart
    pair = [v % 2 for v in range(64)]
    halves = np.array([int(r) & (0x5555555555555555 << (v % 2)) for v, r in enumerate(adj)], np.uint64)
    assert team.debug_pcm_clique(ctx, halves, pair, min_support=2) == host.team_pcm_clique(halves, pair, min_support=2)
    # the twin's refusals, and nothing written
    out = defs.TeamPcmResultC(71, 72, 73, 74, 75, 76)
    assert team.debug_pcm_clique(ctx, np.array([2, 0], np.uint64), out=out) == E_ARG and team.debug_pcm_clique(ctx, adj, max_nodes=0, out=out) == E_ARG
    assert (out.n_factors, out.n_kept, out.n_pairs, out.n_pairs_kept, out.exact, out.nodes_max) == (71, 72, 73, 74, 75, 76)


def default_cases():
    """the cases under the default parameters, the empty group among them"""
    return [c for c in CASES if not c["params"]]


def batch_calls(ctx, n_groups):
    """n_groups groups, the default cases over and over in slots of their own -> the groups as the call takes them"""
    cs = default_cases()
    picks = [cs[i % len(cs)] for i in range(n_groups)]
    ctx.pose_graph_init(sum(len(c["members"]) for c in picks), MAX_FRAMES, MAX_LOOPS)
    calls, first = [], 0
    for c in picks:
        slots = fill(ctx, c["members"], first)
        calls.append((slots, on_slots(c["factors"], slots)))
        first += len(slots)
    return picks, calls


def test_a_groups_record_does_not_depend_on_its_batch(ctx):
    picks, calls = batch_calls(ctx, 64)
    assert any(not c["factors"] for c in picks[1:-1])  # an empty group between full ones
    together = team.factors_consistent(ctx, calls)
    assert isinstance(together, list) and len(together) == 64
    cs = default_cases()
    for i, (c, r) in enumerate(zip(picks, together)):
        assert r == together[i % len(cs)], c["name"]  # the same group in other slots
    alone = [team.factors_consistent(ctx, [calls[i]])[0] for i in range(len(cs))]
    assert alone == together[:len(cs)]
    assert team.factors_consistent(ctx, calls[::-1])[::-1] == together
    # another batch in between (the staging and the LDS used), then the same call
    assert isinstance(team.factors_consistent(ctx, [calls[5], calls[2], calls[40]], min_support=1, max_nodes=17, max_translation=0.01), list)
    assert team.factors_consistent(ctx, calls) == together
    # without the empty groups nothing changes for the others
    full = [i for i, c in enumerate(picks) if c["factors"]]
    assert team.factors_consistent(ctx, [calls[i] for i in full]) == [together[i] for i in full]
    for c, r in zip(cs, together):
        assert r == host_record(ctx, calls[cs.index(c)][0], c["factors"]), c["name"]
    assert team.factors_consistent(ctx, []) == []


def test_planted_group_keeps_its_mask_behind_a_rebase(ctx):
    """10 on the device: the planted group's record, then member 1's graph rebased in the context by the 7 m / 26 degree X of
    tests/test_team_pcm_host.py — the kernel forms every X_l from the rebased f64 poses — and the record again: each equal
    to the host's on the context's poses in every bit, and the same mask, exactly the inliers.  (That host test shows by the
    checker alone that no pair lies near a bar, before and after.)"""
    import pose_graph_np as pnp

    c = tpc.planted()
    ctx.pose_graph_init(2, MAX_FRAMES, MAX_LOOPS)
    slots = fill(ctx, c["members"])
    groups = [(slots, on_slots(c["factors"], slots))]
    X = np.eye(4)
    X[:3, :3] = pnp.rot_axis(1, np.deg2rad(26.0))  # (the archive's vertical axis is 1)
    X[:3, 3] = [4.0, -1.0, 5.657]
    before = team.factors_consistent(ctx, groups)
    assert before[0] == host_record(ctx, slots, c["factors"]) and before[0]["kept"] == tpc.PLANTED_INLIERS
    pushed = ctx.debug_pose_graph_poses_f64(1).copy()
    assert team.pose_graph_rebase(ctx, [1], [X]) == 0
    assert np.abs(ctx.debug_pose_graph_poses_f64(1) - pushed).max() > 3.0  # (the rebase did move the member)
    after = team.factors_consistent(ctx, groups)
    assert after[0] == host_record(ctx, slots, c["factors"])
    assert after == before and after[0]["kept"] == tpc.PLANTED_INLIERS and (after[0]["n_pairs"], after[0]["n_pairs_kept"], after[0]["exact"]) == (1, 1, 1)


def test_the_call_changes_no_graph(ctx):
    c = tpc.planted()
    ctx.pose_graph_init(2, MAX_FRAMES, MAX_LOOPS)
    slots = fill(ctx, c["members"])
    state = lambda: [(ctx.pose_graph_count(s), ctx.debug_pose_graph_poses_f64(s).tobytes(), ctx.pose_graph_poses(s).tobytes()) for s in slots]
    before = state()
    assert team.factors_consistent(ctx, [(slots, on_slots(c["factors"], slots))])[0]["kept"] == tpc.PLANTED_INLIERS
    assert state() == before


def test_refusals_change_nothing(pkg, ieskf, ctx):
    c = tpc.planted()
    fs = c["factors"]
    assert team.factors_consistent(ctx, [([0, 1], on_slots(fs, [0, 1]))]) == E_STATE
    ctx.pose_graph_init(4, MAX_FRAMES, MAX_LOOPS)  # slot 2: a third graph; slot 3: no frames
    slots = fill(ctx, c["members"])
    fill(ctx, [c["members"][0]], 2)
    ok = on_slots(fs, slots)
    out = (defs.TeamPcmResultC * 2)()
    C.memmove(out, bytes(range(71, 71 + 64)), 64)  # every byte of both 32-byte records
    sentinel = bytes(out)
    assert len(sentinel) == 64 and out[1].kept[1] != 0

    def refused(groups, **kw):
        rc = team.factors_consistent(ctx, groups, out=out, **kw)
        assert bytes(out) == sentinel, (groups[0][0], kw)
        return rc

    def with_(i, **kw):
        f = dict(zip(("slot_b", "id_b", "slot_a", "id_a", "Z", "var"), ok[i]))
        f.update(kw)
        return ok[:i] + [f] + ok[i + 1:]

    for kw in (dict(max_translation=-1.0), dict(max_translation=np.inf), dict(min_cos_rotation=np.nan), dict(translation_per_frame=-1.0),
               dict(translation_per_frame=np.nan), dict(min_support=0), dict(max_nodes=0)):
        assert refused([(slots, ok)], **kw) == E_ARG, kw
    for moff, foff in (([1, 2], [0, 8]), ([0, 2], [1, 8]), ([0, 2, 1], [0, 8, 8]), ([0, 2, 3], [0, 8, 0]), ([0, 2, 2], [0, 8, 8]), ([0, 5], [0, 8])):
        assert refused([(slots + [2], ok)] + [([], [])] * (len(moff) - 2), member_offsets=moff, factor_offsets=foff) == E_ARG, (moff, foff)
    assert refused([([], [])]) == E_ARG  # an empty group
    for members in ([0, 4], [0, -1], [0, 3], [0, 0]):  # out of range, without frames, twice
        assert refused([(members, [])]) == E_ARG, members
    assert refused([(slots, ok), ([2, 1], [])]) == E_ARG  # twice in the call
    for kw in (dict(slot_b=2), dict(slot_a=2), dict(slot_b=4), dict(slot_a=-1), dict(slot_b=1), dict(slot_a=0), dict(id_b=130), dict(id_a=-1)):
        assert refused([(slots, with_(0, **kw)), ([2], [])]) == E_ARG, kw  # (slot 2 is another group's)
    Z = np.array(ok[3][4])
    nan_z, skew = Z.copy(), Z.copy()
    nan_z[10], skew[4] = np.nan, Z[4] + 1e-6
    for kw in (dict(Z=nan_z), dict(Z=skew), dict(var=0.0), dict(var=np.nan), dict(var=np.inf), dict(var=-1.0)):
        assert refused([(slots, with_(3, **kw))]) == E_INPUT, kw
    m = tpc.pair_members(70)
    ctx2 = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    try:
        # 65 factors are refused whatever max_loops is, 64 are taken (max_loops is 1 here)
        ctx2.pose_graph_init(2, 70, 1)
        s2 = fill(ctx2, m)
        many = on_slots([tpc.near(m, i, i) for i in range(65)], s2)
        assert team.factors_consistent(ctx2, [(s2, many)], out=out) == E_CAPACITY and bytes(out) == sentinel
        assert team.factors_consistent(ctx2, [(s2, many[:64])])[0]["n_kept"] == 64
        # behind the refusals the valid call is a fresh context's
        ctx2.pose_graph_init(2, MAX_FRAMES, MAX_LOOPS)
        fill(ctx2, c["members"])
        fresh = team.factors_consistent(ctx2, [(slots, ok)])
    finally:
        ctx2.close()
    got = team.factors_consistent(ctx, [(slots, ok), ([2], [])])
    assert got[0] == fresh[0] and got[0]["kept"] == tpc.PLANTED_INLIERS and got[1] == dict(n_factors=0, n_kept=0, n_pairs=0, n_pairs_kept=0, exact=1, nodes_max=0, kept=[])


ROOT_VARIANCE = [2.5e-6] * 3 + [2.5e-3] * 3  # a root after an ICP, as tests/test_gpu_team_graph.py ROOT_AFTER_ICP


def solved(ctx, c, factors):
    """fresh graphs of the case, the team [0, 1] solved with `factors` -> (result, every slot's state, member 1's f64 poses)"""
    ctx.pose_graph_init(2, MAX_FRAMES, MAX_LOOPS)
    slots = fill(ctx, c["members"])
    r = team.graph_solve(ctx, [(slots, factors)], root_variance=ROOT_VARIANCE)
    assert isinstance(r, list) and r[0]["status"] == 0
    return r[0], [(ctx.pose_graph_count(s), ctx.debug_pose_graph_poses_f64(s).tobytes(), ctx.pose_graph_poses(s).tobytes()) for s in slots], \
        ctx.debug_pose_graph_poses_f64(1).copy()


def host_origin_errors(c, factor_sets):
    """lins_host_team_graph_solve on the CPU with each factor set -> member 1's mean origin error against the poses as pushed"""
    out = []
    for fs in factor_sets:
        gs = [host.PoseGraph(len(m["aft"]), MAX_LOOPS) for m in c["members"]]
        for g, m in zip(gs, c["members"]):
            pgc.fill(g, m)
        pushed = gs[1].poses_f64()[:, 9:].copy()
        r = host.team_graph_solve(gs, fs, None, ROOT_VARIANCE)
        assert r["status"] == 0
        out.append(float(np.linalg.norm(gs[1].poses_f64()[:, 9:] - pushed, axis=1).mean()))
    return out


def test_planted_case_end_to_end(ctx):
    """keep_factors followed by the team solve is, bit for bit, the solve handed the six inliers directly.  Reported: member
    1's mean origin error against the poses as pushed with all 8 factors and with the kept 6; measured on an MI355X:
    6.1310 m against 0.0264 m (lins_host_team_graph_solve on the CPU: the same to four places; DESIGN.md section 5.3
    "Pairwise-consistent team factors").  kept < unfiltered is asserted only where the CPU restatement shows a tenfold
    gap first."""
    c = tpc.planted()
    ctx.pose_graph_init(2, MAX_FRAMES, MAX_LOOPS)
    slots = fill(ctx, c["members"])
    pushed = ctx.debug_pose_graph_poses_f64(1)[:, 9:].copy()
    all8 = on_slots(c["factors"], slots)
    res = team.factors_consistent(ctx, [(slots, all8)])
    kept, off = team.keep_factors(all8, [0, len(all8)], res)
    assert list(off) == [0, 6] and len(kept) == 6 and all(a is all8[i] for a, i in zip(kept, tpc.PLANTED_INLIERS))
    r_kept, s_kept, T_kept = solved(ctx, c, kept)
    r_direct, s_direct, _ = solved(ctx, c, [all8[i] for i in tpc.PLANTED_INLIERS])
    assert r_kept == r_direct and s_kept == s_direct and r_kept["n_factors"] == 6 and r_kept["iterations"] > 0
    r_all, _, T_all = solved(ctx, c, all8)
    err = lambda T: float(np.linalg.norm(T[:, 9:] - pushed, axis=1).mean())
    cpu_all, cpu_kept = host_origin_errors(c, [c["factors"], [c["factors"][i] for i in tpc.PLANTED_INLIERS]])
    print("member 1's mean origin error against the poses as pushed: all 8 factors %.4f m (CPU %.4f), the kept 6 %.4f m (CPU %.4f); cost %.4g -> %.4g against %.4g -> %.4g" % (
        err(T_all), cpu_all, err(T_kept), cpu_kept, r_all["cost_before"], r_all["cost_after"], r_kept["cost_before"], r_kept["cost_after"]))
    if cpu_all >= 10.0 * cpu_kept:
        assert err(T_kept) < err(T_all)


def test_the_windows_hypotheses_before_and_after_a_rebase(pkg, ieskf):
    """the fixture of tests/rendezvous_window_cases.py: the admissible hypotheses of slot 1 and of slot 3 as factors, one group
    per target slot named.  Before any rebase slot 1 keeps all five at the defaults and slot 3's two aliases — they claim
    frames 3 m apart — keep nothing at min_support 2; after lins_team_rebase of slot 1 by the winner's X the mask is the same."""
    import test_gpu_rendezvous_window as rw

    c = rw.context(pkg, ieskf)
    try:
        got = dict(zip((1, 3), rw.step(c, [1, 3], rw.params(ieskf))))
        groups = {}
        for s in (1, 3):
            g = got[s]
            by_target = {}
            for h in g["hyp"]:
                if h["admissible"]:
                    f = team.factor_from_alignment(c, s, g["query_id"][h["query"]], h["cand"]["slot"], h["cand"]["id"],
                                                   np.asarray(h["icp"]["transform"], np.float64), h["icp"]["fitness"])
                    assert not isinstance(f, int)
                    by_target.setdefault(h["cand"]["slot"], []).append(f)
            groups[s] = [([t, s], fs) for t, fs in sorted(by_target.items())]
        assert got[1]["outcome"] == rw.FOUND and [len(fs) for _, fs in groups[1]] == [5] and groups[1][0][0] == [0, 1]
        before = team.factors_consistent(c, groups[1])
        assert before[0]["kept"] == [0, 1, 2, 3, 4] and (before[0]["n_pairs"], before[0]["n_pairs_kept"], before[0]["exact"]) == (1, 1, 1)
        assert [(m, len(fs)) for m, fs in groups[3]] == [([0, 3], 2), ([1, 3], 2)]  # (slot 1 drove where slot 0 did: the aliases look like both)
        for g in groups[3]:  # (slot 3 is a member of both: a call each)
            aliases = team.factors_consistent(c, [g], min_support=2)
            assert aliases[0]["kept"] == [] and (aliases[0]["n_factors"], aliases[0]["n_pairs"], aliases[0]["n_pairs_kept"]) == (2, 1, 0)
        assert team.rebase(c, [1], [np.asarray(got[1]["X"], np.float64).reshape(4, 4)], streams=[1]) == 0
        assert team.factors_consistent(c, groups[1]) == before
    finally:
        c.close()
