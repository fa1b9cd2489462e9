"""lins_rendezvous_step (include/lins_team.h) on the fixture of tests/rendezvous_cases.py — three robots, slot 1's map
frame displaced from slot 0's by G, 7 m and 26 degrees (tests/test_rendezvous_inputs.py asserts the fixture on the CPU).
Every entry's bits are those of the explicit chain of the four calls for its slot, in any batch and order; the call
leaves graph, archive and the streams' map poses as they were; slot 1's latest frame is FOUND in slot 0.

X against the CPU restatement: the bar of tests/test_gpu_loop_icp.py, loop_icp_cases.BAR_T in every entry of T.
X against the truth: the CPU restatement's X puts the query frame's origin e = 0.036 m from where it truly stood
(asserted on the CPU against place_loop_cases.bound()[0] = 0.105 m); the device is asserted at 2 e, the margin
tests/test_gpu_place_loop.py took."""
import numpy as np
import pytest

import loop_icp_cases as licp
import loop_step_cases as lsc
import place_loop_cases as plc
import rendezvous_cases as rc
from map_step_chain import sm

pytestmark = pytest.mark.gpu
host, team, defs = rc.host, rc.team, lsc.defs
N, LATEST = rc.N, rc.N - 1
ALL = [0, 1, 2]
E_ARG, E_INPUT, E_STATE = -1, -4, -6


def params(ieskf, **kw):
    return lsc.params(ieskf.lib(), **dict(dict(min_gap_s=rc.GAP, search_num=rc.H), **kw))


def context(pkg, ieskf, place=True):
    fr = rc.slots()[0]
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=3, max_targets=1024)
    c.streams_init(3)
    c.local_map_init(3, 3, 1024)  # (the streams' map side wants a local map; its rings stay empty)
    c.archive_init(3, 16, sum(len(x) for s in fr.values() for f in s for x in f[:3]) + 16)
    sm.init(c, 3)
    c.pose_graph_init(3, 16, 2)
    if place:
        assert c.place_init(up_axis=rc.UP) == 0
    for s in ALL:
        for i, f in enumerate(fr[s]):
            pose = tuple(float(v) for v in f[3])
            assert c.archive_push(s, *f[:3], pose, time=float(i)) == c.pose_graph_push(s, plc.six_of_key(fr[s][i - 1][3]) if i else None, plc.six_of_key(f[3])) == i
        # a map pose with every field set, different per stream: the streams' records are part of what a step must leave alone
        six = np.asarray(plc.six_of_key(fr[s][N - 1][3]), np.float32)
        sm.set_pose(c, s, dict(bef=six - np.float32(0.01 * (s + 1)), aft=six, tobe=six + np.float32(0.02), last=six, prev=six[3:6], n_frames=N,
                               last_time=float(N - 1) + 0.1 * s))
    return c


def map_pose(c, s):
    p = sm.get_pose(c, s)
    return tuple(np.asarray(p[k], np.float32).tobytes() for k in ("bef", "aft", "tobe", "last", "prev")) + (p["n_frames"], p["last_time"])


def state(c):
    """graph, archive and the stream's map pose of every slot as bytes (the archive's key poses through an assembly of every frame)"""
    out = []
    for s in ALL:
        c.archive_assemble([dict(slot=s, ids=list(range(N)), clouds=7, leaf=0.0, flags=0)])
        out.append((c.pose_graph_count(s), c.pose_graph_poses(s).tobytes(), c.debug_pose_graph_poses_f64(s).tobytes(), c.archive_download(0).tobytes(),
                    map_pose(c, s)))
    return out


def zero_result():
    info = defs.SubmapInfoC().as_dict()
    return dict(outcome=defs.RENDEZVOUS_NONE, status=0, latest_id=-1, n_candidates=0, chosen=-1, target_slot=-1, target_id=-1, latest=info, cand=[],
                target=[], icp=[], X=np.zeros((4, 4)))


def chain(c, slot, prm, targets=ALL, shortlist=rc.M, k=rc.K, max_distance=1.0):
    """the explicit chain of the four calls for one slot -> the dict lins_rendezvous_step gives for its entry"""
    fr = rc.slots()[0]
    r = zero_result()
    latest = r["latest_id"] = c.archive_count(slot) - 1
    ranks = team.topk(c, [(slot, latest, rc.NOW, prm.min_gap_s)], targets, shortlist=shortlist, k=k, min_sep=prm.search_num)[0]
    r["cand"] = [x for x in ranks if not x["distance"] > max_distance]
    r["n_candidates"] = len(r["cand"])
    if not r["cand"]:
        return r
    infos = c.archive_assemble([dict(slot=slot, ids=[latest], clouds=3, leaf=0.0, flags=1)] +
                               [dict(slot=x["slot"], ids=host.loop_window(c.archive_count(x["slot"]) - 1, x["id"], prm.search_num), clouds=3,
                                     leaf=prm.history_leaf, flags=0) for x in r["cand"]])
    r["latest"], r["target"] = infos[0], infos[1:]
    T0 = [team.host_guess(fr[slot][latest][3], fr[x["slot"]][x["id"]][3], x["shift"], rc.UP) for x in r["cand"]]
    r["icp"] = c.loop_icp_from([(0, 1 + j) for j in range(len(T0))], T0, prm.icp)
    r["outcome"] = defs.RENDEZVOUS_REJECTED
    j = r["chosen"] = host.loop_choose([i["converged"] for i in r["icp"]], [i["fitness"] for i in r["icp"]], prm.max_fitness)
    if j >= 0:
        r["outcome"], r["target_slot"], r["target_id"], r["X"] = defs.RENDEZVOUS_FOUND, r["cand"][j]["slot"], r["cand"][j]["id"], r["icp"][j]["transform"]
    return r


def step(c, entries, prm, targets=ALL, **kw):
    kw.setdefault("shortlist", rc.M), kw.setdefault("k", rc.K)
    return team.rendezvous_step(c, [(s, rc.NOW) for s in entries], targets, prm, **kw)


@pytest.fixture(scope="module")
def pair(pkg, ieskf):
    a, b = context(pkg, ieskf), context(pkg, ieskf)
    yield a, b
    a.close(), b.close()


def test_the_step_is_the_explicit_chain_and_leaves_the_state(pair, ieskf):
    a, b = pair
    prm = params(ieskf)
    before = state(a)
    got = step(a, ALL, prm)
    assert isinstance(got, list) and state(a) == before
    want = [chain(b, s, prm) for s in ALL]
    for s in ALL:
        assert lsc.frozen(got[s]) == lsc.frozen(want[s]), s
    print("outcomes:", [(g["outcome"], g["target_slot"], g["target_id"], g["n_candidates"], g["chosen"]) for g in got])
    # the other order, each entry alone, and again after other calls on the context
    assert lsc.frozen(step(a, ALL[::-1], prm)) == lsc.frozen(got[::-1])
    for s in ALL:
        assert lsc.frozen(step(a, [s], prm)) == lsc.frozen([got[s]])
    assert isinstance(a.place_search([(0, 3, 1, 3.0, -1.0)] * 5), list)
    a.archive_assemble([dict(slot=2, ids=[0, 1], clouds=7, leaf=0.4, flags=0)])
    assert lsc.frozen(step(a, ALL, prm, targets=[2, 0, 1])) == lsc.frozen(got)
    assert state(a) == before
    # other parameters take other paths: a gate that drops every rank; one rank; a target list without the counterpart's slot
    assert lsc.frozen(step(a, ALL, prm, max_distance=0.0)) == lsc.frozen([chain(b, s, prm, max_distance=0.0) for s in ALL])
    assert all(g["outcome"] == defs.RENDEZVOUS_NONE and g["latest_id"] == LATEST and g["n_candidates"] == 0 for g in step(a, ALL, prm, max_distance=0.0))
    assert lsc.frozen(step(a, [1, 2], prm, targets=[1, 2], shortlist=3, k=1)) == lsc.frozen([chain(b, s, prm, [1, 2], 3, 1) for s in (1, 2)])
    assert step(a, [], prm) == []


def test_slot_1_finds_itself_in_slot_0_and_X_is_G(pair, ieskf):
    a, b = pair
    got = step(a, [1], params(ieskf))[0]
    h = rc.host_chain(1)
    print("device ranks:", [(x["slot"], x["id"], x["shift"], float(x["distance"])) for x in got["cand"]], "fitness:", [i["fitness"] for i in got["icp"]])
    assert (got["outcome"], got["target_slot"], got["target_id"], got["status"]) == (defs.RENDEZVOUS_FOUND, 0, LATEST, 0)
    # the shortlist and the ranks are the restatement's, bit for bit; the alignment within the loop ICP's device bar
    assert [(x["slot"], x["id"], x["shift"], x["distance"].tobytes(), x["dk"]) for x in got["cand"]] == \
        [(x["slot"], x["id"], x["shift"], x["distance"].tobytes(), x["dk"]) for x in h["ranks"]]
    assert got["chosen"] == h["chosen"] == 0
    diff = float(np.abs(got["X"] - h["X"]).max())
    e_host, e_dev = rc.origin_error(h["X"]), rc.origin_error(got["X"])
    print("X: device against the restatement %.3g (bar %.3g); origin error: restatement %.4f m, device %.4f m" % (diff, licp.BAR_T, e_host, e_dev))
    assert diff <= licp.BAR_T
    assert e_host <= plc.bound()[0] and e_dev <= 2.0 * e_host
    # X takes slot 1's map frame to slot 0's: G, as far as the alignment goes
    assert np.abs(got["X"] - rc.G()).max() < 0.1


def test_refusals_change_nothing(pkg, ieskf, pair):
    a, _ = pair
    prm = params(ieskf)
    before = state(a)
    want = step(a, ALL, prm)
    for entries, targets in (([0, 0], ALL), ([3], ALL), ([-1], ALL), ([0], [0, 0]), ([0], [3])):
        assert step(a, entries, prm, targets) == E_ARG, (entries, targets)
    for kw in (dict(shortlist=0), dict(k=9), dict(min_sep=-2), dict(max_distance=float("nan"))):
        assert step(a, ALL, prm, **kw) == E_ARG, kw
    assert step(a, ALL, params(ieskf, search_num=-1)) == E_ARG and step(a, ALL, params(ieskf, history_leaf=-1.0)) == E_ARG
    assert team.rendezvous_step(a, [(0, rc.NOW), (1, float("inf"))], ALL, prm) == E_INPUT
    assert lsc.frozen(step(a, ALL, prm)) == lsc.frozen(want) and state(a) == before
    c = context(pkg, ieskf, place=False)
    assert step(c, ALL, prm) == E_STATE  # before lins_place_init
    c.close()
