"""lins_rendezvous_window_step (include/lins_team.h) on the four-robot fixture of tests/rendezvous_window_cases.py, twelve
frames a slot (tests/test_rendezvous_window_inputs.py asserts the fixture on the CPU).  Every entry's bits are those of
the explicit chain for its slot — lins_place_team_topk_batch, the drop, lins_archive_assemble, lins_loop_icp_batch_from,
lins_host_rendezvous_consensus — in any batch and order; with a window of one and min_support 1 the step is
lins_rendezvous_step; slot 3, whose latest frame alone is FOUND, is UNCONFIRMED over a window; slot 1 is FOUND in slot 0
with all five frames agreeing; slot 2 is REJECTED; a refused call and the step itself leave graphs, archive, rings and
map poses as they were; the window's X goes to lins_team_rebase as it is.

X against the truth: the CPU restatement's winner puts its frame's origin e = 0.043 m from where it truly stood (asserted
on the CPU against place_loop_cases.bound()[0] = 0.105 m); the device is asserted at that same bound."""
import numpy as np
import pytest

import loop_step_cases as lsc
import map_step_chain as ch
import place_loop_cases as plc
import rendezvous_cases as rc
import rendezvous_window_cases as rwc
from map_step_chain import sm

pytestmark = pytest.mark.gpu
host, team, defs = rc.host, rc.team, lsc.defs
N, LATEST, F = rwc.N, rwc.N - 1, np.float32
ALL, TARGETS = [0, 1, 2, 3], [0, 1, 2]
E_ARG, E_INPUT, E_STATE = -1, -4, -6
NONE, REJECTED, FOUND, UNCONFIRMED = defs.RENDEZVOUS_NONE, defs.RENDEZVOUS_REJECTED, defs.RENDEZVOUS_FOUND, defs.RENDEZVOUS_UNCONFIRMED


def params(ieskf, **kw):
    return lsc.params(ieskf.lib(), **dict(dict(min_gap_s=rwc.GAP, search_num=rwc.H), **kw))


def context(pkg, ieskf, place=True):
    """archive, ring (window 3), graph, place store and a map pose per stream, four of each"""
    fr = rwc.slots()
    c = ch.context(pkg, ieskf, n=4)
    c.streams_init(4)
    c.local_map_init(4, 3, ch.MAX_PTS)
    c.archive_init(4, 16, sum(len(x) for s in fr.values() for f in s for x in f[:3]) + (1 << 17))  # (room for the key frame of a map step)
    sm.init(c, 4, ch.INTERVAL)
    c.pose_graph_init(4, 16, 2)
    if place:
        assert c.place_init(up_axis=rwc.UP) == 0
    for s in ALL:
        for i, f in enumerate(fr[s]):
            pose = tuple(float(v) for v in f[3])
            assert c.archive_push(s, *f[:3], pose, time=float(i)) == c.pose_graph_push(s, plc.six_of_key(fr[s][i - 1][3]) if i else None, plc.six_of_key(f[3])) == i
            c.local_map_push(s, *f[:3], pose)
        # a map pose with every field set, different per stream: the streams' records are part of what a step must leave alone
        six = np.asarray(plc.six_of_key(fr[s][LATEST][3]), F)
        sm.set_pose(c, s, dict(bef=six - F(0.01 * (s + 1)), aft=six, tobe=six + F(0.02), last=six, prev=six[3:6], n_frames=N, last_time=float(LATEST) + 0.1 * s))
    return c


def state(c):
    """graph, archive (an assembly of every frame), ring (a build against it) and the stream's map pose of every slot, as bytes"""
    out = []
    scan = rwc.slots()[0][0][:3]
    for s in ALL:
        c.archive_assemble([dict(slot=s, ids=list(range(N)), clouds=7, leaf=0.0, flags=0)])
        arch = c.archive_download(0).tobytes()
        c.local_map_build([s], [scan])
        p = sm.get_pose(c, s)
        out.append((c.pose_graph_count(s), c.pose_graph_poses(s).tobytes(), c.debug_pose_graph_poses_f64(s).tobytes(), arch,
                    c.local_map_download(0, 0).tobytes(), c.local_map_download(0, 1).tobytes(),
                    tuple(np.asarray(p[k], F).tobytes() for k in ("bef", "aft", "tobe", "last", "prev")) + (p["n_frames"], p["last_time"])))
    return out


def chain(c, slot, prm, window=5, stride=1, min_support=3, targets=TARGETS, shortlist=rwc.M, k=rwc.K, max_distance=1.0):
    """the explicit chain of the five calls for one slot -> the dict lins_rendezvous_window_step gives for its entry"""
    fr = rwc.slots()
    latest = c.archive_count(slot) - 1
    qid = [latest - j * stride for j in range(window) if latest - j * stride >= 0]
    r = dict(outcome=NONE, status=0, n_queries=len(qid), n_hypotheses=0, winner=-1, support=0, n_admissible=0, target_slot=-1, target_id=-1, members=[],
             query_id=qid, n_ranks=[0] * len(qid), source=[defs.SubmapInfoC().as_dict() for _ in qid], X=np.zeros((4, 4)), hyp=[])
    if not qid:
        return r
    found = team.topk(c, [(slot, q, rwc.NOW, prm.min_gap_s) for q in qid], targets, shortlist=shortlist, k=k, min_sep=prm.search_num)
    for j, ranks in enumerate(found):
        for x in ranks:
            if not x["distance"] > max_distance and x["slot"] != slot:
                r["hyp"].append(dict(query=j, rank=r["n_ranks"][j], admissible=0, member=0, cand=x))
                r["n_ranks"][j] += 1
    r["n_hypotheses"] = len(r["hyp"])
    if not r["hyp"]:
        return r
    specs, src_of = [], {}
    for h in r["hyp"]:
        if h["rank"] == 0:
            src_of[h["query"]] = len(specs)
            specs.append(dict(slot=slot, ids=[qid[h["query"]]], clouds=3, leaf=0.0, flags=1))
        h["spec"] = len(specs)
        x = h["cand"]
        specs.append(dict(slot=x["slot"], ids=host.loop_window(c.archive_count(x["slot"]) - 1, x["id"], prm.search_num), clouds=3, leaf=prm.history_leaf, flags=0))
    infos = c.archive_assemble(specs)
    for j, at in src_of.items():
        r["source"][j] = infos[at]
    T0 = [team.host_guess(fr[slot][qid[h["query"]]][3], fr[h["cand"]["slot"]][h["cand"]["id"]][3], h["cand"]["shift"], rwc.UP) for h in r["hyp"]]
    icp = c.loop_icp_from([(src_of[h["query"]], h["spec"]) for h in r["hyp"]], T0, prm.icp)
    table = []
    for h, i in zip(r["hyp"], icp):
        h["target"], h["icp"] = infos[h.pop("spec")], i
        h["admissible"] = int(i["status"] == 0 and bool(np.isfinite(i["fitness"])) and host.loop_accept(i["converged"], i["fitness"], prm.max_fitness))
        table.append(dict(X=i["transform"] if h["admissible"] else np.zeros((4, 4)), p=np.asarray(fr[slot][qid[h["query"]]][3][:3], np.float64),
                          fitness=i["fitness"] if h["admissible"] else 0.0, query=h["query"], rank=h["rank"], target_slot=h["cand"]["slot"],
                          admissible=h["admissible"]))
    v = host.rendezvous_consensus(table)
    r.update(winner=v["winner"], support=v["support"], n_admissible=v["n_admissible"], members=v["members"])
    for i in v["members"]:
        r["hyp"][i]["member"] = 1
    r["outcome"] = REJECTED if v["winner"] < 0 else (UNCONFIRMED if v["support"] < min_support else FOUND)
    if r["outcome"] == FOUND:
        w = r["hyp"][v["winner"]]
        r.update(target_slot=w["cand"]["slot"], target_id=w["cand"]["id"], X=w["icp"]["transform"])
    return r


def step(c, entries, prm, targets=TARGETS, consensus=None, **kw):
    kw.setdefault("shortlist", rwc.M), kw.setdefault("k", rwc.K)
    return team.rendezvous_window_step(c, [(s, rwc.NOW) for s in entries], targets, prm, consensus, **kw)


def lone(c, entries, prm, targets=TARGETS):
    return team.rendezvous_step(c, [(s, rwc.NOW) for s in entries], targets, prm, shortlist=rwc.M, k=rwc.K)


@pytest.fixture(scope="module")
def pair(pkg, ieskf):
    a, b = context(pkg, ieskf), context(pkg, ieskf)
    yield a, b
    a.close(), b.close()


@pytest.fixture(scope="module")
def results(pair, ieskf):
    """the step over all four slots on context a (with the state before and after), the explicit chains on context b — computed once"""
    a, b = pair
    prm = params(ieskf)
    before = state(a)
    got = step(a, [3, 1, 2, 0], prm)
    after = state(a)
    assert isinstance(got, list)
    return dict(got={s: g for s, g in zip([3, 1, 2, 0], got)}, want={s: chain(b, s, prm) for s in ALL}, before=before, after=after, prm=prm)


def test_the_step_is_the_explicit_chain_in_any_batch_and_order(pair, results):
    a, _ = pair
    got, want, prm = results["got"], results["want"], results["prm"]
    for s in ALL:
        assert lsc.frozen(got[s]) == lsc.frozen(want[s]), s
    print("outcomes:", {s: (got[s]["outcome"], got[s]["target_slot"], got[s]["target_id"], got[s]["n_hypotheses"], got[s]["n_admissible"], got[s]["support"]) for s in ALL})
    for batch in ([1], [3], [1, 3]):
        assert lsc.frozen(step(a, batch, prm)) == lsc.frozen([got[s] for s in batch]), batch
    # after other calls on the context, with the targets in another order
    assert isinstance(a.place_search([(0, 3, 1, 3.0, -1.0)] * 5), list)
    a.archive_assemble([dict(slot=2, ids=[0, 1], clouds=7, leaf=0.4, flags=0)])
    assert lsc.frozen(step(a, [3, 1], prm, targets=[2, 0, 1])) == lsc.frozen([got[3], got[1]])
    assert step(a, [], prm) == []


def test_other_windows_take_other_paths(pair, ieskf):
    a, b = pair
    prm = params(ieskf)
    for kw in (dict(window=8, stride=2, min_support=2), dict(window=16, stride=1, min_support=16), dict(window=2, stride=7, min_support=1)):
        got = step(a, [1, 3], prm, consensus=kw)
        assert lsc.frozen(got) == lsc.frozen([chain(b, s, prm, **kw) for s in (1, 3)]), kw
    assert [len(g["query_id"]) for g in step(a, [1], prm, consensus=dict(window=16, min_support=1))] == [12]  # (only the frames that exist ask)
    assert step(a, [1], prm, consensus=dict(window=2, stride=7, min_support=1))[0]["query_id"] == [11, 4]
    # a gate that drops every rank: NONE, nothing aligned; a target list of the asking slot alone: its own frames never count
    for g in step(a, [1, 3], prm, max_distance=0.0) + step(a, [1], prm, targets=[1]):
        assert (g["outcome"], g["n_hypotheses"], g["hyp"], g["n_queries"]) == (NONE, 0, [], 5)
    assert lsc.frozen(step(a, [1], prm, targets=[1, 0])) == lsc.frozen([chain(b, 1, prm, targets=[1, 0])])


def test_a_window_of_one_is_the_lone_frame_step(pair, ieskf):
    a, _ = pair
    prm = params(ieskf)
    for s in ALL:
        targets = [t for t in TARGETS if t != s]
        one, old = step(a, [s], prm, targets, consensus=dict(window=1, min_support=1))[0], lone(a, [s], prm, targets)[0]
        assert (one["outcome"], one["target_slot"], one["target_id"], one["X"].tobytes()) == (old["outcome"], old["target_slot"], old["target_id"], old["X"].tobytes()), s
        assert one["n_hypotheses"] == old["n_candidates"] and lsc.frozen([h["icp"] for h in one["hyp"]]) == lsc.frozen(old["icp"]) and one["winner"] == old["chosen"]


def test_slot_3_is_found_by_one_frame_and_unconfirmed_by_five(pair, results):
    a, _ = pair
    old = lone(a, [3], results["prm"])[0]
    assert old["outcome"] == FOUND and old["target_slot"] in (0, 1)  # the mistake: a rebase into a map it never saw
    g = results["got"][3]
    print("slot 3:", [(g["query_id"][h["query"]], h["cand"]["slot"], h["cand"]["id"], h["admissible"], h["icp"]["fitness"]) for h in g["hyp"]])
    assert (g["outcome"], g["status"], g["support"], g["target_slot"], g["target_id"]) == (UNCONFIRMED, 0, 1, -1, -1) and not g["X"].any()
    # the caller sees why: every hypothesis is reported, the admissible ones are those of frames 9 and 11, and the winner stands alone
    assert g["n_hypotheses"] == len(g["hyp"]) == sum(g["n_ranks"]) and g["query_id"] == [11, 10, 9, 8, 7]
    assert {g["query_id"][h["query"]] for h in g["hyp"] if h["admissible"]} == {9, 11} and g["n_admissible"] == sum(h["admissible"] for h in g["hyp"])
    assert g["members"] == [g["winner"]] and [h["member"] for h in g["hyp"]] == [int(i == g["winner"]) for i in range(len(g["hyp"]))]
    assert all(h["icp"]["iterations"] > 0 and h["target"]["n"] > 0 for h in g["hyp"])


def test_slot_1_is_found_in_slot_0_by_all_five_frames(results):
    g = results["got"][1]
    w = g["hyp"][g["winner"]]
    e = rc.origin_error(g["X"], g["query_id"][w["query"]])
    print("slot 1: winner frame %d, fitness %.4f, support %d, origin error %.4f m (bound %.4f m)" % (g["query_id"][w["query"]], w["icp"]["fitness"], g["support"], e, plc.bound()[0]))
    assert (g["outcome"], g["status"], g["target_slot"], g["support"]) == (FOUND, 0, 0, 5)
    assert g["target_id"] == w["cand"]["id"] and g["X"].tobytes() == w["icp"]["transform"].tobytes()
    assert sorted(g["query_id"][g["hyp"][i]["query"]] for i in g["members"]) == [7, 8, 9, 10, 11]
    assert e <= plc.bound()[0]
    assert np.abs(g["X"] - rc.G()).max() < 0.1


def test_slot_2_is_rejected(results):
    g = results["got"][2]
    assert (g["outcome"], g["status"], g["winner"], g["n_admissible"], g["members"]) == (REJECTED, 0, -1, 0, []) and g["n_hypotheses"] > 0


def test_an_assembly_status_stops_its_entries_and_no_other(pair, results):
    """A frame of target slot 0 that no hypothesis names and no entry asks from — its pose feeds neither the search nor a
    guess — stored so far away that its points leave |coord| <= 1e6: every window that holds it assembles to LINS_E_INPUT
    and an empty cloud.  The entries with such a window stop with that status, nothing aligned; the others are the
    unspoiled run's bytes."""
    a, _ = pair
    got, prm = results["got"], results["prm"]
    t = 0
    named = {h["cand"]["id"] for s in ALL for h in got[s]["hyp"] if h["cand"]["slot"] == t} | set(got[t]["query_id"])

    def holds(h, f):
        return h["cand"]["slot"] == t and f in host.loop_window(LATEST, h["cand"]["id"], rwc.H)

    far, hit = next((f, hit) for f in range(N) if f not in named
                    for hit in [[s for s in ALL if any(holds(h, f) for h in got[s]["hyp"])]] if 0 < len(hit) < len(ALL))
    print("far frame: slot %d frame %d; entries that reach it: %s" % (t, far, hit))
    a.archive_set_poses(t, far, [(1.0e6, 0.0, 0.0, 0.0, 0.0, 0.0)])
    try:
        res = dict(zip([3, 1, 2, 0], step(a, [3, 1, 2, 0], prm)))
    finally:
        a.archive_set_poses(t, far, [tuple(float(v) for v in rwc.slots()[t][far][3])])
    zero_icp = lsc.frozen(defs.LoopIcpResultC().as_dict())
    for s in ALL:
        g, u = res[s], got[s]
        if s not in hit:
            assert lsc.frozen(g) == lsc.frozen(u), s
            continue
        assert (g["outcome"], g["status"], g["winner"], g["support"], g["n_admissible"], g["target_slot"], g["target_id"], g["members"]) == (NONE, E_INPUT, -1, 0, 0, -1, -1, []), s
        assert not g["X"].any() and g["n_hypotheses"] == u["n_hypotheses"] > 0
        assert lsc.frozen([g[k] for k in ("n_queries", "query_id", "n_ranks", "source")]) == lsc.frozen([u[k] for k in ("n_queries", "query_id", "n_ranks", "source")])
        for h, w in zip(g["hyp"], u["hyp"]):
            assert lsc.frozen([h[k] for k in ("query", "rank", "cand")]) == lsc.frozen([w[k] for k in ("query", "rank", "cand")])
            assert lsc.frozen(h["icp"]) == zero_icp and (h["admissible"], h["member"]) == (0, 0)  # no hypothesis was aligned
            if holds(h, far):
                assert (h["target"]["status"], h["target"]["n"]) == (E_INPUT, 0)
            else:
                assert lsc.frozen(h["target"]) == lsc.frozen(w["target"])
    assert state(a) == results["before"]  # (the frame's pose is back)


def test_the_step_leaves_graphs_archive_rings_and_map_poses(results):
    assert results["after"] == results["before"]


def test_refusals_change_nothing(pkg, ieskf, pair):
    a, _ = pair
    prm = params(ieskf)
    before = state(a)
    want = lone(a, ALL, prm)
    for entries, targets in (([0, 0], TARGETS), ([4], TARGETS), ([-1], TARGETS), ([0], [0, 0]), ([0], [4])):
        assert step(a, entries, prm, targets) == E_ARG, (entries, targets)
    for kw in (dict(shortlist=0), dict(k=9), dict(min_sep=-2), dict(max_distance=float("nan"))):
        assert step(a, ALL, prm, **kw) == E_ARG, kw
    assert step(a, ALL, params(ieskf, search_num=-1)) == E_ARG and step(a, ALL, params(ieskf, history_leaf=-1.0)) == E_ARG
    for kw in (dict(window=0), dict(window=17), dict(stride=0), dict(min_support=0), dict(window=4, min_support=5), dict(max_translation=-1.0),
               dict(max_translation=float("inf")), dict(min_cos_rotation=float("nan"))):
        assert step(a, ALL, prm, consensus=kw) == E_ARG, kw
    assert team.rendezvous_window_step(a, [(0, rwc.NOW), (1, float("inf"))], TARGETS, prm, shortlist=rwc.M, k=rwc.K) == E_INPUT
    assert lsc.frozen(lone(a, ALL, prm)) == lsc.frozen(want) and state(a) == before
    c = context(pkg, ieskf, place=False)
    assert step(c, ALL, prm) == E_STATE  # before lins_place_init
    c.close()


def test_the_windows_X_rebases_slot_1_and_the_next_map_step_runs_in_team_mode(pkg, ieskf):
    c = context(pkg, ieskf)
    g = step(c, [1], params(ieskf))[0]
    assert g["outcome"] == FOUND
    assert team.rebase(c, [1], [np.asarray(g["X"], np.float64).reshape(4, 4)], streams=[1]) == 0
    assert sm.team(c, True, 50.0, 0.02) == 0 and sm.team_groups(c, [0, 1], [0, 0]) == 0
    st, cov = np.zeros((4, 19)), np.stack([host.synth_pair(0).cov] * 4)
    st[:, 6] = 1.0
    c.streams_step_raw([host.synth_seq_raw_scan(70 + i, 0) for i in range(4)], st, cov)
    pose = sm.get_pose(c, 1)
    res = sm.step(c, [1], [sm.odom(pose["bef"], float(LATEST) + 1.0)])[0]  # transformSum = transformBefMapped: the scan starts at the rebased pose
    print("map step on the rebased stream:", {k: res[k] for k in ("status", "iters", "converged", "n_sel", "key_frame")}, "team list slots:", sorted({s for s, _ in sm.team_list(c, 1)}))
    assert res["status"] == 0
    c.close()
