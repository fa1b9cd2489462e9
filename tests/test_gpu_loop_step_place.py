"""lins_loop_step_place (include/lins_place.h): the loop thread's step with its loops detected by appearance, on the
fixture of tests/place_verify_cases.py, where the descriptor's winner is the wrong place (tests/test_place_verify_inputs.py
asserts the fixture on the CPU).  The step shortlists (7, 1), verifies both by ICP in one batch, chooses rank 1 by its
fitness and closes the loop onto frame 1; the top-1 chain of tests/test_gpu_place_loop.py closes the same fixture onto
frame 7, 15 m wrong.  Every entry's bits and the state it leaves are those of the explicit chain for its slot, in any
batch and order.

The position bound.  The step weighs its factor as lins_loop_step does, by the reference's rule: the variance is the
ICP's fitness (~0.05) against 1e-6 per odometry factor, and the solve then leaves the last frame where odometry put it
(tests/place_loop_cases.py LOOP_VARIANCE has the figures; measured here on the device: 7.137 m from the truth, printed
by the first test).  The bound of place_loop_cases.bound() is therefore asserted as the CPU test asserts it: the step's
chosen loop — its closest_id and pose_from — solved with LOOP_VARIANCE on the device.  Measured: 0.118 m on the device
and on the CPU restatement, against the bound of 0.210 m; the top-1 chain ends 15.83 m off."""
import numpy as np
import pytest

import loop_icp_cases as licp
import loop_step_cases as lsc
import place_loop_cases as plc
import place_verify_cases as pvc

pytestmark = pytest.mark.gpu
host, defs = pvc.host, lsc.defs
N, LATEST = pvc.N, pvc.N - 1
E_ARG, E_STATE = -1, -6
ZERO = (0.0, 0.0, 0.0)


def params(ieskf, **kw):
    return lsc.params(ieskf.lib(), search_radius=pvc.RADIUS, min_gap_s=pvc.GAP, search_num=pvc.H, **kw)


def place_params(ieskf, **kw):
    return defs.loop_place_params(ieskf.lib(), **kw)


def pose_case():
    """(frames, centre): the 12-frame archive case of loop_icp_cases and a centre at which the pose search has a candidate"""
    frames, _, wrong, _ = licp.archive_case()
    poses, times = np.array([f[3] for f in frames]), np.arange(12.0)
    near = host.find_loop(poses, times, wrong[:3], 7.0, pvc.NOW, 5.0)
    assert near >= 0
    centre = frames[near][3][:3]
    assert host.find_loop(poses, times, centre, pvc.RADIUS, pvc.NOW, pvc.GAP) >= 0
    return frames, centre


def kinds():
    """name -> (frames, times, centre)"""
    frames, true, wrong = pvc.case()
    pf, pc_ = pose_case()
    return dict(verify=(frames, [float(i) for i in range(N)], wrong[:3]),
                none=(frames, [pvc.NOW - 0.2 * (LATEST - i) for i in range(N)], wrong[:3]),  # every frame within the gap
                pose=(pf, [float(i) for i in range(12)], pc_),
                plain=(plc.case()[0], [float(i) for i in range(N)], plc.case()[2][:3]))


def context(pkg, ieskf, names, place=True, graph_slots=0):
    """slot s holds kind names[s] in archive and graph; graph_slots more slots exist, empty"""
    n = len(names) + graph_slots
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=n, max_targets=1024)
    K = kinds()
    c.archive_init(n, 16, sum(sum(len(f[0]) + len(f[1]) + len(f[2]) for f in K[k][0]) for k in names) + 16)
    c.pose_graph_init(n, 16, 2)
    if place:
        assert c.place_init(up_axis=pvc.UP) == 0
    for s, k in enumerate(names):
        fr, t, _ = K[k]
        for i, f in enumerate(fr):
            assert c.archive_push(s, *f, time=t[i]) == c.pose_graph_push(s, plc.six_of_key(fr[i - 1][3]) if i else None, plc.six_of_key(f[3])) == i
    return c


def entry(slot, kind):
    return defs.loop_step_entry(slot, kinds()[kind][2], pvc.NOW)


def state(c, slot):
    """what a step leaves in graph and archive for a slot, as bytes (the archive's key poses through an assembly of every frame)"""
    n, loops = c.pose_graph_count(slot)
    c.archive_assemble([dict(slot=slot, ids=list(range(n)), clouds=7, leaf=0.0, flags=0)])
    return (n, loops, c.debug_pose_graph_poses_f64(slot).tobytes(), c.pose_graph_poses(slot).tobytes(),
            [c.debug_pose_graph_loop_z(slot, l).tobytes() for l in range(loops)], c.archive_download(0).tobytes())


def chain(c, slot, kind, prm, k, min_sep, last_pair=(-1, -1)):
    """the explicit chain for one slot, by appearance -> the dict lins_loop_step_place gives for its entry"""
    stored = [f[3] for f in kinds()[kind][0]]
    r = dict(step=lsc.result_zero(), detect=1, n_candidates=0, chosen=-1, cand=[], icp=[])
    st = r["step"]
    latest = st["latest_id"] = c.archive_count(slot) - 1
    ranks = c.place_topk([(slot, latest, slot, pvc.NOW, prm.min_gap_s)], k, min_sep)[0]
    what = [host.loop_candidate(latest, x["id"], *last_pair) for x in ranks]
    r["cand"] = [x for x, w in zip(ranks, what) if w == -1]
    r["n_candidates"] = len(r["cand"])
    if not r["cand"]:
        st["outcome"] = defs.LOOP_REPEAT if defs.LOOP_REPEAT in what else defs.LOOP_NONE
        return r
    infos = c.archive_assemble([dict(slot=slot, ids=[latest], clouds=3, leaf=0.0, flags=1)] +
                               [dict(slot=slot, ids=host.loop_window(latest, x["id"], prm.search_num), clouds=3, leaf=prm.history_leaf, flags=0)
                                for x in r["cand"]])
    st["latest"] = infos[0]
    T0 = [host.place_guess(stored[latest], stored[x["id"]], x["shift"], pvc.UP) for x in r["cand"]]
    r["icp"] = c.loop_icp_from([(0, 1 + j) for j in range(len(T0))], T0, prm.icp)
    st["outcome"] = defs.LOOP_REJECTED
    j = r["chosen"] = host.loop_choose([i["converged"] for i in r["icp"]], [i["fitness"] for i in r["icp"]], prm.max_fitness)
    if j < 0:
        return r
    st["closest_id"], st["history"], st["icp"] = r["cand"][j]["id"], infos[1 + j], r["icp"][j]
    if not host.loop_variance(st["icp"]["fitness"])[0]:
        return r
    st["pose_from"] = host.loop_pose_from(st["icp"]["transform"], c.pose_graph_poses(slot, latest, 1)[0])
    c.pose_graph_add_loop(slot, latest, st["closest_id"], st["pose_from"], st["icp"]["fitness"])
    st["graph"] = c.pose_graph_solve([slot], prm.graph)[0]
    c.pose_graph_apply(slot, -1)
    st["outcome"] = defs.LOOP_CLOSED
    return r


def off_truth(pose, true):
    return float(np.linalg.norm(np.asarray(pose[:3], np.float64) - true[:3]))


def test_the_step_verifies_the_shortlist_and_closes_the_right_loop(pkg, ieskf):
    frames, true, wrong = pvc.case()
    prm, pl = params(ieskf), place_params(ieskf)
    assert (pl.mode, pl.k, pl.min_sep, pl.max_distance) == (defs.LOOP_DETECT_PLACE, 4, -1, 1.0)  # min_sep -1: search_num = 4 here
    a, b = context(pkg, ieskf, ["verify"]), context(pkg, ieskf, ["verify"], graph_slots=1)
    assert a.archive_find_loop(0, wrong[:3], pvc.RADIUS, pvc.NOW, pvc.GAP) == -1
    got = a.loop_step_place([entry(0, "verify")], prm, pl)[0]
    st = got["step"]
    print("ranks:", [(x["id"], x["shift"], float(x["distance"])) for x in got["cand"]], "fitness:", [i["fitness"] for i in got["icp"]])
    assert (st["outcome"], got["detect"], got["n_candidates"], got["chosen"], st["closest_id"]) == (defs.LOOP_CLOSED, 1, 2, 1, pvc.REVISITED)
    assert [x["id"] for x in got["cand"]] == [pvc.TWIN, pvc.REVISITED]
    assert a.loop_step_stats()["closed"] == 1 and a.loop_step_stats()["aligned"] == 1
    cloud = a.loop_closed_cloud(0)
    assert len(cloud) == st["latest"]["n"] > 0
    # bit for bit the explicit chain, and the state it leaves
    want = chain(b, 0, "verify", prm, pvc.K, pvc.MIN_SEP)
    assert lsc.frozen(got) == lsc.frozen(want)
    assert state(a, 0) == state(b, 0)
    # the host restatement agrees on what was decided
    hc = pvc.host_chain()
    assert [(x["id"], x["shift"], x["distance"].tobytes()) for x in got["cand"]] == [(x["id"], x["shift"], x["distance"].tobytes()) for x in hc["ranks"]]
    assert got["icp"][1]["fitness"] < got["icp"][0]["fitness"] <= pvc.MAX_FITNESS and hc["chosen"] == 1
    # the position bound (the module's docstring): the chosen loop weighed with LOOP_VARIANCE, on the device
    own = off_truth(a.pose_graph_poses(0, LATEST, 1)[0], true)
    for i, f in enumerate(frames):
        assert b.pose_graph_push(1, plc.six_of_key(frames[i - 1][3]) if i else None, plc.six_of_key(f[3])) == i
    b.pose_graph_add_loop(1, LATEST, st["closest_id"], st["pose_from"], plc.LOOP_VARIANCE)
    assert b.pose_graph_solve([1])[0]["iterations"] > 0
    err = off_truth(b.pose_graph_poses(1, LATEST, 1)[0], true)
    left, bound = plc.bound()
    print("last frame from its true position: %.3f m with the loop weighed by LOOP_VARIANCE (bound %.3f m); %.3f m as the step "
          "leaves it with the reference's variance = fitness" % (err, bound, own))
    assert err <= bound
    a.close(), b.close()


def test_the_top1_chain_closes_the_wrong_loop(pkg, ieskf):
    """the chain of tests/test_gpu_place_loop.py on this fixture: what a caller had before lins_loop_step_place"""
    frames, true, wrong = pvc.case()
    c = context(pkg, ieskf, ["verify"])
    found = c.place_search([(0, LATEST, 0, pvc.NOW, pvc.GAP)])[0]
    assert found["id"] == pvc.TWIN
    T0 = host.place_guess(wrong, frames[found["id"]][3], found["shift"], pvc.UP)
    c.archive_assemble([dict(slot=0, ids=[LATEST], clouds=3, leaf=0.0, flags=1),
                        dict(slot=0, ids=plc.window(found["id"], LATEST), clouds=3, leaf=0.4, flags=0)])
    icp = c.loop_icp_from([(0, 1)], [T0])[0]
    assert icp["converged"] == 1 and icp["fitness"] <= pvc.MAX_FITNESS and host.loop_accept(icp["converged"], icp["fitness"], pvc.MAX_FITNESS)  # LM:1140 passes it
    pose_from = host.loop_pose_from(icp["transform"], c.pose_graph_poses(0, LATEST, 1)[0])
    c.pose_graph_add_loop(0, LATEST, found["id"], pose_from, plc.LOOP_VARIANCE)
    c.pose_graph_solve([0])
    err = off_truth(c.pose_graph_poses(0, LATEST, 1)[0], true)
    print("top-1: closed onto frame %d at fitness %.3f; the last frame ends %.2f m from its true position" % (found["id"], icp["fitness"], err))
    assert err > 10.0
    c.close()
    # and the step itself with k = 1 is that pipeline: it closes onto the twin
    c = context(pkg, ieskf, ["verify"])
    got = c.loop_step_place([entry(0, "verify")], params(ieskf), place_params(ieskf, k=1))[0]
    assert (got["step"]["outcome"], got["n_candidates"], got["chosen"], got["step"]["closest_id"]) == (defs.LOOP_CLOSED, 1, 0, pvc.TWIN)
    c.close()


def test_a_batch_in_both_orders_equals_its_singles(pkg, ieskf):
    names = ["verify", "none", "pose"]
    prm, pl = params(ieskf), place_params(ieskf, mode=defs.LOOP_DETECT_POSE_THEN_PLACE)
    ent = [entry(s, k) for s, k in enumerate(names)]
    fwd, rev, one, step = (context(pkg, ieskf, names) for _ in range(4))
    a = fwd.loop_step_place(ent, prm, pl)
    b = rev.loop_step_place(ent[::-1], prm, pl)[::-1]
    singles = [one.loop_step_place([e], prm, pl)[0] for e in ent]
    assert lsc.frozen(a) == lsc.frozen(b) == lsc.frozen(singles)
    for s in range(3):
        assert state(fwd, s) == state(rev, s) == state(one, s), names[s]
    assert (a[0]["step"]["outcome"], a[0]["detect"], a[0]["chosen"], a[0]["step"]["closest_id"]) == (defs.LOOP_CLOSED, 1, 1, pvc.REVISITED)
    assert (a[1]["step"]["outcome"], a[1]["detect"], a[1]["n_candidates"], a[1]["step"]["closest_id"], a[1]["cand"]) == (defs.LOOP_NONE, 1, 0, -1, [])
    # the slot whose pose search has a candidate is lins_loop_step's entry, bit for bit, and leaves its state
    want = step.loop_step([ent[2]], prm)[0]
    assert a[2]["detect"] == 0 and want["closest_id"] >= 0 and want["outcome"] in (defs.LOOP_REJECTED, defs.LOOP_CLOSED)
    assert lsc.frozen(a[2]["step"]) == lsc.frozen(want) and state(fwd, 2) == state(step, 2)
    assert a[2]["n_candidates"] == 1 and a[2]["cand"][0]["id"] == want["closest_id"] and lsc.frozen(a[2]["icp"][0]) == lsc.frozen(want["icp"])
    for c in (fwd, rev, one, step):
        c.close()


def test_a_second_step_with_the_same_pair_is_a_repeat(pkg, ieskf):
    """place_loop_cases' own fixture, where the revisited frame leads: k = 1 closes (11, 1); nothing new arrives, the same
    search returns the same pair, and the step neither aligns nor adds"""
    c = context(pkg, ieskf, ["plain"])
    prm, pl = params(ieskf), place_params(ieskf, k=1)
    first = c.loop_step_place([entry(0, "plain")], prm, pl)[0]
    assert (first["step"]["outcome"], first["step"]["closest_id"]) == (defs.LOOP_CLOSED, plc.REVISITED)
    before = state(c, 0)
    again = c.loop_step_place([entry(0, "plain")], prm, pl)[0]
    assert (again["step"]["outcome"], again["n_candidates"], again["chosen"], again["cand"], again["icp"]) == (defs.LOOP_REPEAT, 0, -1, [], [])
    assert c.loop_step_stats()["candidates"] == 0 and state(c, 0) == before
    c.close()


def test_refusals_change_nothing(pkg, ieskf):
    prm = params(ieskf)
    c = context(pkg, ieskf, ["none"], place=False)
    e = [entry(0, "none")]
    before = c.pose_graph_poses(0).tobytes()
    assert c.loop_step_place(e, prm, place_params(ieskf)) == E_STATE  # before lins_place_init
    assert c.place_init(up_axis=pvc.UP) == 0
    for bad in (dict(k=0), dict(k=9), dict(mode=2), dict(mode=-1), dict(min_sep=-2), dict(max_distance=float("nan"))):
        assert c.loop_step_place(e, prm, place_params(ieskf, **bad)) == E_ARG, bad
    assert c.loop_step_place(e + e, prm, place_params(ieskf)) == E_ARG  # a slot named twice: lins_loop_step's refusal
    assert c.loop_step_place([defs.loop_step_entry(0, ZERO, float("inf"))], prm, place_params(ieskf)) == -4
    assert c.place_stats()["frames_built"] == 0  # nothing was queued: no frame was described
    assert c.pose_graph_poses(0).tobytes() == before and c.pose_graph_count(0) == (N, 0)
    got = c.loop_step_place(e, prm, place_params(ieskf))[0]
    assert got["step"]["outcome"] == defs.LOOP_NONE and c.place_stats()["frames_built"] == N
    assert c.loop_step_place([], prm, place_params(ieskf)) == []
    c.close()
