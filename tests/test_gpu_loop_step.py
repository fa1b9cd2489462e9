"""lins_loop_step — performLoopClosure + correctPoses for n slots in one call — against the explicit seven-call chain a
caller had to write before it (tests/loop_step_cases.py explicit_chain) on a second context: every result field and the
state the step leaves in the graph, the archive and the ring, bit for bit; the repeat and rejection branches, batch
independence, the loop capacity, the errors, and the closed cloud.  tests/test_loop_step_inputs.py asserts on the CPU that
the set-up takes the branches these tests mean."""
import numpy as np
import pytest

import loop_step_cases as lsc
import pose_graph_cases as cases

pytestmark = pytest.mark.gpu
defs, host = lsc.defs, lsc.host
KINDS = ("loop", "inside", "loop")  # slot 0 and 2: the archive case; slot 1: every time inside the gap, no candidate
CLOSED, NONE, REPEAT, REJECTED = defs.LOOP_CLOSED, defs.LOOP_NONE, defs.LOOP_REPEAT, defs.LOOP_REJECTED


@pytest.fixture(scope="module")
def pair(pkg, ieskf):
    a = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    b = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    yield a, b
    a.close()
    b.close()


def fresh(c, n_slots=3, kinds=KINDS, max_loops=lsc.MAX_LOOPS):
    lsc.init(c, n_slots, max_loops)
    for s, kind in enumerate(kinds):
        lsc.push(c, s, kind)


def entries(slots):
    return [(s, lsc.centre(), lsc.NOW) for s in slots]


def states(c, slots=(0, 1, 2)):
    scan = lsc.build_scan()
    return {s: lsc.state_of(c, s, scan) for s in slots}


@pytest.fixture(scope="module")
def ref(pair, ieskf):
    """one step over the three slots on context A, the chain slot by slot on context B, both from freshly pushed state"""
    a, b = pair
    prm = lsc.params(ieskf.lib())
    fresh(a)
    step = [lsc.frozen(r) for r in a.loop_step(entries([0, 1, 2]), prm)]
    stats = a.loop_step_stats()
    step_states = states(a)
    fresh(b)
    raw = [lsc.explicit_chain(b, s, lsc.centre(), lsc.NOW, prm) for s in range(3)]
    return dict(step=step, step_states=step_states, chain=[lsc.frozen(r) for r in raw], chain_states=states(b), raw=raw, stats=stats)


def test_step_equals_the_explicit_chain(ref):
    raw = ref["raw"]
    assert [r["outcome"] for r in raw] == [CLOSED, NONE, CLOSED]
    for s in range(3):
        assert ref["step"][s] == ref["chain"][s], (s, raw[s])
        assert ref["step_states"][s] == ref["chain_states"][s], s
    r = raw[0]
    assert r["latest_id"] == 11 and 0 <= r["closest_id"] <= 5 and r["status"] == 0
    assert r["icp"]["converged"] == 1 and r["icp"]["fitness"] <= 0.3 and r["graph"]["iterations"] > 0 and r["graph"]["cost_after"] < r["graph"]["cost_before"]
    assert r["latest"]["n"] > 0 and r["history"]["n"] > 0 and r["history"]["frames"] == len(host.loop_window(11, r["closest_id"], lsc.H))
    # the entry without a candidate: nothing ran for it, its fields are zero and its history keeps the pushed bits
    want = lsc.result_zero()
    want["latest_id"] = 11
    assert ref["step"][1] == lsc.frozen(want)
    assert ref["step_states"][1][:2] == (12, 0)
    assert ref["step_states"][0][:2] == (12, 1) and ref["step_states"][0] == ref["step_states"][2]  # the same case in two slots
    assert ref["step_states"][0][2:] != ref["step_states"][1][2:]  # ... and the solve moved it
    assert ref["stats"]["candidates"] == ref["stats"]["aligned"] == ref["stats"]["closed"] == 2
    assert ref["stats"]["assemble_ms"] > 0 and ref["stats"]["icp_ms"] > 0 and ref["stats"]["solve_ms"] > 0


def test_the_same_call_again_is_a_repeat(pair, ieskf):
    a, _ = pair
    prm = lsc.params(ieskf.lib())
    fresh(a)
    first = a.loop_step(entries([0, 1, 2]), prm)
    before = states(a)
    again = a.loop_step(entries([0, 1, 2]), prm)
    assert [r["outcome"] for r in again] == [REPEAT, NONE, REPEAT]
    for s in (0, 2):
        want = lsc.result_zero()
        want.update(outcome=REPEAT, latest_id=11, closest_id=first[s]["closest_id"])
        assert lsc.frozen(again[s]) == lsc.frozen(want)
    assert states(a) == before  # loop counts, poses, the archive's and the ring's clouds
    assert a.loop_step_stats()["candidates"] == 0
    assert [before[s][1] for s in range(3)] == [1, 0, 1]


def test_rejection_leaves_the_graph_alone(pair, ieskf, ref):
    a, _ = pair
    fresh(a)
    before = states(a)
    res = a.loop_step(entries([0, 1, 2]), lsc.params(ieskf.lib(), max_fitness=0.0))
    assert [r["outcome"] for r in res] == [REJECTED, NONE, REJECTED]
    r = res[0]
    assert r["status"] == 0 and r["icp"]["converged"] == 1 and r["icp"]["fitness"] > 0.0 and r["icp"]["iterations"] > 0
    assert lsc.frozen(r["icp"]) == lsc.frozen(ref["raw"][0]["icp"])  # the alignment is the accepted one's
    assert lsc.frozen(r["graph"]) == lsc.frozen(lsc.result_zero()["graph"]) and not r["pose_from"].any()
    assert states(a) == before and all(before[s][1] == 0 for s in range(3))


def test_an_entrys_bits_do_not_depend_on_its_batch(pair, ieskf, ref):
    a, _ = pair
    prm = lsc.params(ieskf.lib())

    def run(groups, n_slots=3, before=None):
        fresh(a, n_slots)
        if before:
            before(a)
        res = {}
        for grp in groups:
            for s, r in zip(grp, a.loop_step(entries(grp), prm)):
                res[s] = lsc.frozen(r)
        return [res[s] for s in range(3)], states(a)

    want = (ref["step"], ref["step_states"])
    assert run([[2, 1, 0]]) == want
    assert run([[0], [1], [2]]) == want
    assert run([[1, 2], [0]]) == want

    def unrelated(c):  # another slot's graph with a loop, solved; an alignment of host clouds
        aft = cases.host_cases()[2]["aft"][:lsc.MAX_FRAMES]
        for k in range(len(aft)):
            c.pose_graph_push(3, aft[k - 1] if k else None, aft[k])
        c.pose_graph_add_loop(3, 14, 2, cases.corrected(aft[14], 0.3, 2.0, 9), 1e-6)
        assert c.pose_graph_solve([3])[0]["iterations"] > 0
        f = lsc.frames()
        c.loop_icp([(f[3][1], f[4][1])])

    got = run([[0, 1, 2]], n_slots=4, before=unrelated)
    assert got[0] == want[0]
    # (the archive's arena is sized for four slots here: the frames lie where they lay, the clouds are the same bits)
    assert got[1] == want[1]


def test_a_full_slot_reports_capacity_and_the_others_close(pair, ieskf, ref):
    a, _ = pair
    fresh(a, kinds=("loop", "loop", "loop"), max_loops=1)
    aft = lsc.six_of_key(lsc.frames()[10][3])
    a.pose_graph_add_loop(1, 10, 2, cases.corrected(aft, 0.05, 0.5, 3), 1e-6)  # slot 1 holds its one loop: another pair than the candidate's
    before = states(a, [1])
    res = a.loop_step(entries([0, 1, 2]), lsc.params(ieskf.lib()))
    assert [(r["outcome"], r["status"]) for r in res] == [(CLOSED, 0), (NONE, -3), (CLOSED, 0)]
    want = lsc.result_zero()
    want.update(status=-3, latest_id=11, closest_id=res[0]["closest_id"])
    assert lsc.frozen(res[1]) == lsc.frozen(want)
    assert states(a, [1]) == before and a.pose_graph_count(1) == (12, 1)
    assert lsc.frozen(res[0]) == ref["step"][0] and lsc.frozen(res[2]) == ref["step"][2]


def test_an_assembly_status_stops_its_entry_and_the_others_close(pair, ieskf, ref):
    """A frame of slot 0's history window — not the candidate, whose pose the search reads — stored so far away that its
    points leave |coord| <= 1e6: the window's assembly reports LINS_E_INPUT and an empty cloud.  The entry stops there
    with that status; its neighbours in the call are what they are alone."""
    a, b = pair
    prm = lsc.params(ieskf.lib())
    closest = ref["raw"][0]["closest_id"]
    far = closest + 1  # inside the window (H = 4), neither the candidate nor the latest frame
    assert 0 <= closest < far < 11 and far in host.loop_window(11, closest, lsc.H)
    fresh(b)
    single = {s: lsc.frozen(b.loop_step(entries([s]), prm)[0]) for s in (1, 2)}
    single_states = states(b, [1, 2])
    fresh(a)
    a.archive_set_poses(0, far, [(1.0e6, 0.0, 0.0, 0.0, 0.0, 0.0)])
    before = states(a, [0])
    res = a.loop_step(entries([0, 1, 2]), prm)
    stats = a.loop_step_stats()
    r = res[0]
    print("entry 0:", {k: r[k] for k in ("outcome", "status", "latest_id", "closest_id", "latest", "history")})
    assert (r["outcome"], r["status"], r["latest_id"], r["closest_id"]) == (NONE, -4, 11, closest)
    assert r["latest"]["status"] == 0 and r["latest"]["n"] > 0 and (r["history"]["status"], r["history"]["n"]) == (-4, 0)
    zero = lsc.result_zero()
    assert all(lsc.frozen(r[k]) == lsc.frozen(zero[k]) for k in ("icp", "pose_from", "graph"))  # nothing was aligned or solved for it
    assert (stats["candidates"], stats["aligned"], stats["closed"]) == (2, 1, 1)
    for entry in (0, 1):  # the entry that stopped at its assembly, the entry without a candidate
        with pytest.raises(ieskf.LinsError, match="error -1"):
            a.loop_closed_cloud(entry)
    assert len(a.loop_closed_cloud(2)) == res[2]["latest"]["n"] > 0
    assert states(a, [0]) == before and a.pose_graph_count(0) == (12, 0)  # its graph is untouched
    for s in (1, 2):
        assert lsc.frozen(res[s]) == single[s] == ref["step"][s], s
    assert states(a, [1, 2]) == single_states
    fresh(a)  # (the far pose does not outlive the test)


def test_errors_leave_the_context_usable(pkg, ieskf, pair, ref):
    a, _ = pair
    L = ieskf.lib()
    prm = lsc.params(L)
    with ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024) as c:
        with pytest.raises(ieskf.LinsError, match="error -6"):  # before lins_archive_init
            c.loop_step(entries([0]), prm)
        c.archive_init(1, 4, 1024)
        with pytest.raises(ieskf.LinsError, match="error -6"):  # before lins_pose_graph_init
            c.loop_step(entries([0]), prm)
        c.pose_graph_init(1, 4, 1)
        r = c.loop_step(entries([0]), prm)[0]  # a slot without frames: no loop
        assert lsc.frozen(r) == lsc.frozen(lsc.result_zero())
    fresh(a, 4)
    a.pose_graph_push(3, None, lsc.six_of_key(lsc.frames()[0][3]))  # slot 3: a frame in the graph, none in the archive
    before = states(a)
    ok = (0, lsc.centre(), lsc.NOW)
    bad_centre = np.array([np.nan, 0, 0], np.float32)
    for match, ent, p in (
            ("error -1", [(-1, lsc.centre(), lsc.NOW)], prm), ("error -1", [(4, lsc.centre(), lsc.NOW)], prm),
            ("error -1", [ok, (1, lsc.centre(), lsc.NOW), ok], prm),          # a slot named twice
            ("error -1", [ok, (3, lsc.centre(), lsc.NOW)], prm),             # archive and graph hold different frame counts
            ("error -1", [(0, lsc.centre(), lsc.NOW, 0)], prm),               # a stream, and no streams
            ("error -1", [defs.loop_step_entry(0, None, lsc.NOW)], prm),      # LINS_LOOP_CENTRE_STREAM without a stream
            ("error -4", [ok[:1] + (bad_centre, lsc.NOW)], prm), ("error -4", [(1, lsc.centre(), np.inf)], prm),
            ("error -4", [(2, np.array([0, np.inf, 0], np.float32), lsc.NOW)], prm),
            ("error -1", [ok], lsc.params(L, search_num=-1)), ("error -1", [ok], lsc.params(L, search_radius=-1.0)),
            ("error -1", [ok], lsc.params(L, history_leaf=-0.4)), ("error -1", [ok], lsc.params(L, icp=dict(max_iterations=0))),
            ("error -1", [ok], lsc.params(L, graph=dict(lambda_up=1.0))), ("error -1", [ok], lsc.params(L, min_gap_s=np.nan))):
        with pytest.raises(ieskf.LinsError, match=match):
            a.loop_step(ent, p)
    e = defs.loop_step_entry(0, lsc.centre(), lsc.NOW)
    e.flags = 2
    with pytest.raises(ieskf.LinsError, match="error -1"):
        a.loop_step([e], prm)
    assert states(a) == before  # nothing changed
    res = [lsc.frozen(r) for r in a.loop_step(entries([0, 1, 2]), prm)]
    assert res == ref["step"] and states(a) == ref["step_states"]


def test_closed_cloud_is_the_move_at_the_final_transform(pair, ieskf):
    a, _ = pair
    fresh(a)
    res = a.loop_step(entries([0, 1, 2]), lsc.params(ieskf.lib()))
    for entry, source in ((0, 0), (2, 2)):  # the step's assembly: two clouds per candidate, in entry order
        got = a.loop_closed_cloud(entry)
        src = a.archive_download(source)
        assert len(src) == res[entry]["latest"]["n"] == len(got) > 0
        M = res[entry]["icp"]["transform"][:3].astype(np.float32)  # step 1 of the ICP's contract: T rounded entry by entry
        x, y, z = src[:, 0], src[:, 1], src[:, 2]
        want = src.copy()
        for i in range(3):
            want[:, i] = ((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3]
        assert want.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
        assert np.abs(got[:, :3] - src[:, :3]).max() > 0.01  # the alignment moved it
    with pytest.raises(ieskf.LinsError, match="error -1"):  # the entry without a candidate was not aligned
        a.loop_closed_cloud(1)
    with pytest.raises(ieskf.LinsError, match="error -1"):
        a.loop_closed_cloud(3)
    a.archive_assemble([dict(slot=0, ids=[0], clouds=3, leaf=0.0, flags=0)])
    with pytest.raises(ieskf.LinsError, match="error -6"):  # the source is no longer the archive's last assembly
        a.loop_closed_cloud(0)
