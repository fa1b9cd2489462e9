"""lins_team_rebase / lins_pose_graph_rebase_batch (include/lins_team.h "merge") on the fixture of tests/rendezvous_cases.py:
slot 1 found itself in slot 0 (lins_rendezvous_step), and the X it got moves slot 1's whole history — graph, archive, ring
and the stream's map pose — into slot 0's frame.

Device against the CPU restatement (lins_host_pose_graph_rebase, the same X): both run csrc/pose_graph.h's text on the same
f64 measurements, and the poses of a graph without loops are products and sums alone, so the two differ only where the two
compilers' libm calls do when a frame is pushed.  Measured on an MI355X on this fixture: the largest difference of an f64
pose entry is 0 — the two hold the same bits, and so do the six floats; the bar is 4 x that, as tests/test_gpu_pose_graph.py
took for DEVICE_BAR: REBASE_BAR = 0, bit for bit.

Where the rebased frames lie.  With o_k the stored origin of slot 1's frame k, p_k its true position in slot 0's frame and
L the query frame of the rendezvous:  X o_k - p_k = (X o_L - p_L) + (R_X - R_G)(o_k - o_L) + rounding, because the truth
G takes o_k - o_L to p_k - p_L.  The first term is the origin error of the rendezvous, asserted at 2 e by
tests/test_gpu_rendezvous.py (e: the CPU restatement's, tests/test_rendezvous_inputs.py); the second is at most
|R_X R_G^T - I|_2 |o_k - o_L|, the lever arm's share of X's rotation error; the rounding is that of the stored f32 poses
(the fixture's, G^-1 composed and rounded) and of the rebased six floats, two roundings of coordinates below 16 m and one
of the rotation applied to them: 3 x 2^-24 x 16 x sqrt(3) = 5e-6 m, taken as ROUNDING = 1e-5 m."""
import numpy as np
import pytest

import map_step_chain as ch
import place_loop_cases as plc
import rendezvous_cases as rc
from map_step_chain import sm
from test_gpu_rendezvous import ALL, LATEST, N, params

pytestmark = pytest.mark.gpu
host, team, defs = rc.host, rc.team, ch.defs
F = np.float32
E_ARG, E_INPUT = -1, -4
REBASE_MEASURED = 0.0
REBASE_BAR = 4 * REBASE_MEASURED
ROUNDING = 1e-5
WINDOW = 3


def newest_six(s):
    return plc.six_of_key(rc.slots()[0][s][LATEST][3])


def context(pkg, ieskf, fill=ALL):
    """archive, ring (window 3), graph, place store and a map pose per stream: every module a rebase writes through"""
    fr = rc.slots()[0]
    c = ch.context(pkg, ieskf)
    c.streams_init(3)
    c.local_map_init(3, WINDOW, ch.MAX_PTS)
    c.archive_init(3, 16, sum(len(x) for s in fr.values() for f in s for x in f[:3]) + (1 << 17))  # (room for the key frame of the map step)
    sm.init(c, 3, ch.INTERVAL)
    c.pose_graph_init(3, 16, 2)
    assert c.place_init(up_axis=rc.UP) == 0
    for s in fill:
        for i, f in enumerate(fr[s]):
            pose = tuple(float(v) for v in f[3])
            assert c.archive_push(s, *f[:3], pose, time=float(i)) == c.pose_graph_push(s, plc.six_of_key(fr[s][i - 1][3]) if i else None, plc.six_of_key(f[3])) == i
            c.local_map_push(s, *f[:3], pose)
        six = np.asarray(newest_six(s), F)
        sm.set_pose(c, s, dict(bef=six, aft=six, tobe=six, last=six, prev=six[3:6], n_frames=N, last_time=float(LATEST)))
    return c


def record(c, s):
    p = sm.get_pose(c, s)
    return tuple(np.asarray(p[k], F).tobytes() for k in ("bef", "aft", "tobe", "last", "prev")) + (p["n_frames"], p["last_time"])


def state(c, s):
    """graph, archive (an assembly of every frame) and the stream's map pose of slot s, as bytes"""
    c.archive_assemble([dict(slot=s, ids=list(range(N)), clouds=7, leaf=0.0, flags=0)])
    return (c.pose_graph_count(s), c.pose_graph_poses(s).tobytes(), c.debug_pose_graph_poses_f64(s).tobytes(), c.archive_download(0).tobytes(), record(c, s))


def host_graph(s=1):
    fr = rc.slots()[0][s]
    g = host.PoseGraph(16, 2)
    for i, f in enumerate(fr):
        assert g.push(plc.six_of_key(fr[i - 1][3]) if i else None, plc.six_of_key(f[3])) == i
    return g


@pytest.fixture(scope="module")
def merged(pkg, ieskf):
    """context a: slot 1 rebased by the X of its own rendezvous; context b: as filled; the CPU restatement rebased by the same X"""
    a, b = context(pkg, ieskf), context(pkg, ieskf)
    before = [state(a, s) for s in ALL]
    got = team.rendezvous_step(a, [(1, rc.NOW)], ALL, params(ieskf), shortlist=rc.M, k=rc.K)[0]
    assert (got["outcome"], got["target_slot"]) == (defs.RENDEZVOUS_FOUND, 0)
    X = np.asarray(got["X"], np.float64).reshape(4, 4)
    h = host_graph()
    assert h.rebase(X) == 0
    assert team.rebase(a, [1], [X], streams=[1]) == 0
    yield dict(a=a, b=b, before=before, X=X, h=h, after=[state(a, s) for s in ALL])
    a.close(), b.close()


def test_device_poses_are_the_restatements(merged):
    a, h = merged["a"], merged["h"]
    d = float(np.abs(a.debug_pose_graph_poses_f64(1) - h.poses_f64()).max())
    six = int(np.abs(a.pose_graph_poses(1).view(np.int32).astype(np.int64) - h.poses().view(np.int32).astype(np.int64)).max())
    print("rebased f64 poses, device against the restatement: %.3g (bar %.3g); six floats: %d ulp" % (d, REBASE_BAR, six))
    assert d <= REBASE_BAR
    assert a.pose_graph_count(1) == (N, 0)


def test_archive_ring_and_stream_follow_and_the_others_keep_their_bits(merged):
    a, b, h = merged["a"], merged["b"], merged["h"]
    # the archive of slot 1: as after lins_archive_set_poses of the restatement's rebased poses, bit for bit
    b.archive_set_poses(1, 0, h.poses())
    b.archive_assemble([dict(slot=1, ids=list(range(N)), clouds=7, leaf=0.0, flags=0)])
    assert merged["after"][1][3] == b.archive_download(0).tobytes() and merged["after"][1][3] != merged["before"][1][3]
    # the ring's frames are the newest, by age: a build of it equals a build of b's ring with the same poses set
    scan = rc.slots()[0][0][LATEST][:3]
    for age in range(WINDOW):
        b.local_map_set_pose(1, age, tuple(float(v) for v in h.poses()[N - 1 - age]))
    sa, sb = a.local_map_build([1], [scan]), b.local_map_build([1], [scan])
    assert tuple(sa[0]["n"]) == tuple(sb[0]["n"]) and all(a.local_map_download(0, w).tobytes() == b.local_map_download(0, w).tobytes() for w in (0, 1))
    # the stream's map pose: aft = last = tobe = the newest rebased pose; bef, prev, n_frames, last_time untouched
    rec, rec0 = merged["after"][1][4], merged["before"][1][4]
    newest = np.asarray(plc.six_of_key(a.pose_graph_poses(1)[LATEST]), F).tobytes()
    assert rec[1] == rec[2] == rec[3] == newest and (rec[0],) + rec[4:] == (rec0[0],) + rec0[4:] and rec[1] != rec0[1]
    # slots 0 and 2: not a bit
    for s in (0, 2):
        assert merged["after"][s] == merged["before"][s], s


def test_slot_1_lies_where_it_truly_stood_in_slot_0s_frame(merged):
    a, X = merged["a"], merged["X"]
    fr, pb = rc.slots()
    e = rc.origin_error(rc.host_chain(1)["X"])
    G = rc.G()
    rot_err = float(np.linalg.norm(X[:3, :3] @ G[:3, :3].T - np.eye(3), 2))
    stored = np.array([f[3][:3] for f in fr[1]], np.float64)
    at = a.pose_graph_poses(1)[:, :3].astype(np.float64)
    err = np.linalg.norm(at - np.asarray(pb, np.float64)[:, :3], axis=1)
    bound = 2.0 * e + rot_err * np.linalg.norm(stored - stored[LATEST], axis=1) + ROUNDING
    print("e %.4f m, rotation error of X %.3g; origin errors of slot 1's frames %s\nbounds %s" % (e, rot_err, np.round(err, 4), np.round(bound, 4)))
    assert e <= plc.bound()[0] and np.all(err <= bound)
    # ... which is not where they were stored: the frames moved by about G's 7 m
    assert np.linalg.norm(at - stored, axis=1).min() > 3.0


def test_refusals_change_nothing_and_the_graph_alone_moves_alone(merged):
    a, X = merged["a"], merged["X"]
    before = [state(a, s) for s in ALL]
    bad = X.copy()
    bad[:3, :3] *= 1.00001
    nan = X.copy()
    nan[0, 3] = np.nan
    assert team.rebase(a, [2], [bad], streams=[2]) == E_INPUT and team.pose_graph_rebase(a, [2], [nan]) == E_INPUT
    assert team.rebase(a, [0, 2], [X, bad]) == E_INPUT  # (an entry behind a good one: nothing of the good one is done)
    assert team.rebase(a, [2, 2], [X, X]) == E_ARG and team.rebase(a, [3], [X]) == E_ARG and team.pose_graph_rebase(a, [-1], [X]) == E_ARG
    assert team.rebase(a, [2], [X], streams=[3]) == E_ARG and team.rebase(a, [0, 2], [X, X], streams=[1, 1]) == E_ARG
    far = np.eye(4)
    far[0, 3] = 2e6  # poses the archive does not take: asked of the rebased poses before they are stored
    assert team.rebase(a, [2], [far], streams=[2]) == E_INPUT
    assert [state(a, s) for s in ALL] == before
    assert team.rebase(a, [], []) == 0 and team.pose_graph_rebase(a, [], []) == 0
    # lins_pose_graph_rebase_batch moves the graph and nothing else; the inverse brings the f64 poses back within the bar
    assert team.pose_graph_rebase(a, [2], [X]) == 0
    now = state(a, 2)
    assert now[1] != before[2][1] and now[3:] == before[2][3:] and [state(a, s) for s in (0, 1)] == before[:2]
    assert team.rebase(a, [2], [np.linalg.inv(X)], streams=[2]) == 0
    assert np.abs(a.debug_pose_graph_poses_f64(2) - np.frombuffer(before[2][2]).reshape(-1, 12)).max() <= 1e-12


def test_a_snapshot_after_the_rebase_restores_the_rebased_state(merged, pkg, ieskf):
    a, X = merged["a"], merged["X"]
    want = state(a, 1)
    (blob,) = a.streams_snapshot([1])
    c = context(pkg, ieskf, fill=[])
    try:
        c.streams_restore([1], [blob])
        assert state(c, 1) == want and c.streams_snapshot([1]) == [blob]
        # the prior travelled as f64: a further rebase of both gives the same bits
        step = np.linalg.inv(X)
        assert team.rebase(a, [1], [step], streams=[1]) == 0 and team.rebase(c, [1], [step], streams=[1]) == 0
        assert state(c, 1) == state(a, 1)
        assert team.rebase(a, [1], [X], streams=[1]) == 0  # (slot 1 back in slot 0's frame for the tests behind this one)
    finally:
        c.close()


def test_the_rebased_stream_takes_a_further_map_step(merged):
    a = merged["a"]
    ch.feed(a, 0)
    st = sm.get_pose(a, 1)
    res = sm.step(a, [1], [sm.odom(st["bef"], float(LATEST) + 1.0)])[0]  # transformSum = transformBefMapped: the scan starts at the rebased pose
    print("map step on the rebased stream:", {k: res[k] for k in ("status", "iters", "converged", "n_sel", "key_frame")})
    assert res["status"] == 0
    assert np.abs(np.asarray(res["tobe_start"], F) - np.asarray(st["aft"], F)).max() < 1e-4
