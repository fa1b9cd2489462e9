"""Place recognition closes a loop the pose-based detector cannot see, on the device end to end (the chain of
INTEGRATION.md "Place recognition"): lins_place_search_batch -> lins_host_place_guess -> lins_archive_assemble ->
lins_loop_icp_batch_from -> lins_host_loop_pose_from -> lins_pose_graph_add_loop -> lins_pose_graph_solve ->
lins_pose_graph_apply.  The case and its fairness: tests/place_loop_cases.py, tests/test_place_loop_inputs.py.

Measured on the CPU restatement: the last frame ends 0.059 m from its true position; the identity-start archive case of
loop_icp_cases leaves 0.105 m under the same chain, so the bound is 0.210 m."""
import numpy as np
import pytest

import place_loop_cases as plc

pytestmark = pytest.mark.gpu
host = plc.host


def test_a_loop_odometry_cannot_find_is_closed_from_the_scans(pkg, ieskf):
    frames, true, wrong = plc.case()
    latest = plc.N - 1
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    c.archive_init(1, 16, sum(len(f[0]) + len(f[1]) + len(f[2]) for f in frames))
    c.pose_graph_init(1, 16, 2)
    assert c.place_init(up_axis=plc.UP) == 0
    for i, f in enumerate(frames):
        assert c.archive_push(0, *f, time=float(i)) == c.pose_graph_push(0, plc.six_of_key(frames[i - 1][3]) if i else None, plc.six_of_key(f[3])) == i
    # where the robot believes it is there is no old frame within the search radius
    assert c.archive_find_loop(0, wrong[:3], plc.RADIUS, plc.NOW, plc.GAP) == -1
    found = c.place_search([(0, latest, 0, plc.NOW, plc.GAP)])[0]
    want = plc.host_chain()
    assert (found["id"], found["shift"], found["candidates"]) == (want["search"]["id"], want["search"]["shift"], 8)
    assert found["distance"].tobytes() == want["search"]["distance"].tobytes()
    # the revisited frame, or a trajectory neighbour whose true position is nearer than the frame spacing
    spacing = min(np.linalg.norm(frames[i + 1][3][:3] - frames[i][3][:3]) for i in range(plc.N - 2))
    assert found["id"] == plc.REVISITED or np.linalg.norm(frames[found["id"]][3][:3] - true[:3]) < spacing
    yaw = (float(true[5]) - float(frames[found["id"]][3][5])) / plc.DS
    assert abs(found["shift"] - yaw) <= 1.0
    T0 = host.place_guess(wrong, frames[found["id"]][3], found["shift"], plc.UP)
    c.archive_assemble([dict(slot=0, ids=[latest], clouds=3, leaf=0.0, flags=1),
                        dict(slot=0, ids=plc.window(found["id"], latest), clouds=3, leaf=0.4, flags=0)])
    icp = c.loop_icp_from([(0, 1)], [T0])[0]
    assert icp["converged"] == 1 and icp["fitness"] <= 0.3  # LM:1140
    pose_from = host.loop_pose_from(icp["transform"], c.pose_graph_poses(0, latest, 1)[0])
    c.pose_graph_add_loop(0, latest, found["id"], pose_from, plc.LOOP_VARIANCE)
    r = c.pose_graph_solve([0])[0]
    assert r["iterations"] > 0 and r["cost_after"] < 0.5 * r["cost_before"]
    c.pose_graph_apply(0)
    final = c.pose_graph_poses(0, latest, 1)[0]
    err = float(np.linalg.norm(final[:3].astype(np.float64) - true[:3]))
    left, bound = plc.bound()
    print("last frame: %.3f m from its true position (CPU restatement %.3f m); bound %.3f m = 2 x %.3f m" % (
        err, np.linalg.norm(want["final"][:3].astype(np.float64) - true[:3]), bound, left))
    assert err <= bound
    # the archive holds the corrected pose: the pose-based detector now sees the loop
    assert c.archive_find_loop(0, final[:3], plc.RADIUS, plc.NOW, plc.GAP) == plc.REVISITED
    c.close()
