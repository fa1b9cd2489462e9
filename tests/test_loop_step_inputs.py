"""What the GPU tests of tests/test_gpu_loop_step.py rest on, asserted with the CPU restatements (host.find_loop,
host.submap, host.loop_icp, host.PoseGraph) on the set-up of tests/loop_step_cases.py: the archive case has a loop
candidate that is a real loop, its alignment is accepted, and after the solve the same centre finds the same candidate —
so the second step of the repeat test really takes the repeat branch."""
import numpy as np

import loop_step_cases as lsc

host, defs = lsc.host, lsc.defs


def key_poses(fr):
    return np.array([f[3] for f in fr], np.float32)


def test_the_archive_case_closes_a_loop_and_then_repeats():
    fr = lsc.frames()
    latest = len(fr) - 1
    poses, centre = key_poses(fr), lsc.centre()
    closest = host.find_loop(poses, lsc.times("loop"), centre, lsc.RADIUS, lsc.NOW, lsc.GAP)
    # a candidate exists, is not the latest frame and lies beyond the gap: frames 0 .. 5
    assert 0 <= closest <= 5 and closest != latest
    assert host.loop_candidate(latest, closest) == -1
    # with every time inside the gap there is none
    assert host.find_loop(poses, lsc.times("inside"), centre, lsc.RADIUS, lsc.NOW, lsc.GAP) == -1
    assert all(abs(t - lsc.NOW) <= lsc.GAP for t in lsc.times("inside"))
    # the two submaps and the alignment: converged, fitness within the reference's 0.3, a usable variance
    ids = host.loop_window(latest, closest, lsc.H)
    assert ids == list(range(max(0, closest - lsc.H), min(latest, closest + lsc.H) + 1))
    src = host.submap(fr, [latest], 3, 0.0, 1)[0]
    tgt = host.submap(fr, ids, 3, 0.4, 0)[0]
    icp = host.loop_icp(src, tgt)
    print("closest %d, window %s, source %d target %d points, fitness %.4g after %d rounds" % (
        closest, ids, len(src), len(tgt), icp["fitness"], icp["iterations"]))
    assert icp["converged"] == 1 and icp["fitness"] <= 0.3
    assert host.loop_accept(icp["converged"], icp["fitness"]) and host.loop_variance(icp["fitness"])[0]
    # rejection test: no positive fitness passes max_fitness = 0
    assert icp["fitness"] > 0.0 and not host.loop_accept(icp["converged"], icp["fitness"], 0.0)
    # the graph, solved; the corrected poses then go to the archive's frame list
    g = host.PoseGraph(lsc.MAX_FRAMES, lsc.MAX_LOOPS)
    for i, f in enumerate(fr):
        g.push(lsc.six_of_key(fr[i - 1][3]) if i else None, lsc.six_of_key(f[3]))
    wrong = g.poses(latest, 1)[0]
    assert np.array_equal(wrong, fr[latest][3])
    g.add_loop(latest, closest, host.loop_pose_from(icp["transform"], wrong), icp["fitness"])
    r = g.solve()
    assert r["iterations"] > 0 and r["cost_after"] < r["cost_before"]
    solved = g.poses()
    assert np.abs(solved - poses).max() > 0.0
    # the same centre and time on the corrected history: the same candidate again -> (latest, closest) is the pair of the
    # slot's most recent loop factor, the repeat branch
    again = host.find_loop(solved, lsc.times("loop"), centre, lsc.RADIUS, lsc.NOW, lsc.GAP)
    assert again == closest
    assert host.loop_candidate(latest, again, latest, closest) == defs.LOOP_REPEAT
