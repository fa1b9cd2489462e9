"""What tests/test_gpu_loop_step_place.py rests on, asserted on the CPU with the host restatement: the fixture of
tests/place_verify_cases.py is fair.  The pose search finds nothing; by appearance the half-turn twin leads the revisited
frame; the twin's ICP converges under the reference's fitness bar and would close the loop more than 10 m wrong; the
revisited frame's ICP fits better, lins_host_loop_choose picks it, and the solve then leaves the last frame within the
project's bound of its true position.

Measured on the CPU restatement: d 0.105 (frame 7) / 0.107 (frame 1) / 0.406 (frame 2) / 0.409 (frame 6); fitness 0.165
(from frame 7's guess) / 0.055 (from frame 1's).  The assertions are on orders and on the named bounds, not these digits."""
import numpy as np

import place_loop_cases as plc
import place_verify_cases as pvc

host = pvc.host


def test_the_descriptor_shortlists_and_the_winner_is_the_twin():
    frames, true, wrong = pvc.case()
    poses = np.array([f[3] for f in frames])
    assert host.find_loop(poses, np.arange(pvc.N, dtype=np.float64), wrong[:3], pvc.RADIUS, pvc.NOW, pvc.GAP) == -1
    r = pvc.host_chain()
    row = r["row"]
    print("d by frame:", " ".join("%d: %.3f" % (i, d) for i, d in enumerate(row)))
    ids = [c["id"] for c in r["ranks"]]
    print("ranks with k = %d, min_sep = %d:" % (pvc.K, pvc.MIN_SEP), [(c["id"], c["shift"], float(c["distance"])) for c in r["ranks"]])
    assert r["candidates"] == 8  # frames 0 .. 7 lie beyond the gap
    assert ids == [pvc.TWIN, pvc.REVISITED]  # the neighbours 6 and 2 are suppressed, and nothing else is 4 ids away from both
    assert row[pvc.TWIN] < row[pvc.REVISITED]  # rank 0 is the twin
    # without the separation the shortlist fills with the neighbours
    top, _ = host.place_topk(*_search_args(), 4, 0, skip_id=pvc.N - 1)
    assert sorted(c["id"] for c in top) == [1, 2, 6, 7]
    # rank 0 is what the top-1 search returns
    s = host.place_search(*_search_args(), skip_id=pvc.N - 1)
    assert (s["id"], s["shift"], s["distance"].tobytes()) == (r["ranks"][0]["id"], r["ranks"][0]["shift"], r["ranks"][0]["distance"].tobytes())


def _search_args():
    frames, _, _ = pvc.case()
    prm = host.place_params(up_axis=pvc.UP)
    D = [host.place_descriptor(*f[:3], params=prm) for f in frames]
    return D[-1], D, np.arange(pvc.N, dtype=np.float64), pvc.NOW, pvc.GAP


def test_the_geometry_decides():
    frames, true, wrong = pvc.case()
    r = pvc.host_chain()
    twin, right = r["icp"]
    print("fitness: from the twin's guess %.3f (converged %d), from the revisited frame's %.3f (converged %d)" % (
        twin["fitness"], twin["converged"], right["fitness"], right["converged"]))
    # the wrong loop WOULD be accepted: LM:1140's rule passes it
    assert twin["converged"] == 1 and twin["fitness"] <= pvc.MAX_FITNESS and host.loop_accept(twin["converged"], twin["fitness"], pvc.MAX_FITNESS)
    off = float(np.linalg.norm(r["final_top1"][pvc.N - 1][:3].astype(np.float64) - true[:3]))
    print("a top-1 pipeline leaves the last frame at (%.2f, %.2f), %.2f m from the truth (%.2f, %.2f)" % (
        r["final_top1"][pvc.N - 1][0], r["final_top1"][pvc.N - 1][1], off, true[0], true[1]))
    assert off > 10.0
    # the right frame fits better, and the choice is its rank
    assert right["converged"] == 1 and right["fitness"] < twin["fitness"]
    assert r["chosen"] == 1
    err = float(np.linalg.norm(r["final"][pvc.N - 1][:3].astype(np.float64) - true[:3]))
    left, bound = plc.bound()
    print("after the solve with the chosen loop: %.3f m from the truth; bound %.3f m" % (err, bound))
    assert err <= bound
