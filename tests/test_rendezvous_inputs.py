"""The fairness of the rendezvous fixture (tests/rendezvous_cases.py), on the CPU restatement alone: what
tests/test_gpu_rendezvous.py expects of the device must be there to be found.  These are conditions on the FIXTURE; if
one fails the fixture changes, not the bar.
  - slot 1's stored poses are G^-1 composed with its true ones, so the truth of a rendezvous in slot 0 is G;
  - with the shortlist the GPU test uses (M = 8) the true counterpart — slot 0's frame 11, where slot 1's latest frame
    stood — is in the shortlist, and is the first rank;
  - the chosen ICP converges under max_fitness (0.3);
  - the restatement's X puts the query frame's origin within e of where it truly stood.  e is not taken from this case:
    it is the error the identity-start archive case of tests/loop_icp_cases.py leaves after its chain
    (place_loop_cases.bound()[0], 0.105 m) — the same room, the same scan noise, the same ICP.  Measured here: 0.036 m."""
import numpy as np

import place_loop_cases as plc
import rendezvous_cases as rc


def test_slot_1_lives_in_a_frame_displaced_by_G():
    fr, pb = rc.slots()
    G = rc.G()
    assert abs(np.linalg.norm(G[:3, 3]) - 7.0) < 0.01 and abs(np.degrees(np.arctan2(G[1, 0], G[0, 0])) - 26.0) < 1e-9
    for i in range(rc.N):
        # f32 poses: 1e-7 relative, on coordinates of up to 15 m
        assert np.abs(rc.matrix(fr[1][i][3]) - np.linalg.inv(G) @ rc.matrix(pb[i])).max() < 2e-6
        assert np.abs(rc.truth(i) - G).max() < 2e-6
    assert rc.origin_error(G) < 2e-6 and rc.origin_error(np.eye(4)) > 5.0


def test_the_counterpart_is_shortlisted_and_its_icp_converges():
    r = rc.host_chain(1)
    ranks = [(x["slot"], x["id"]) for x in r["ranks"]]
    print("ranks:", [(x["slot"], x["id"], x["shift"], float(x["distance"]), x["dk"]) for x in r["ranks"]],
          "fitness:", [i["fitness"] for i in r["icp"]])
    assert (0, rc.N - 1) in r["shortlist"] and ranks[0] == (0, rc.N - 1)
    assert r["chosen"] == 0
    icp = r["icp"][0]
    assert icp["converged"] == 1 and icp["fitness"] <= 0.3
    # the guess alone is a sector's worth off; the ICP brings it in
    e = rc.origin_error(r["X"])
    print("origin error of the guess %.3f m, of X %.4f m; bound %.4f m" % (rc.origin_error(r["T0"][0]), e, plc.bound()[0]))
    assert e <= plc.bound()[0]
    assert rc.origin_error(r["T0"][0]) > e


def test_the_other_entries_have_an_outcome_of_their_own():
    """slot 2 maps another building: its ranks are aligned and none is accepted; slot 0 finds slot 1's latest frame first"""
    r2, r0 = rc.host_chain(2), rc.host_chain(0)
    assert r2["ranks"] and r2["chosen"] == -1
    assert (r0["ranks"][0]["slot"], r0["ranks"][0]["id"]) == (1, rc.N - 1) and r0["icp"][0]["converged"] == 1 and r0["icp"][0]["fitness"] <= 0.3
