"""What tests/test_gpu_place_loop.py rests on, asserted on the CPU with the host restatement: the fixture of
tests/place_loop_cases.py is fair — the pose-based detector finds nothing, the revisited frame wins the appearance search
by a clear margin over the frame a half turn of the room away, the guess starts an ICP that converges — and the bound
the device is held to."""
import numpy as np

import place_loop_cases as plc

host = plc.host


def test_the_fixture_is_fair():
    frames, true, wrong = plc.case()
    poses = np.array([f[3] for f in frames])
    assert np.linalg.norm(wrong[:3] - true[:3]) > plc.RADIUS and abs(wrong[5] - true[5]) > 4 * plc.DS
    assert host.find_loop(poses, np.arange(plc.N, dtype=np.float64), wrong[:3], plc.RADIUS, plc.NOW, plc.GAP) == -1
    r = plc.host_chain()
    row = np.array(r["row"])
    twin = (plc.REVISITED + plc.N // 2) % plc.N  # where the room's half turn takes the revisited frame
    others = np.delete(row, [plc.REVISITED, twin])
    print("d: revisited %.3f, half-turn twin %.3f, every other frame >= %.3f" % (row[plc.REVISITED], row[twin], others.min()))
    assert r["search"]["id"] == plc.REVISITED and r["search"]["candidates"] == 8
    assert row[twin] - row[plc.REVISITED] > 0.08 and others.min() - row[plc.REVISITED] > 0.25  # measured: 0.097 and 0.314
    # the shift is the relative yaw of the two sensor frames (query minus candidate), to within one sector
    want = (float(true[5]) - float(frames[plc.REVISITED][3][5])) / plc.DS
    assert abs(r["search"]["shift"] - want) <= 1.0


def test_the_chain_closes_the_loop_on_the_cpu():
    frames, true, wrong = plc.case()
    r = plc.host_chain()
    assert r["icp"]["converged"] == 1 and r["icp"]["fitness"] <= 0.3  # LM:1140
    err = float(np.linalg.norm(r["final"][:3].astype(np.float64) - true[:3]))
    left, bound = plc.bound()
    print("last frame: %.3f m from its true position after the solve; the identity-start archive case leaves %.3f m; bound %.3f m" % (err, left, bound))
    assert err <= bound
    assert 0.05 < left < 0.2  # (the bound is not vacuous: measured 0.105 m, the case's own error 0.059 m)
