"""Place recognition on the CPU (include/lins_host.h lins_host_place_*, the definition the device is held to) against
the independent numpy statement tests/place_np.py, and its edge cases as the contract states them."""
import numpy as np
import pytest

import place_cases as pc
import place_np as pnp

F = np.float32
ALL = np.concatenate


def desc(host, fr, up=1, **kw):
    return host.place_descriptor(*fr, params=host.place_params(up_axis=up, **kw))


@pytest.mark.parametrize("up", [0, 1, 2])
def test_descriptors_equal_the_numpy_statement_exactly(host, up):
    for q, cands, _, _, _ in pc.winner_cases(up):
        for fr in [q] + cands[:3]:
            got, want = desc(host, fr, up), pnp.descriptor(ALL(fr), up=up)
            assert got.dtype == F and np.array_equal(got, want)
            assert (got > 0).sum() > 100
    # a mask of one cloud describes that cloud alone
    q = pc.winner_cases(up)[0][0]
    assert np.array_equal(desc(host, q, up, clouds=2), pnp.descriptor(q[1], up=up))
    assert not np.array_equal(desc(host, q, up, clouds=2), desc(host, q, up))


def test_distances_and_winners_against_f64(host):
    """distances within 1e-5 (80 f32 roundings of values <= 1, with margin); the winner equal wherever the f64 runner-up
    is more than 1e-4 behind — and the cases are built so that every one is"""
    skipped = 0
    for q, cands, times, true_id, true_shift in pc.winner_cases(1):
        Dq, Dc = desc(host, q), [desc(host, c) for c in cands]
        for c in (0, true_id, 12):
            got, want = host.place_distance(Dq, Dc[c]), pnp.distances(Dq, Dc[c])
            print("max |d - d64|", np.abs(got - want).max())
            assert got.dtype == F and np.abs(got - want).max() <= 1e-5
        wid, wk, wd, wn, runner = pnp.search(Dq, Dc, times, 100.0, 1.0)
        print("winner", wid, wk, wd, "runner-up", runner)
        if runner - wd <= 1e-4:
            skipped += 1
            continue
        got = host.place_search(Dq, Dc, times, 100.0, 1.0)
        assert (got["id"], got["shift"], got["candidates"]) == (wid, wk, wn) == (true_id, true_shift, 13)
        assert abs(float(got["distance"]) - wd) <= 1e-5
    assert skipped == 0


def test_sign_convention_and_guess(host):
    """a frame and its copy turned by +7 sectors: shift 7 one way, 53 the other; the guess maps one cloud onto the other
    to within half a sector at 10 m"""
    for up in (1, 2):
        a, b = pc.place(42, up=up), pc.place(42, up=up, turn=7)
        Da, Db = desc(host, pc.frame(a), up), desc(host, pc.frame(b), up)
        assert int(np.argmin(host.place_distance(Da, Db))) == 7 and int(np.argmin(host.place_distance(Db, Da))) == 53
        # both frames stored at the same pose: T0 maps the query's assembled cloud onto the candidate's
        pose = (1.0, -2.0, 0.5, 0.02, -0.01, 0.3)
        from map_synth import rot
        R, t = rot(*pose[3:]), np.array(pose[:3])
        T0 = host.place_guess(pose, pose, 7, up)
        wa, wb = a[:, :3].astype(np.float64) @ R.T + t, b[:, :3].astype(np.float64) @ R.T + t
        moved = wa @ T0[:3, :3].T + T0[:3, 3]
        err = np.linalg.norm(moved - wb, axis=1)
        rho = np.linalg.norm(np.delete(a[:, :3], up, 1), axis=1)
        print("up", up, "max error at <= 10 m", err[rho <= 10].max())
        assert err[rho <= 10].max() <= 10 * pc.DS / 2
        assert np.abs(host.place_guess(pose, pose, 0, up) - np.eye(4)).max() <= 1e-12
    assert host.place_guess(pose, pose, 60, 1) == -1 and host.place_guess(pose, pose, 0, 3) == -1


def test_the_guess_uses_the_pose_conversion_behind_loop_pose_from(host):
    """lins_host_loop_pose_from (LM:1156-1166) answers "which pose has matrix T M(wrong)" in the reference's shuffled
    order (z, x, y, yaw, roll, pitch).  Its camera / lidar shuffle of T is exact where T turns about one axis, so there
    the pose it returns, put back into key-pose order, must give place_guess(wrong, pose, 0) = M(pose) M(wrong)^-1 = T
    to f32 rounding: the guess's M is the matrix pose_from means."""
    wrong = (1.0, -2.0, 0.5, 0.2, -0.3, 0.7)
    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        T = np.eye(4)
        T[a, a] = T[b, b] = np.cos(0.4)
        T[b, a], T[a, b] = np.sin(0.4), -np.sin(0.4)
        T[:3, 3] = (0.5, -1.5, 2.0)
        pf = host.loop_pose_from(T, wrong)
        pose = (pf[1], pf[2], pf[0], pf[4], pf[5], pf[3])
        got = host.place_guess(wrong, pose, 0, 1)
        print("axis", axis, "max |guess - T|", np.abs(got - T).max())
        assert np.abs(got - T).max() <= 2e-6


def test_edge_cases(host):
    ed = pc.edge_frames(1)
    D = {k: desc(host, v) for k, v in ed.items()}
    assert not D["empty"].any()
    assert np.array_equal(host.place_distance(D["empty"], D["single"]), np.ones(60, F))
    assert np.array_equal(host.place_distance(D["empty"], D["empty"]), np.ones(60, F))
    assert (D["single"] > 0).sum() == 1 and D["single"][2, int((0.4 + np.pi) / pc.DS)] == F(3.0)
    assert np.array_equal(host.place_distance(D["single"], D["single"])[:1], np.zeros(1, F))
    assert (D["rho0"] > 0).sum() == 1 and D["rho0"][0, 30] == F(1.0)  # atan2(0, 0) = 0: (0 + pi_f) * inv_s rounds to 30
    assert (D["at_rmax"] > 0).sum() == 1 and D["at_rmax"][3].max() == F(1.5)                # the point at r_max is dropped
    assert (D["ring_edge_az0"] > 0).sum() == 1 and D["ring_edge_az0"][1].max() == F(1.0)  # 4.0 m: ring 1
    assert D["ring_edge_az0"][1, 30] == F(1.0)  # azimuth exactly 0: sector 30
    assert D["az_pi"][2, 59] == F(1.0) and D["az_pi"][4, 0] == F(1.0) and D["az_pi"][6, 30] == F(1.0)  # +pi, -pi, -0
    assert (D["az_pi"] > 0).sum() == 3
    assert (D["floor"] > 0).sum() == 2 and D["floor"][1].max() == 0 and D["floor"][3].max() == F(2.0 ** -10)  # below: dropped
    above = np.nextafter(F(2.0 ** -10) - F(pc.LIFT), F(np.inf)) + F(pc.LIFT)  # one step of the coordinate above the floor
    assert D["floor"][5].max() == above > F(2.0 ** -10)
    assert ((D["one_column"] > 0).sum(0) > 0).sum() == 1
    d = host.place_distance(D["one_column"], D["one_column"])
    assert d[0] <= 1e-6 and np.array_equal(d[1:], np.ones(59, F))  # one valid pair at shift 0, none elsewhere
    # exact half-turn symmetry: two shifts tie, the smaller wins
    q, c, k = pc.half_turn_scene(1)
    d = host.place_distance(desc(host, q), desc(host, c))
    assert d[k] == d[k + 30] == d.min()
    assert host.place_search(desc(host, q), [desc(host, c)], [0.0], 10.0, 1.0)["shift"] == k
    # two identical frames: the smaller id wins
    Dq = D["single"]
    got = host.place_search(Dq, [D["one_column"], Dq, Dq], [0.0, 0.0, 0.0], 10.0, 1.0)
    assert (got["id"], got["shift"], float(got["distance"])) == (1, 0, 0.0)
    assert host.place_search(Dq, [Dq, Dq, Dq], [0.0] * 3, 10.0, 1.0, skip_id=0)["id"] == 1
    # the time gate: at equality the candidate is not admissible; a negative gap admits every time
    assert host.place_search(Dq, [Dq, Dq], [9.0, 8.5], 10.0, 1.0) == dict(id=1, shift=0, distance=F(0), candidates=1)
    assert host.place_search(Dq, [Dq, Dq], [9.0, 10.0], 10.0, -1.0)["candidates"] == 2
    assert host.place_search(Dq, [Dq, Dq], [9.5, 10.0], 10.0, 1.0) == dict(id=-1, shift=0, distance=F(1), candidates=0)
    assert host.place_search(Dq, [], [], 10.0, 1.0)["id"] == -1
    assert host.place_search(Dq, [Dq], [0.0], np.inf, 1.0) == -4 and host.place_search(Dq, [Dq], [0.0], 1.0, np.nan) == -4


def test_loop_icp_from_identity_is_loop_icp(host):
    import loop_icp_cases as lc

    for s, t in lc.all_whole_loop_clouds():
        a, b = host.loop_icp(s, t), host.loop_icp_from(s, t, np.eye(4))
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    s, t = lc.all_whole_loop_clouds()[0]
    bad = np.eye(4)
    bad[1, 3] = np.nan
    assert host.loop_icp_from(s, t, bad) == -4
