"""The two pose kernels of csrc/map_pose_kernels.hip.

map_associate_kernel through lins_map_associate_batch: the host test's cases (map_pose_cases.CASES) padded to n = 65 —
a second wave with a single lane — and each at n = 1, against the f64 composition of tests/map_pose_np.py under the
bar 4 x E_host (device and host evaluate the same f32 text and differ only by ocml's and glibc's last-place
trigonometry); a case's bits do not depend on its position in the batch or on the batch's size.

map_pose_finish_kernel through lins_streams_map_step on states written with lins_streams_map_set_pose: the key-frame
rule at the 0.3 m threshold and one ulp either side of it, with and without key frames, and transformUpdate's tail with
and without IMU — bit for bit against lins_host_map_key_rule / lins_host_map_transform_update (no trigonometry in
either: the float sqrt and the f64 blend are correctly rounded on both sides)."""
import numpy as np
import pytest

import map_pose_cases as mc
import map_step_chain as ch
from map_step_chain import defs, sm

pytestmark = pytest.mark.gpu
F = np.float32
WAVE_PLUS_ONE = 65


def batches():
    """CASES in batches of 65 rows (the last one padded with its own first case)"""
    rows = [(b, a, s) for _, b, a, s in mc.CASES]
    out = []
    for i in range(0, len(rows), WAVE_PLUS_ONE):
        part = rows[i:i + WAVE_PLUS_ONE]
        out.append((len(part), part + [part[0]] * (WAVE_PLUS_ONE - len(part))))
    return out


@pytest.fixture(scope="module")
def device_results(pkg, ieskf):
    """tobe of every case from batches of 65"""
    got = []
    with ch.context(pkg, ieskf, 1) as c:
        for n, part in batches():
            out = sm.map_associate_batch(c, [p[0] for p in part], [p[1] for p in part], [p[2] for p in part])
            assert out.shape == (WAVE_PLUS_ONE, 6)
            got += list(out[:n])
    return got


def test_associate_batch_against_the_f64_composition(device_results):
    e_rot = e_trans = 0.0
    for (name, b, a, s), got in zip(mc.CASES, device_results):
        r, t = mc.diff_to_composition(got, b, a, s)
        e_rot, e_trans = max(e_rot, r), max(e_trans, t)
    print("device over %d cases: rotation %.3e, translation %.3e m (E_host %.3e, %.3e)" % (len(mc.CASES), e_rot, e_trans, mc.E_HOST_ROT, mc.E_HOST_TRANS))
    assert e_rot <= 4 * mc.E_HOST_ROT and e_trans <= 4 * mc.E_HOST_TRANS


def test_associate_bits_do_not_depend_on_position_or_batch_size(pkg, ieskf, device_results):
    pick = [0, 7, 30, 64, 100, 200, len(mc.CASES) - 1]
    with ch.context(pkg, ieskf, 1) as c:
        for i in pick:  # n = 1
            _, b, a, s = mc.CASES[i]
            assert mc.same_bits(sm.map_associate_batch(c, [b], [a], [s])[0], device_results[i]), i
        # the same case at index 0 and at index 64 of one batch (the single lane of the second wave)
        rows = [mc.CASES[(40 + k) % len(mc.CASES)][1:] for k in range(WAVE_PLUS_ONE)]
        rows[64] = rows[0]
        out = sm.map_associate_batch(c, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
        assert mc.same_bits(out[0], out[64]) and mc.same_bits(out[0], device_results[40])
        assert sm.map_associate_batch(c, np.zeros((0, 6)), np.zeros((0, 6)), np.zeros((0, 6))).shape == (0, 6)
        bad = np.zeros((2, 6), F)
        bad[1, 4] = np.inf
        with pytest.raises(RuntimeError, match="-4"):
            sm.map_associate_batch(c, bad, np.zeros((2, 6)), np.zeros((2, 6)))


def test_finish_key_rule_at_the_threshold(pkg, ieskf):
    """empty rings: LM:1636 does not hold, transformUpdate does not run, the rule sees the aft that set_pose wrote"""
    cases = [(p, a, have) for p, a in mc.key_rule_threshold_cases() for have in (0, 1)]
    total = np.array([0.01, -0.02, 0.03, 1.0, 2.0, 3.0], F)
    with ch.context(pkg, ieskf) as c:
        ch.setup(c, archive=False)
        ch.feed(c, 0)
        for i in range(0, len(cases), ch.N):
            c.local_map_init(ch.N, ch.WINDOW, ch.MAX_PTS)  # (empty rings again)
            sm.init(c, ch.N)
            part = cases[i:i + ch.N]
            for s, (prev, aft, have) in enumerate(part):
                sm.set_pose(c, s, dict(aft=aft, bef=np.full(6, 0.5, F), prev=prev, n_frames=have))
            streams = list(range(len(part)))
            res = sm.step(c, streams, [sm.odom(total, 1.0, 0.3, 0.4, True) for _ in streams])
            for s, (prev, aft, have) in enumerate(part):
                save, want_prev = sm.host_key_rule(prev, aft, have)
                st = sm.get_pose(c, s)
                assert res[s]["status"] == 0 and res[s]["iters"] == 0 and res[s]["key_frame"] == save, (i, s)
                assert mc.same_bits(st["prev"], want_prev) and mc.same_bits(st["aft"], aft) and mc.same_bits(res[s]["transform"], aft)
                assert mc.same_bits(st["bef"], np.full(6, 0.5, F))  # (no transformUpdate)
                assert st["n_frames"] == have + save and st["last_time"] == (1.0)
                start = res[s]["tobe_start"]
                assert mc.same_bits(start, sm.map_associate_batch(c, [np.full(6, 0.5, F)], [aft], [total])[0])
                if save:  # the first key frame takes tobe, a later one aft — and then tobe = last = aft
                    key = start if have == 0 else aft
                    assert mc.same_bits(res[s]["key_pose"], key) and mc.same_bits(st["last"], key) and mc.same_bits(st["tobe"], key)
                    assert res[s]["ring_age"] == 0 and res[s]["archive_id"] == -1
                else:
                    assert mc.same_bits(st["tobe"], start) and res[s]["ring_age"] == -1


def test_finish_transform_update_with_and_without_imu(pkg, ieskf):
    with ch.context(pkg, ieskf) as c:
        ch.setup(c, archive=False)
        sm.init(c, ch.N)
        ch.feed(c, 0)
        first = sm.step(c, [0, 1, 2], ch.odoms(0))
        assert all(r["key_frame"] == 1 and r["iters"] == 0 for r in first)  # the rings were empty
        ch.feed(c, 1)
        before = [sm.get_pose(c, s) for s in range(ch.N)]
        imu = [(True, F(0.11), F(-0.07)), (False, F(0.5), F(0.5)), (True, F(-0.3), F(0.02))]
        odo = [(ch.odometry(1)[s][0], 0.4, imu[s][1], imu[s][2], imu[s][0]) for s in range(ch.N)]
        res = sm.step(c, [0, 1, 2], [sm.odom(o[0], o[1], o[2], o[3], o[4]) for o in odo])
        # the rounds' own result: the same context, the same build, the same start
        rounds = c.scan2map_batch([defs.MapProblem.local(r["tobe_start"]) for r in res])
        for s in range(ch.N):
            assert res[s]["status"] == 0 and res[s]["iters"] > 0, s  # one key frame per ring: LM:1636 holds
            assert (res[s]["iters"], res[s]["converged"], res[s]["degenerate"], res[s]["n_sel"]) == tuple(rounds[s][f] for f in ("iters", "converged", "degenerate", "n_sel"))
            tobe, bef, aft = sm.host_transform_update(rounds[s]["transform"], imu[s][0], imu[s][1], imu[s][2], odo[s][0], before[s]["bef"], before[s]["aft"])
            save, prev = sm.host_key_rule(before[s]["prev"], aft, 1)
            st = sm.get_pose(c, s)
            assert mc.same_bits(st["bef"], odo[s][0]) and mc.same_bits(st["aft"], aft) and mc.same_bits(res[s]["transform"], aft), s
            assert mc.same_bits(st["tobe"], aft if save else tobe) and mc.same_bits(st["prev"], prev) and res[s]["key_frame"] == save
            if not imu[s][0]:
                assert mc.same_bits(aft, rounds[s]["transform"])
