"""lins_streams_map_step — the mapping node's run() for streams in one call — against the explicit chain a caller had to
write before it (tests/map_step_chain.py: lins_map_associate_batch, lins_local_map_build_streams, lins_scan2map_batch
with LINS_MAP_LOCAL, host transform_update + key_rule, the two push calls) on a second context fed the same scans: every
result field, the six clouds of every build and every stream's pose state, bit for bit, over 8 scans of three streams with
a ring of 3 frames, a stream that does not make every scan a key frame, and one the interval gate stops once; the ring is
made to wrap for certain in the set_pose test (previousRobotPosPoint moved away before every step)."""
import numpy as np
import pytest

import map_step_chain as ch
from map_step_chain import defs, sm

pytestmark = pytest.mark.gpu
F = np.float32
STREAMS = [0, 1, 2]


def clouds_of(c, entries, step_call):
    get = (lambda k, w: sm.download(c, k, w)) if step_call else c.local_map_download
    return [[get(k, w) for w in range(6)] for k in range(entries)]


def run_step_sequence(pkg, ieskf, steps=ch.STEPS, hook=None):
    """context A: per step the results, the clouds of the step's build and the pose states"""
    out = []
    with ch.context(pkg, ieskf) as a:
        ch.setup(a)
        sm.init(a, ch.N, ch.INTERVAL)
        for step in range(steps):
            ch.feed(a, step)
            if hook:
                hook(a, step)
            res = sm.step(a, STREAMS, ch.odoms(step))
            ran = sum(r["status"] != defs.MAP_STEP_SKIPPED for r in res)
            out.append(dict(res=res, clouds=clouds_of(a, ran, True), poses=[sm.get_pose(a, s) for s in STREAMS], ms=sm.last_ms(a)))
    return out


def run_chain_sequence(pkg, ieskf, steps=ch.STEPS, hook=None):
    out = []
    with ch.context(pkg, ieskf) as b:
        ch.setup(b)
        states = [ch.fresh_state() for _ in STREAMS]
        for step in range(steps):
            ch.feed(b, step)
            if hook:
                hook(states, step)
            res = ch.explicit_step(b, states, STREAMS, ch.odometry(step))
            ran = sum(r["status"] != defs.MAP_STEP_SKIPPED for r in res)
            out.append(dict(res=res, clouds=clouds_of(b, ran, False), poses=[dict(s) for s in states]))
    return out


@pytest.fixture(scope="module")
def seq_a(pkg, ieskf):
    return run_step_sequence(pkg, ieskf)


@pytest.fixture(scope="module")
def seq_b(pkg, ieskf):
    return run_chain_sequence(pkg, ieskf)


def assert_same_sequences(x, y):
    assert len(x) == len(y)
    for step, (p, q) in enumerate(zip(x, y)):
        for s in STREAMS:
            assert ch.same_result(p["res"][s], q["res"][s]), (step, s, p["res"][s], q["res"][s])
            assert ch.same_state(p["poses"][s], q["poses"][s]), (step, s, p["poses"][s], q["poses"][s])
        assert len(p["clouds"]) == len(q["clouds"])
        for k, (cp, cq) in enumerate(zip(p["clouds"], q["clouds"])):
            for w in range(6):
                assert cp[w].shape == cq[w].shape and np.array_equal(ch.bits(cp[w]), ch.bits(cq[w])), (step, k, w)


def test_step_equals_the_explicit_chain(seq_a, seq_b):
    assert_same_sequences(seq_a, seq_b)


def test_what_the_sequence_covers(seq_a):
    res = [[st["res"][s] for st in seq_a] for s in STREAMS]
    for s in STREAMS:
        first = res[s][0]
        # the ring is empty: no round runs, aft stays zero, the frame is saved with tobe_start (LM:1636, 1669, 1676-1686)
        assert first["iters"] == 0 and first["key_frame"] == 1 and first["ring_age"] == 0 and first["archive_id"] == 0
        assert np.array_equal(ch.bits(first["key_pose"]), ch.bits(first["tobe_start"])) and not first["transform"].any()
        for r in res[s][1:]:
            if r["key_frame"]:  # later key frames take transformAftMapped
                assert np.array_equal(ch.bits(r["key_pose"]), ch.bits(r["transform"]))
        ids = [r["archive_id"] for r in res[s] if r["key_frame"]]
        assert ids == list(range(len(ids)))
    assert all(r["iters"] > 0 for s in STREAMS for r in res[s][1:] if r["status"] == 0)  # one frame in the ring suffices here
    assert any(r["status"] == 0 and not r["key_frame"] for r in res[0]), "stream 0 made every scan a key frame"
    print("key frames per stream over %d scans: %s (window %d)" % (len(seq_a), [sum(r["key_frame"] for r in res[s]) for s in STREAMS], ch.WINDOW))
    # (how many scans become key frames is scan-to-map's answer, not the drift's alone: a ring that WRAPS is made
    # certain in test_set_pose_in_mid_sequence_is_honoured)
    # the interval gate: stream 2's scan 4 repeats a time stamp — skipped, and nothing of the stream changes
    assert [r["status"] for r in res[2]] == [0, 0, 0, 0, defs.MAP_STEP_SKIPPED, 0, 0, 0]
    assert ch.same_state(seq_a[4]["poses"][2], seq_a[3]["poses"][2]) and len(seq_a[4]["clouds"]) == 2
    assert all(st["ms"][0] > 0 and st["ms"][1] > 0 for st in seq_a)


def test_the_same_sequence_on_a_fresh_context_gives_the_same_bits(pkg, ieskf, seq_a):
    again = run_step_sequence(pkg, ieskf, steps=5)
    assert_same_sequences(again, seq_a[:5])


def test_set_pose_in_mid_sequence_is_honoured(pkg, ieskf):
    moved = dict(bef=[0.01, 0.02, -0.01, 0.1, 0.0, 0.5], aft=[0.02, 0.03, 0.0, 0.3, -0.1, 0.9], tobe=[0.02, 0.03, 0.0, 0.3, -0.1, 0.9],
                 last=[0.02, 0.03, 0.0, 0.3, -0.1, 0.9], prev=[0.3, -0.1, 0.9], n_frames=2, last_time=0.45)

    def hook_a(a, step):
        if step == 2:
            sm.set_pose(a, 1, moved)
            got = sm.get_pose(a, 1)
            assert got["n_frames"] == 2 and got["last_time"] == 0.45 and np.array_equal(got["aft"], np.array(moved["aft"], F))
        elif step > 2:  # previousRobotPosPoint 10 m away: the key rule saves this scan whatever scan-to-map answers
            st = sm.get_pose(a, 1)
            st["prev"] = st["prev"] + F(10)
            sm.set_pose(a, 1, st)

    def hook_b(states, step):
        if step == 2:
            states[1] = {k: (np.array(v, F) if isinstance(v, list) else v) for k, v in moved.items()}
        elif step > 2:
            states[1]["prev"] = states[1]["prev"] + F(10)

    x, y = run_step_sequence(pkg, ieskf, 6, hook_a), run_chain_sequence(pkg, ieskf, 6, hook_b)
    assert_same_sequences(x, y)
    saved = [st["res"][1]["key_frame"] for st in x]
    assert saved[0] == 1 and saved[3:] == [1, 1, 1] and sum(saved) > ch.WINDOW  # the ring of stream 1 wrapped
    assert np.array_equal(x[2]["poses"][1]["bef"], ch.odometry(2)[1][0])  # (the step after set_pose ran from it)


def test_contract_cases_leave_every_state_as_it_was(pkg, ieskf):
    with ch.context(pkg, ieskf) as a, ch.context(pkg, ieskf) as b:
        L = ieskf.lib()
        for c in (a, b):
            ch.setup(c)
        with pytest.raises(RuntimeError, match="-6"):  # before lins_streams_map_init
            sm.step(a, STREAMS, ch.odoms(0))
        sm.init(a, ch.N, ch.INTERVAL)
        states = [ch.fresh_state() for _ in STREAMS]
        for step in range(3):
            for c in (a, b):
                ch.feed(c, step)
            ra, rb = sm.step(a, STREAMS, ch.odoms(step)), ch.explicit_step(b, states, STREAMS, ch.odometry(step))
            assert all(ch.same_result(p, q) for p, q in zip(ra, rb))
        before = [sm.get_pose(a, s) for s in STREAMS]
        counts = [a.archive_count(s) for s in STREAMS]
        bad = ch.odoms(3)
        bad[1].transform_sum[2] = float("nan")
        with pytest.raises(RuntimeError, match="-4"):
            sm.step(a, STREAMS, bad)
        with pytest.raises(RuntimeError, match="-1"):  # a stream twice, a stream that does not exist, more entries than streams
            sm.step(a, [0, 0], ch.odoms(3, [0, 0]))
        with pytest.raises(RuntimeError, match="-1"):
            sm.step(a, [0, 3], ch.odoms(3, [0, 1]))
        with pytest.raises(RuntimeError, match="-1"):
            sm.step(a, [0, 1, 2, 1], ch.odoms(3, [0, 1, 2, 1]))
        assert all(ch.same_state(sm.get_pose(a, s), before[s]) for s in STREAMS)
        assert [a.archive_count(s) for s in STREAMS] == counts
        assert sm.step(a, [], []) == []
        # the calls the step is made of still work on this context, and return what the other context's return
        sa, sb = a.local_map_build_streams(STREAMS, STREAMS), b.local_map_build_streams(STREAMS, STREAMS)
        assert sa == sb
        t0 = [before[s]["aft"] for s in STREAMS]
        ga, gb = (c.scan2map_batch([defs.MapProblem.local(t) for t in t0]) for c in (a, b))
        for p, q in zip(ga, gb):
            assert np.array_equal(ch.bits(p["transform"]), ch.bits(q["transform"]))
            assert (p["iters"], p["converged"], p["degenerate"], p["n_sel"]) == (q["iters"], q["converged"], q["degenerate"], q["n_sel"])
        for k in STREAMS:
            for w in range(6):
                assert np.array_equal(ch.bits(a.local_map_download(k, w)), ch.bits(b.local_map_download(k, w)))
        # ... and a subset of the streams, in another order, steps as the chain does
        for c in (a, b):
            ch.feed(c, 3)
        ra, rb = sm.step(a, [2, 0], ch.odoms(3, [2, 0])), ch.explicit_step(b, states, [2, 0], [ch.odometry(3)[s] for s in (2, 0)])
        assert all(ch.same_result(p, q) for p, q in zip(ra, rb))
        assert all(ch.same_state(sm.get_pose(a, s), states[s]) for s in STREAMS)
