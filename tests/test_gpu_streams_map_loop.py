"""lins_streams_map_loop: with it on, lins_streams_map_step makes saveKeyFramesAndFactor's factor (LM:1673-1705) for every
key frame it stores — the graph of slot = stream stays in step with the archive — and remembers currentRobotPosPoint for
LINS_LOOP_CENTRE_STREAM.  Three streams over the 8 scans and odometry rows of tests/map_step_chain.py; a second context
with the mode off and a graph initialised gives the same step results and leaves the graph empty."""
import numpy as np
import pytest

import map_step_chain as ch
from loop_step_cases import frozen as lsc_frozen
from map_step_chain import defs, host, sm

pytestmark = pytest.mark.gpu
F = np.float32
STREAMS = [0, 1, 2]
MAX_FRAMES = 2 * ch.STEPS


def prepared(pkg, ieskf, loop):
    c = ch.context(pkg, ieskf)
    ch.setup(c)
    sm.init(c, ch.N, ch.INTERVAL)
    c.pose_graph_init(ch.N, MAX_FRAMES, 0)  # (no room for a loop: a loop step stops behind its detection)
    if loop:
        sm.loop(c, True)
    return c


@pytest.fixture(scope="module")
def runs(pkg, ieskf):
    """per step of context A (mode on): results, transformLast before the step, graph poses; context B (mode off): results"""
    a, b = prepared(pkg, ieskf, True), prepared(pkg, ieskf, False)
    out = []
    try:
        for step in range(ch.STEPS):
            ch.feed(a, step)
            ch.feed(b, step)
            last = [sm.get_pose(a, s)["last"] for s in STREAMS]
            res = sm.step(a, STREAMS, ch.odoms(step))
            out.append(dict(res=res, last=last, off=sm.step(b, STREAMS, ch.odoms(step)), counts=[a.pose_graph_count(s) for s in STREAMS],
                            n_frames=[sm.get_pose(a, s)["n_frames"] for s in STREAMS], poses=[a.pose_graph_poses(s) for s in STREAMS],
                            f64=[a.debug_pose_graph_poses_f64(s) for s in STREAMS], archive=[a.archive_count(s) for s in STREAMS],
                            off_counts=[b.pose_graph_count(s) for s in STREAMS]))
        yield a, b, out
    finally:
        a.close()
        b.close()


def test_the_graph_stays_in_step_with_the_archive(runs):
    _, _, out = runs
    graphs = [host.PoseGraph(MAX_FRAMES, 2) for _ in STREAMS]
    keys = [[] for _ in STREAMS]
    for step, o in enumerate(out):
        for s in STREAMS:
            r = o["res"][s]
            if r["key_frame"]:
                # the id the graph gave is the archive's: frames so far
                assert r["archive_id"] == len(keys[s]) == graphs[s].push(o["last"][s] if keys[s] else None, r["key_pose"])
                keys[s].append(ch.key_pose_of(r["key_pose"]))
            assert o["counts"][s] == (o["n_frames"][s], 0) and o["n_frames"][s] == len(keys[s]) == o["archive"][s], (step, s)
            assert np.array_equal(ch.bits(o["poses"][s]), ch.bits(np.array(keys[s], F).reshape(-1, 6))), (step, s)
            assert np.array_equal(o["f64"][s], graphs[s].poses_f64()), (step, s)
    assert [len(k) for k in keys] == [o for o in out[-1]["archive"]] and all(len(k) >= 3 for k in keys)
    # not every scan is a key frame: an odometry factor spans the scans between two (last6 is transformLast, the last key pose)
    assert any(len(k) < ch.STEPS for k in keys)


def test_off_is_todays_step_and_leaves_the_graph_alone(runs):
    _, _, out = runs
    for step, o in enumerate(out):
        for s in STREAMS:
            assert ch.same_result(o["res"][s], o["off"][s]), (step, s)
        assert o["off_counts"] == [(0, 0)] * ch.N


def test_centre_stream_is_the_last_ok_steps_position(runs, ieskf):
    a, _, out = runs
    prm = defs.loop_step_params(ieskf.lib(), search_radius=50.0, min_gap_s=0.5)
    now = ch.odometry(ch.STEPS - 1)[0][1]
    last_ok = [[o["res"][s] for o in out if o["res"][s]["status"] == 0][-1] for s in STREAMS]
    flagged = a.loop_step([defs.loop_step_entry(s, None, now, stream=s) for s in STREAMS], prm)
    explicit = a.loop_step([defs.loop_step_entry(s, last_ok[s]["transform"][3:6], now, stream=s) for s in STREAMS], prm)
    assert any(r["closest_id"] >= 0 and r["status"] == -3 for r in flagged)  # the search found frames: the centre mattered
    for s in STREAMS:
        assert lsc_frozen(flagged[s]) == lsc_frozen(explicit[s]), s
        assert flagged[s]["latest_id"] == out[-1]["archive"][s] - 1 and flagged[s]["outcome"] == defs.LOOP_NONE
        # ... and is not any centre: the search from far away finds nothing
        far = a.loop_step([defs.loop_step_entry(s, last_ok[s]["transform"][3:6] + F(1000.0), now, stream=s)], prm)[0]
        assert far["closest_id"] == -1


def test_a_stream_that_has_not_stepped_and_the_switch(pkg, ieskf):
    with ch.context(pkg, ieskf) as c:
        ch.setup(c)
        with pytest.raises(ieskf.LinsError, match="error -6"):  # before lins_streams_map_init
            sm.loop(c, True)
        sm.init(c, ch.N, ch.INTERVAL)
        with pytest.raises(ieskf.LinsError, match="error -6"):  # before lins_pose_graph_init
            sm.loop(c, True)
        c.pose_graph_init(ch.N - 1, MAX_FRAMES, 2)
        with pytest.raises(ieskf.LinsError, match="error -6"):  # fewer slots than streams
            sm.loop(c, True)
        c.pose_graph_init(ch.N, MAX_FRAMES, 2)
        sm.loop(c, True)
        prm = defs.loop_step_params(ieskf.lib())
        with pytest.raises(ieskf.LinsError, match="error -6"):  # LINS_LOOP_CENTRE_STREAM: the stream has not completed a step
            c.loop_step([defs.loop_step_entry(0, None, 0.0, stream=0)], prm)
        ch.feed(c, 0)
        res = sm.step(c, [1], ch.odoms(0, [1]))
        assert res[0]["key_frame"] == 1 and c.pose_graph_count(1) == (1, 0)
        assert c.loop_step([defs.loop_step_entry(1, None, 0.0, stream=1)], prm)[0]["outcome"] == defs.LOOP_NONE
        with pytest.raises(ieskf.LinsError, match="error -6"):
            c.loop_step([defs.loop_step_entry(0, None, 0.0, stream=0)], prm)
        sm.loop(c, False)
        st = sm.get_pose(c, 1)
        st["prev"] = st["prev"] + F(100.0)  # previousRobotPosPoint moved away: the next scan is a key frame for certain
        sm.set_pose(c, 1, st)
        ch.feed(c, 1)
        res = sm.step(c, [1], ch.odoms(1, [1]))
        assert res[0]["key_frame"] == 1 and c.pose_graph_count(1) == (1, 0) and c.archive_count(1) == 2
        with pytest.raises(ieskf.LinsError, match="error -6"):  # graph and archive are out of step now
            sm.loop(c, True)
