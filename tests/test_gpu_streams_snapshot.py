"""Moving a stream between contexts (include/lins_snapshot.h), on the harness of tests/test_gpu_streams_retire.py: three
streams in machine mode with local map, archive, pose graph and loop mode (a second variant: surround mode), driven by
lins_streams_slam_step on the sequences of tests/boot_common.py; the map interval is half a sweep.
  context B  runs all sweeps and never moves anything (it takes one snapshot of stream 1 before sweep K, for the
             canonical-form check; the read-only test holds a context that snapshots three times against it)
  context A  runs K sweeps, snapshots stream 1 and retires it: its streams 0 and 2 equal B's on every sweep
  context D  is fresh; its streams 0 and 1 are given other sequences from their sweep 0 and sit in INIT / FIRST_SCAN
             beside the newcomer; the blob is restored into slot 2.  D's stream 2 equals B's stream 1 bit for bit: every
             sweep's results, and at the end the map pose, archive, surround list or pose graph, a local-map build, a
             pose-graph solve and the loop thread's step.
K = 6 (the retire test's 4 leave stream 1 with one key frame: the sequences move 0.1 - 0.3 m a sweep and map from sweep 2
on, so the second key frame comes by sweep 5).  Loop mode: the sequences close no loop by then, so A and B each add one
by hand (lins_pose_graph_add_loop between the newest frame and frame 0), solve and apply before the snapshot: the solved
increments that live on the device alone travel in the blob, and the solve at the end starts from them.
All comparisons are bit for bit."""
import importlib

import numpy as np
import pytest

import boot_common as bc
import map_step_chain as ch
from map_step_chain import defs, host, sm

pytestmark = pytest.mark.gpu
PKG = "lins---lidar-inertial-slam_amd"
sl = importlib.import_module(PKG + ".streams_slam")
ieskf_mod = importlib.import_module(PKG + ".ieskf")
LinsError = ieskf_mod.LinsError

N, K, AFTER, WINDOW, MAX_PTS, INTERVAL = 3, 6, 4, ch.WINDOW, ch.MAX_PTS, 0.05
SWEEPS = K + AFTER
MAX_FRAMES = 2 * SWEEPS
MOVED, TO = 1, 2
KEPT = (0, 2)
INIT, FIRST_SCAN, RUNNING = 0, 1, 3
E_ARG, E_CAPACITY, E_INPUT, E_STATE = "error -1:", "error -3:", "error -4:", "error -6:"
IDENT = (0, 1, 2)   # who[s]: the logical stream whose sequence and IMU angles slot s is given
IN_D = (0, 2, 1)    # context D: slot 2 continues logical stream 1; slots 0 and 1 start sequences 0 and 2 from their sweep 0


@pytest.fixture(scope="module")
def data():
    return [bc.load(host, s, SWEEPS) for s in bc.SEQS]


def context(pkg, ieskf, num_iter=8):
    return ieskf.IeskfContext(pkg.default_params(num_iter=num_iter), max_batch=N, max_targets=16384)


def init(c, mode, window=WINDOW, max_frames=MAX_FRAMES, graph=True):
    c.streams_init(N)
    c.streams_machine_init()
    c.local_map_init(N, window, MAX_PTS)
    c.archive_init(N, max_frames, 1 << 20)
    sm.init(c, N, INTERVAL)
    if mode == "loop":
        if graph:
            c.pose_graph_init(N, MAX_FRAMES, 2)
            sm.loop(c, True)
    else:
        sm.surround(c, True, 50.0, 1.0)


def imu_of(logical, k):
    return sl.slam_imu(0.01 * k, -0.02 * k, True) if logical == 1 else sl.slam_imu()


def sweep(c, data, who, at, k):
    """one lins_streams_slam_step at the time of sweep k: slot s is given sweep at[s] of logical stream who[s]"""
    raws = [data[who[s]]["raws"][at[s]] for s in range(N)]
    rows = [data[who[s]]["rows"][at[s]] for s in range(N)]
    return sl.slam_step(c, raws, rows, [bc.scan_time(k)] * N, imu_rp=[imu_of(who[s], k) for s in range(N)])


def stream_bits(out, s):
    """everything a sweep returned for stream s, floats by their bits"""
    res, status, mp, fused = out
    r = res[s]
    m = {f: (v.tobytes() if isinstance(v, np.ndarray) else v) for f, v in mp[s].items()}
    return ((r.state.tobytes(), r.cov.tobytes(), r.iters, r.converged, r.diverged, r.m_surf, r.m_corner, r.reserved[0], r.residual_norm,
             r.update_norm), int(status[s]), m, fused[s]["transform_mapped"].tobytes(), fused[s]["orientation"].tobytes())


def pose_bits(c, s):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in sm.get_pose(c, s).items()}


def frozen(x):
    if isinstance(x, dict):
        return tuple((k, frozen(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, np.ndarray):
        return x.tobytes()
    return x.hex() if isinstance(x, float) else x


def hand_loop(c, slot):
    """one loop factor between the newest frame and frame 0, a solve and the write-back (the same calls on every context)"""
    n = c.pose_graph_count(slot)[0]
    assert n >= 2, n
    p = c.pose_graph_poses(slot)[n - 1] + np.array([0.02, -0.01, 0.01, 0.001, -0.002, 0.003], np.float32)
    c.pose_graph_add_loop(slot, n - 1, 0, tuple(float(v) for v in p), 0.3)
    (r,) = c.pose_graph_solve([slot])
    assert r["status"] == 0 and r["iterations"] >= 1
    c.pose_graph_apply(slot, slot)
    return frozen(r)


def final_facts(c, ieskf, mode, slot):
    """what is compared at the end, for the stream in `slot` (the calls change the context: made last, in this order)"""
    f = dict(pose=pose_bits(c, slot), archive=c.archive_count(slot), status=int(c.streams_status()[slot]))
    sizes = c.local_map_build_streams([slot], [slot])
    f["local_map"] = (frozen(sizes), [c.local_map_download(0, w).tobytes() for w in range(6)])
    if mode == "loop":
        f["graph"] = c.pose_graph_count(slot)
        f["graph_poses"] = c.pose_graph_poses(slot).tobytes()
        f["solve"] = frozen(c.pose_graph_solve([slot]))
        prm = defs.loop_step_params(ieskf.lib(), search_radius=50.0, min_gap_s=0.25)
        f["loop_step"] = frozen(c.loop_step([defs.loop_step_entry(slot, None, bc.scan_time(SWEEPS - 1), stream=slot)], prm))
        f["graph_after"] = (c.pose_graph_count(slot), c.pose_graph_poses(slot).tobytes(), pose_bits(c, slot))
    else:
        f["surround"] = sm.surround_list(c, slot)
    return f


def reference(pkg, ieskf, data, mode):
    """context B: the sweeps' outputs, stream 1's blob before sweep K, the final facts of stream 1"""
    with context(pkg, ieskf) as b:
        init(b, mode)
        outs, extra = [], None
        for k in range(SWEEPS):
            if k == K:
                extra = hand_loop(b, MOVED) if mode == "loop" else None
                (blob,) = b.streams_snapshot([MOVED])
            outs.append(sweep(b, data, IDENT, [k] * N, k))
        return dict(outs=outs, blob=blob, hand=extra, final=final_facts(b, ieskf, mode, MOVED))


@pytest.fixture(scope="module")
def ref_loop(pkg, ieskf, data):
    return reference(pkg, ieskf, data, "loop")


@pytest.fixture(scope="module")
def ref_surround(pkg, ieskf, data):
    return reference(pkg, ieskf, data, "surround")


def run_a_to_k(a, data, mode, ref):
    """A's first K sweeps (equal to B's), the hand-made loop in loop mode"""
    for k in range(K):
        out = sweep(a, data, IDENT, [k] * N, k)
        for s in range(N):
            assert stream_bits(out, s) == stream_bits(ref["outs"][k], s), (k, s)
    if mode == "loop":
        assert hand_loop(a, MOVED) == ref["hand"]


def continue_in_d(d, data, ref, first=K, n=AFTER, sweeps_of_neighbours=0):
    """D's sweeps first .. first + n - 1: its slot 2 equals B's stream 1 on every one; the neighbours take their sequences
    from their own sweep sweeps_of_neighbours on"""
    for j in range(n):
        k = first + j
        out = sweep(d, data, IN_D, [sweeps_of_neighbours + j, sweeps_of_neighbours + j, k], k)
        assert stream_bits(out, TO) == stream_bits(ref["outs"][k], MOVED), k
    return out


def move(pkg, ieskf, data, mode, ref, how):
    with context(pkg, ieskf) as a, context(pkg, ieskf) as d:
        init(a, mode), init(d, mode)
        run_a_to_k(a, data, mode, ref)
        assert list(a.streams_status()) == [RUNNING] * N and a.archive_count(MOVED) >= 1
        if how == "migrate":
            a.streams_migrate(MOVED, d, TO)
        else:
            (blob,) = a.streams_snapshot([MOVED])
            assert blob == ref["blob"]  # canonical: A's blob is B's, byte for byte
            info = ieskf_mod.snapshot_info(blob)
            want = defs.SNAP_STREAM | defs.SNAP_FILTER | defs.SNAP_BOOT | defs.SNAP_ODOM | defs.SNAP_MAP_POSE | defs.SNAP_RING | defs.SNAP_ARCHIVE
            assert info["modules"] == want | (defs.SNAP_GRAPH if mode == "loop" else 0)
            assert info["counts"]["has_scan"] and info["counts"]["archive_frames"] == a.archive_count(MOVED) and info["counts"]["ring_frames"] >= 1
            if mode == "loop":
                assert info["counts"]["graph_loops"] == 1 and info["counts"]["graph_up_frames"] == info["counts"]["graph_frames"] >= 2
            a.streams_retire([MOVED])
            d.streams_restore([TO], [blob])
        assert d.streams_snapshot([TO]) == [ref["blob"]]  # ... and so is the blob of D's slot right after the restore
        assert a.streams_status()[MOVED] == INIT and a.archive_count(MOVED) == 0
        assert list(d.streams_status()) == [INIT, INIT, RUNNING]
        for j in range(AFTER):  # A's streams 0 and 2 go on as B's (its slot 1 starts anew: any clouds)
            k = K + j
            out = sweep(a, data, IDENT, [k, j, k], k)
            for s in KEPT:
                assert stream_bits(out, s) == stream_bits(ref["outs"][k], s), (k, s)
        out = continue_in_d(d, data, ref)
        assert [int(x) for x in out[1]][:2] != [INIT, INIT]  # the neighbours went through their bootstrap beside it
        assert final_facts(d, ieskf, mode, TO) == ref["final"]


def test_move_with_loop_mode(pkg, ieskf, data, ref_loop):
    move(pkg, ieskf, data, "loop", ref_loop, "three calls")


def test_move_with_surround_mode(pkg, ieskf, data, ref_surround):
    assert ref_surround["final"]["surround"] != []
    move(pkg, ieskf, data, "surround", ref_surround, "three calls")


def test_migrate_equals_the_three_calls(pkg, ieskf, data, ref_loop):
    move(pkg, ieskf, data, "loop", ref_loop, "migrate")


def test_snapshot_reads_only_and_round_trip_in_place(pkg, ieskf, data, ref_loop):
    """A snapshots before sweeps K, K + 1 and K + 2 and retires nothing; before sweep K + 2 it also retires stream 1 and
    restores it into its own slot — the frames now lie at the arena's end: A equals B in all three streams throughout"""
    with context(pkg, ieskf) as a:
        init(a, "loop")
        run_a_to_k(a, data, "loop", ref_loop)
        for k in range(K, SWEEPS):
            if k <= K + 2:
                blobs = a.streams_snapshot([0, 1, 2])
                assert blobs[MOVED] == ref_loop["blob"] or k > K
            if k == K + 2:
                used = a.archive_usage()
                a.streams_retire([MOVED])
                assert a.streams_status()[MOVED] == INIT and a.archive_usage()[0] < used[0]
                a.streams_restore([MOVED], [blobs[MOVED]])
                assert a.archive_usage() == used and a.streams_snapshot([0, 1, 2]) == blobs
            out = sweep(a, data, IDENT, [k] * N, k)
            for s in range(N):
                assert stream_bits(out, s) == stream_bits(ref_loop["outs"][k], s), (k, s)
        assert final_facts(a, ieskf, "loop", MOVED) == ref_loop["final"]


@pytest.mark.parametrize("k_snap", [0, 1, 2])
def test_every_state_of_the_machine(pkg, ieskf, data, ref_surround, k_snap):
    """the snapshot taken with 0, 1, 2 sweeps run: INIT, FIRST_SCAN, the first RUNNING scan"""
    with context(pkg, ieskf) as a, context(pkg, ieskf) as d:
        init(a, "surround"), init(d, "surround")
        for k in range(k_snap):
            sweep(a, data, IDENT, [k] * N, k)
        assert a.streams_status()[MOVED] == (INIT, FIRST_SCAN, RUNNING)[k_snap]
        (blob,) = a.streams_snapshot([MOVED])
        d.streams_restore([TO], [blob])
        assert d.streams_status()[TO] == (INIT, FIRST_SCAN, RUNNING)[k_snap] and d.streams_snapshot([TO]) == [blob]
        continue_in_d(d, data, ref_surround, first=k_snap, n=AFTER)


def test_a_fresh_slot_restores_to_a_fresh_slot(pkg, ieskf, data, ref_loop):
    with context(pkg, ieskf) as a, context(pkg, ieskf) as d:
        init(a, "loop"), init(d, "loop")
        sl.odometry(d)  # (D's odometry records exist, so that lins_streams_fuse can say "no valid record")
        (blob,) = a.streams_snapshot([MOVED])
        assert not ieskf_mod.snapshot_info(blob)["counts"]["has_scan"]
        d.streams_restore([TO], [blob])
        # the checks of test_gpu_streams_retire.py retired_slot_is_fresh
        assert d.streams_status()[TO] == INIT and d.archive_count(TO) == 0 and d.pose_graph_count(TO) == (0, 0)
        with pytest.raises(LinsError, match=E_INPUT):
            sl.fuse(d, [TO])
        with pytest.raises(LinsError, match=E_ARG):
            d.local_map_set_pose(TO, 0, (0.0,) * 6)
        with pytest.raises(LinsError, match=E_STATE):
            d.streams_map_cloud(TO, 0)
        with pytest.raises(LinsError, match=E_STATE):
            d.streams_filter_get(TO)
        assert pose_bits(d, TO) == {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in ch.fresh_state().items()}
        for k in range(3):  # ... and it starts as B's stream 1 did
            out = sweep(d, data, IN_D, [k] * N, k)
            assert stream_bits(out, TO) == stream_bits(ref_loop["outs"][k], MOVED), k


def test_without_machine_mode(pkg, ieskf, data):
    """a by-hand start (lins_streams_step_raw + lins_streams_filter_set) and IMU steps, as test_release_without_machine_mode:
    stream 1 moves into slot 2 of a context whose slot was released, and continues as in the context it left"""
    eye = np.tile(np.eye(18)[None] * 1e-4, (N, 1, 1))

    def start(c, who, streams):
        boots = [host.boot_first(bc.imu_last(data[w], 0), bc.scan_time(0)) for w in who]
        c.streams_step_raw([data[w]["raws"][0] for w in who], np.stack([np.array(b[1]) for b in boots]), eye)
        for k in streams:
            c.streams_filter_set(k, boots[k][0], np.array(boots[k][1]))

    def imu_step(c, who, at):
        res, counts, g = c.streams_step_imu_raw([data[who[s]]["raws"][at[s]] for s in range(N)], [data[who[s]]["rows"][at[s]] for s in range(N)])
        return [((r.state.tobytes(), r.cov.tobytes(), r.iters, r.converged, r.diverged, r.m_surf, r.m_corner, r.reserved[0]),
                 np.asarray(counts).reshape(N, -1)[s].tobytes(), np.asarray(g)[s].tobytes()) for s, r in enumerate(res)]

    with context(pkg, ieskf) as a, context(pkg, ieskf) as b, context(pkg, ieskf) as d:
        for x in (a, b, d):
            x.streams_init(N)
        start(a, IDENT, range(N)), start(b, IDENT, range(N))
        for k in (1, 2):
            assert imu_step(a, IDENT, [k] * N) == imu_step(b, IDENT, [k] * N)
        (blob,) = a.streams_snapshot([MOVED])
        assert b.streams_snapshot([MOVED]) == [blob]
        info = ieskf_mod.snapshot_info(blob)
        assert info["modules"] == defs.SNAP_STREAM | defs.SNAP_FILTER and info["counts"]["has_scan"] and not info["facts"]["machine"]
        start(d, IN_D, (0, 1))
        with pytest.raises(LinsError, match=E_STATE):  # the slot holds a resident scan
            d.streams_restore([TO], [blob])
        d.streams_release([TO])
        d.streams_restore([TO], [blob])
        assert d.streams_snapshot([TO]) == [blob]
        fa, fd = a.streams_filter_get(MOVED), d.streams_filter_get(TO)
        assert fa[0].state[:] == fd[0].state[:] and fa[0].cov[:] == fd[0].cov[:] and np.array_equal(fa[1], fd[1])
        for j in (1, 2):
            ob, od = imu_step(b, IDENT, [2 + j] * N), imu_step(d, IN_D, [j, j, 2 + j])
            assert od[TO] == ob[MOVED], j
            assert od[TO][0][2] > 0  # the update ran


def test_migrate_into_a_taken_slot_is_refused(pkg, ieskf, data, ref_loop):
    with context(pkg, ieskf) as a, context(pkg, ieskf) as d:
        init(a, "loop"), init(d, "loop")
        run_a_to_k(a, data, "loop", ref_loop)
        sweep(d, data, IDENT, [0] * N, 0)
        with pytest.raises(LinsError, match=E_STATE):
            a.streams_migrate(MOVED, d, TO)
        with pytest.raises(LinsError, match=E_ARG):
            a.streams_migrate(MOVED, a, MOVED)
        assert list(a.streams_status()) == [RUNNING] * N and list(d.streams_status()) == [FIRST_SCAN] * N
        for k in range(K, K + 2):
            out = sweep(a, data, IDENT, [k] * N, k)
            for s in range(N):
                assert stream_bits(out, s) == stream_bits(ref_loop["outs"][k], s), (k, s)


def test_refusals_change_nothing(pkg, ieskf, data, ref_loop):
    """every refusal has the status of include/lins_snapshot.h, and the refusing context's next sweep equals that of a
    control context of the same configuration that never saw the call"""
    blob = ref_loop["blob"]
    frames = ieskf_mod.snapshot_info(blob)["counts"]["archive_frames"]
    flipped = bytearray(blob)
    flipped[len(blob) - 100] ^= 0x04

    def refused(configure, calls, warm=0):
        with context(pkg, ieskf, **configure.get("ctx", {})) as d, context(pkg, ieskf, **configure.get("ctx", {})) as control:
            for x in (d, control):
                init(x, configure.get("mode", "loop"), **configure.get("init", {}))
                for k in range(warm):
                    sweep(x, data, IDENT, [k] * N, k)
            for slot, b, err in calls:
                with pytest.raises(LinsError, match=err):
                    d.streams_restore([slot], [b])
            od, oc = sweep(d, data, IDENT, [warm] * N, warm), sweep(control, data, IDENT, [warm] * N, warm)
            for s in range(N):
                assert stream_bits(od, s) == stream_bits(oc, s), s
            assert [d.archive_count(s) for s in range(N)] == [control.archive_count(s) for s in range(N)]

    # a destination slot that is not fresh; a truncated blob; a flipped byte; a slot out of range
    refused({}, [(0, blob, E_STATE), (TO, blob[:len(blob) - 1], E_INPUT), (TO, blob[:400], E_INPUT), (TO, bytes(flipped), E_INPUT), (N, blob, E_ARG)],
            warm=1)
    refused(dict(init=dict(graph=False)), [(TO, blob, E_STATE)])         # a blob with a pose graph, a context without one
    refused(dict(mode="surround"), [(TO, blob, E_STATE)])                # loop / surround mismatch
    refused(dict(ctx=dict(num_iter=9)), [(TO, blob, E_STATE)])           # another num_iter
    refused(dict(init=dict(window=WINDOW - 1)), [(TO, blob, E_STATE)])   # a ring window one smaller: a context-wide fact
    refused(dict(init=dict(max_frames=frames - 1)), [(TO, blob, E_CAPACITY)])  # one key frame too few
    with context(pkg, ieskf) as a:  # caps one byte short: the sizes are reported, the context goes on as B
        init(a, "loop")
        run_a_to_k(a, data, "loop", ref_loop)
        with pytest.raises(LinsError, match=E_CAPACITY):
            a.streams_snapshot([MOVED], caps=[len(blob) - 1])
        assert a._snapshot_bytes == [len(blob)]
        out = sweep(a, data, IDENT, [K] * N, K)
        for s in range(N):
            assert stream_bits(out, s) == stream_bits(ref_loop["outs"][K], s), s
