"""A mapping call's bits do not depend on what its context ran before (the rule of DESIGN.md 5.3: every kernel reads
scratch only where the same call wrote it).  tests/test_gpu_context_state.py holds the IESKF update path to this; here
the mapping side — local-map and surround builds, archive assemblies, scan-to-map, the loop-closure ICP, key-pose
selection, the front end and the streams' map step — whose device scratch grows and is never cleared, and whose kernels
return early for the part of a table the current call does not use.

Each test runs a call Y on a fresh context and on a context that first ran a LARGER warm-up X, and compares every
output bit for bit: cloud bytes and every field of the size, info and result records.  There is no tolerance — the two
runs execute the same code on the same inputs.  Where a CPU restatement of the call exists Y is held to it too, under
the bar the call's own test uses.  tests/mapping_state_cases.py builds X and Y; tests/test_mapping_state_inputs.py
asserts that X exceeds Y in every dimension an allocation is sized by, so that a stale read stays inside memory X wrote."""
import numpy as np
import pytest

import loop_icp_cases as icp_cases
import map_step_chain as ch
import mapping_state_cases as mc
from map_step_chain import defs, sm
from map_synth import SCAN2MAP_BAR
from test_gpu_features import bits as feature_bits
from test_gpu_loop_icp import COUNTS as ICP_COUNTS, result_bits as icp_bits
from test_gpu_segmentation import bits as segment_bits

pytestmark = pytest.mark.gpu
F = np.float32
HOST, DEVICE = defs.KEYPOSES_HOST, defs.KEYPOSES_DEVICE


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def make(pkg, ieskf):
    return ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)


def same_cloud(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def assert_same_builds(what, got, want):
    """[(sizes, six clouds)] of two builds: every field of the size records, every cloud byte"""
    assert len(got) == len(want)
    nbytes = 0
    for k, ((gs, gc), (ws, wc)) in enumerate(zip(got, want)):
        assert gs == ws, (what, k, gs, ws)
        for c in range(6):
            assert same_cloud(gc[c], wc[c]), (what, k, c)
            nbytes += gc[c].nbytes
    print("%s: %d entries, %d clouds, %d bytes and the size records, bit for bit" % (what, len(got), 6 * len(got), nbytes))


def built(c, sizes):
    return [(sizes[k], [c.local_map_download(k, w) for w in range(6)]) for k in range(len(sizes))]


# ---- ring builds -----------------------------------------------------------------------------------------------------------
def ring_context(pkg, ieskf, cfg, sides):
    c = make(pkg, ieskf)
    c.local_map_init(cfg["n_slots"], cfg["window"], cfg["max_pts"])
    for side in sides:
        for s in side["slots"]:
            for f in side["frames"][s]:
                c.local_map_push(s, *f)
    return c


def ring_build(c, side):
    return built(c, c.local_map_build(side["slots"], side["scans"]))


@pytest.mark.parametrize("which", ["larger windows first", "four-pass jobs first"])
def test_ring_build(pkg, ieskf, host, which):
    pair, cfg = (mc.ring_pair(), mc.RING) if which == "larger windows first" else (mc.ring_pass_pair(), dict(n_slots=5, window=50, max_pts=4096))
    x, y = pair["X"], pair["Y"]
    with ring_context(pkg, ieskf, cfg, [y]) as fresh:
        want = ring_build(fresh, y)
    with ring_context(pkg, ieskf, cfg, [x, y]) as warm:
        warm_x = ring_build(warm, x)
        got = ring_build(warm, y)
    assert all(s["status"] == 0 for s, _ in warm_x)
    assert_same_builds("ring build after a larger one", got, want)
    restated = [host.local_map(y["frames"][s], sc, cfg["window"]) for s, sc in zip(y["slots"], y["scans"])]
    assert_same_builds("ring build against host.local_map", got, [(ws, w) for w, ws in restated])
    if which == "larger windows first":
        assert [s["status"] for s, _ in got] == [0, -3, 0, 0]
        assert got[0][0]["n"] == [0] * 6 and got[0][0]["frames"] == 0  # the empty ring with empty scan clouds
        assert got[1][0]["n"] == [0] * 6 and all(len(c) == 0 for c in got[1][1])  # the refusal: same status, zero sizes
    else:
        assert all(s["status"] == 0 for s, _ in got) and all(s["n"][0] == 1 for s, _ in got)  # (the zero-pass corner maps)


# ---- surround builds with split scans ----------------------------------------------------------------------------------
def archive_context(pkg, ieskf, local=True):
    c = make(pkg, ieskf)
    if local:
        c.local_map_init(mc.ARCHIVE["n_slots"], 3, 4096)
    c.archive_init(mc.ARCHIVE["n_slots"], mc.ARCHIVE["max_frames"], mc.ARCHIVE["max_points"])
    for s, frames in mc.archive_frames().items():
        for i, f in enumerate(frames):
            assert c.archive_push(s, *f, time=float(i)) == i
    return c


def surround_build(c, side):
    return built(c, c.local_map_build_surround(side["slots"], side["lists"], side["scans"]))


def test_surround_build_with_split_scans(pkg, ieskf, host):
    pair = mc.surround_pair()
    x, y = pair["X"], pair["Y"]
    fresh = {}
    for chunk in (mc.SURROUND_CHUNK, mc.INT_MAX):
        with archive_context(pkg, ieskf) as c:
            c.archive_set_scan_chunk(chunk)
            fresh[chunk] = surround_build(c, y)
            c.archive_set_scan_chunk(0)
    fr = mc.archive_frames()
    restated = [host.surround_map(fr[s], lst, sc) for s, lst, sc in zip(y["slots"], y["lists"], y["scans"])]
    with archive_context(pkg, ieskf) as warm:
        try:
            warm.archive_set_scan_chunk(mc.SURROUND_CHUNK)
            warm_x = surround_build(warm, x)
            assert all(s["status"] == 0 and s["frames"] == 12 for s, _ in warm_x)
            got = surround_build(warm, y)
            assert_same_builds("surround build (fewer chunks, fewer split jobs) after a larger one", got, fresh[mc.SURROUND_CHUNK])
            warm.archive_set_scan_chunk(mc.INT_MAX)
            unsplit = surround_build(warm, y)
            assert_same_builds("surround build without a split after split ones", unsplit, fresh[mc.INT_MAX])
        finally:
            warm.archive_set_scan_chunk(0)
    assert_same_builds("surround build against host.surround_map", got, [(ws, w) for w, ws in restated])
    assert_same_builds("split against unsplit", got, unsplit)


# ---- archive assemblies ------------------------------------------------------------------------------------------------
def assemble(c, specs):
    infos = c.archive_assemble(specs)
    return [(infos[k], c.archive_download(k)) for k in range(len(specs))]


def test_archive_assemblies(pkg, ieskf, host):
    pair = mc.assembly_pair()
    with archive_context(pkg, ieskf, local=False) as fresh:
        want = assemble(fresh, pair["Y"])
    with archive_context(pkg, ieskf, local=False) as warm:
        warm_x = assemble(warm, pair["X"])
        got = assemble(warm, pair["Y"])
    assert all(i["status"] == 0 and i["n"] > 0 for i, _ in warm_x)
    fr = mc.archive_frames()
    nbytes = 0
    for k, (sp, (gi, gc), (wi, wc)) in enumerate(zip(pair["Y"], got, want)):
        assert gi == wi and same_cloud(gc, wc), (k, gi, wi)
        hc, hi = host.submap(fr[sp["slot"]], sp["ids"], sp["clouds"], sp["leaf"], sp["flags"])
        assert gi == hi and same_cloud(gc, hc), (k, gi, hi)
        nbytes += gc.nbytes
    print("archive assembly after a larger one: %d entries, %d bytes and the info records, bit for bit; = host.submap" % (len(got), nbytes))
    assert got[0][0]["n"] < got[0][0]["points_in"]  # (DROP_NEGATIVE dropped some)


# ---- scan-to-map ---------------------------------------------------------------------------------------------------------
FIELDS = ("iters", "converged", "degenerate", "n_sel")


def assert_same_results(what, got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(bits(g["transform"]), bits(w["transform"])), (what, k, g, w)
        assert all(g[f] == w[f] for f in FIELDS), (what, k, g, w)
    print("%s: %d problems, transform bits, %s" % (what, len(got), ", ".join(FIELDS)))


def assert_oracle(oracle, problems, got):
    for p, g in zip(problems, got):
        w = oracle.scan2map(p)
        assert all(g[f] == w[f] for f in FIELDS), (g, w)
        assert np.abs(g["transform"] - w["transform"]).max() <= SCAN2MAP_BAR


def copy_of(p, reuse=False):
    q = defs.MapProblem(p.map_corner, p.map_surf, p.scan_corner, p.scan_surf, p.transform)
    q.reuse_resident_map = reuse
    return q


def test_scan2map_explicit_and_reuse_of_maps_of_other_sizes(pkg, ieskf, oracle):
    pair = mc.map_pair()
    x, y = pair["X"], pair["Y"]
    swapped = [y[1], y[0]]
    with make(pkg, ieskf) as fresh:
        want = fresh.scan2map_batch(y)
    with make(pkg, ieskf) as fresh:
        want_swapped = fresh.scan2map_batch(swapped)
    with make(pkg, ieskf) as warm:
        warm_x = warm.scan2map_batch(x)
        got = warm.scan2map_batch(y)
        # LINS_MAP_REUSE on every problem, but the resident maps (Y's) have other sizes at each position: re-gridded
        got_swapped = warm.scan2map_batch([copy_of(p, reuse=True) for p in swapped])
    assert all(r["iters"] > 0 for r in warm_x + got)
    assert_same_results("explicit scan-to-map after larger maps", got, want)
    assert_same_results("reuse flag on maps of other sizes than the resident ones", got_swapped, want_swapped)
    assert_oracle(oracle, y, got)
    assert_oracle(oracle, swapped, got_swapped)


def local_context(pkg, ieskf):
    case = mc.map_local_case()
    c = make(pkg, ieskf)
    c.local_map_init(mc.MAP_LOCAL["n_slots"], mc.MAP_LOCAL["window"], mc.MAP_LOCAL["max_pts"])
    for s in case["slots"]:
        for f in case["frames"][s]:
            c.local_map_push(s, *f)
    return c, case


def test_scan2map_on_the_local_map_after_explicit_problems(pkg, ieskf, oracle):
    x = mc.map_pair()["X"]
    fresh, case = local_context(pkg, ieskf)
    with fresh:
        want_build = built(fresh, fresh.local_map_build(case["slots"], case["scans"]))
        want = fresh.scan2map_batch([defs.MapProblem.local(t) for t in case["t0"]])
    warm, _ = local_context(pkg, ieskf)
    with warm:
        got_build = built(warm, warm.local_map_build(case["slots"], case["scans"]))
        warm.scan2map_batch(x)
        got = warm.scan2map_batch([defs.MapProblem.local(t) for t in case["t0"]])
    assert_same_builds("the local map both calls read", got_build, want_build)
    assert_same_results("LINS_MAP_LOCAL after explicit problems on larger maps", got, want)
    explicit = [defs.MapProblem(cl[0], cl[1], cl[2], cl[5], t) for (_, cl), t in zip(got_build, case["t0"])]
    assert_oracle(oracle, explicit, got)
    assert all(r["iters"] > 0 for r in got)


# ---- loop-closure ICP ------------------------------------------------------------------------------------------------------
def test_loop_icp(pkg, ieskf, host):
    pair = mc.icp_pair()
    x, y = pair["X"], pair["Y"]
    s, t = y[0]
    with make(pkg, ieskf) as fresh:
        want = fresh.loop_icp(y)
        want_idx, want_d = fresh.loop_icp_correspondences(s, t, np.eye(4), 100.0)
    with make(pkg, ieskf) as warm:
        warm_x = warm.loop_icp(x)
        got = warm.loop_icp(y)
        idx, d = warm.loop_icp_correspondences(s, t, np.eye(4), 100.0)
    assert all(r["status"] == 0 and r["iterations"] > 0 for r in warm_x)
    for k in range(2):
        assert icp_bits(got[k]) == icp_bits(want[k]), (k, got[k], want[k])
    assert idx.tobytes() == want_idx.tobytes() and d.tobytes() == want_d.tobytes()
    print("loop ICP after larger sources: 2 problems, every result field; %d correspondences, %d bytes of idx and sqdist" % (len(idx), idx.nbytes + d.nbytes))
    assert got[1]["status"] == -3 and got[1]["iterations"] == 0 and got[1]["n_corr"] == 0  # the refusal
    h = host.loop_icp(s, t)
    assert all(got[0][c] == h[c] for c in ICP_COUNTS) and got[0]["status"] == 0 and got[0]["converged"] == 1, (got[0], h)
    assert np.abs(got[0]["transform"] - h["transform"]).max() <= icp_cases.BAR_T and abs(got[0]["fitness"] - h["fitness"]) <= icp_cases.BAR_MSE
    hidx, hd = host.loop_icp_correspondences(s, t, np.eye(4), 100.0)
    assert np.array_equal(idx, hidx) and np.array_equal(bits(d), bits(hd))


# ---- key-pose selection ----------------------------------------------------------------------------------------------------
def keypose_fill(c, side):
    c.archive_init(1, 64, 256)
    pt, none = np.array([[0.1, 0.2, 0.3, 0.0]], F), np.zeros((0, 4), F)
    for i, (p, t) in enumerate(zip(side["poses"], side["times"])):
        assert c.archive_push(0, pt, none, none, p, time=float(t)) == i


def keypose_run(c, side):
    out = {}
    for mode in (HOST, DEVICE):
        c.keyposes_set_mode(mode)
        ids, res = c.keyposes_select_batch(side["select"])
        loops = c.keyposes_find_loop_batch(side["loop"])
        lists, res2 = c.keyposes_surround_batch(side["select"], side["lists"])
        out[mode] = dict(ids=[None if i is None else i.tolist() for i in ids], select=res, loops=loops, lists=lists, surround=res2)
    c.keyposes_set_mode(HOST)
    return out


def test_keypose_selection(pkg, ieskf, host):
    pair = mc.keypose_pair()
    x, y = pair["X"], pair["Y"]
    with make(pkg, ieskf) as fresh:
        keypose_fill(fresh, y)
        want = keypose_run(fresh, y)
    with make(pkg, ieskf) as warm:
        keypose_fill(warm, x)
        warm_x = keypose_run(warm, x)
        keypose_fill(warm, y)  # (lins_archive_init again: the archive starts over, the selection's scratch stays)
        got = keypose_run(warm, y)
    assert any(len(i) > 3 for i in warm_x[DEVICE]["ids"])
    assert got == want, (got, want)
    for mode in (HOST, DEVICE):
        g = got[mode]
        for q, (sel, lp, lst) in enumerate(zip(y["select"], y["loop"], y["lists"])):
            ds = host.select_radius(y["poses"], *sel[1:]).tolist()
            assert g["ids"][q] == ds, (mode, q)
            assert g["loops"][q] == host.find_loop(y["poses"], y["times"], *lp[1:]), (mode, q)
            assert g["lists"][q] == host.surround_update(lst, ds), (mode, q)
    print("key-pose selection after more queries on more frames: %d queries x 2 modes — ids, loop candidates, lists and result records" % len(y["select"]))
    assert any(len(i) > 0 for i in got[DEVICE]["ids"])


# ---- the front end ---------------------------------------------------------------------------------------------------------
def frontend_run(c, raws):
    segs, outl = c.segment_batch(raws, outliers=True)
    return segs, outl, c.extract_features_batch(segs)


def test_front_end(pkg, ieskf, host):
    pair = mc.frontend_pair()
    with make(pkg, ieskf) as fresh:
        want = frontend_run(fresh, pair["Y"])
    with make(pkg, ieskf) as warm:
        warm_x = frontend_run(warm, pair["X"])
        got = frontend_run(warm, pair["Y"])
    assert all(s.n > 5000 for s in warm_x[0])
    nbytes = 0
    for k, raw in enumerate(pair["Y"]):
        gs, go, gf = got[0][k], got[1][k], got[2][k]
        ws, wo, wf = want[0][k], want[1][k], want[2][k]
        assert segment_bits(gs) == segment_bits(ws), k
        assert go.shape == wo.shape and go.tobytes() == wo.tobytes(), k
        assert feature_bits(gf) == feature_bits(wf), k
        hs = host.frontend_segment(raw)
        assert segment_bits(gs) == segment_bits(hs) and go.tobytes() == host.frontend_segment_outliers(raw).tobytes(), k
        assert feature_bits(gf) == feature_bits(host.frontend_extract_segmented(hs)), k
        assert gf["n_segmented"] == gs.n and len(go) == gs.c.n_outlier > 50
        nbytes += sum(len(b) for b in segment_bits(gs)[1:5]) + go.nbytes + sum(len(b[1]) for b in feature_bits(gf)[:4])
    assert [s.n for s in got[0][:2]] == [0, 0] and got[0][2].n > 5000 and len(got[2][2]["surf_less_flat"]) > 1000
    print("front end after denser scans: %d scans — segmented scan, outlier cloud, four feature clouds and the counts, %d bytes" % (len(pair["Y"]), nbytes))


# ---- the chain -------------------------------------------------------------------------------------------------------------
STREAMS = [0, 1, 2]


def chain_pass(c, steps):
    """every store set up (again) — a re-initialised context is a fresh one — then `steps` map steps of the three streams"""
    ch.setup(c)
    sm.init(c, ch.N, ch.INTERVAL)
    out = []
    for step in range(steps):
        ch.feed(c, step)
        res = sm.step(c, STREAMS, ch.odoms(step))
        ran = sum(r["status"] != defs.MAP_STEP_SKIPPED for r in res)
        out.append(dict(res=res, clouds=[[sm.download(c, k, w) for w in range(6)] for k in range(ran)], poses=[sm.get_pose(c, s) for s in STREAMS]))
    return out


def test_the_chain_on_a_reinitialised_context(pkg, ieskf):
    assert ch.N == 3
    with ch.context(pkg, ieskf) as c:
        first = chain_pass(c, 3)
        again = chain_pass(c, 2)
    nclouds = 0
    for step, (p, q) in enumerate(zip(first, again)):
        for s in STREAMS:
            assert ch.same_result(p["res"][s], q["res"][s]), (step, s, p["res"][s], q["res"][s])
            assert ch.same_state(p["poses"][s], q["poses"][s]), (step, s, p["poses"][s], q["poses"][s])
        assert len(p["clouds"]) == len(q["clouds"])
        for k, (cp, cq) in enumerate(zip(p["clouds"], q["clouds"])):
            for w in range(6):
                assert same_cloud(cp[w], cq[w]), (step, k, w)
                nclouds += 1
    print("the chain after re-initialisation: 2 steps x 3 streams — results, pose states and %d clouds, bit for bit" % nclouds)
    assert all(r["status"] == 0 for st in first for r in st["res"]) and all(r["iters"] > 0 for r in first[1]["res"])
