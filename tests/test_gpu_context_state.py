"""A context's results never depend on what it ran before.

Real callers reuse one context for thousands of runs (the live filter, lins_streams_step, the bench's timed loop), and
three pieces of device state outlive a run: the carry records of the batch kernel (lins_ctx::d_relay_lane, four planes of
512 16-byte words per scan: ieskf_lds_lean.h), the walk cache (lins_ctx::d_walk_cache, tagged with the low 16 bits of the
launch number) and the run-history ring (lins_launch_ms_history & co.).  The tests below run a batch on a context that
ran OTHER scans in the same slots before, on contexts whose scratch state was poisoned with adversarial but in-bounds
content (positions that exist in the scan's own grid), across the walk cache's 16-bit wrap on either launch queue, and
after the history ring was filled by two-queue runs — and hold every result to a clean context's bits and, where it
applies, to the oracle.

The scratch state is read and written through lins_debug_scratch (a test aid, not part of the drop-in surface); the
launch number a context starts from is the debug knob LINS_RUN_GEN0."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import _same_bits, assert_result_close
from test_ref import widen

# carry records (ieskf_lds_lean.h): per scan [4 planes][512 query slots] of four 32-bit words
LANES = 512
SCAN_BYTES = 4 * LANES * 16
NONE16 = 0xFFFF
INF = np.float32(np.inf).view(np.uint32)


def _params(pkg, nearest=0.5):
    """Ten fixed iterations at a nearest-neighbour radius of sqrt(0.5) m (the reference's NEAREST_FEATURE_SEARCH_SQ_DIST,
    a parameter): under the default 25 m^2 the synthetic families have almost no query that finds its nearest neighbour
    only after the first iteration — the case whose walk part of the carry record is never written on the cold one."""
    prm = pkg.default_params(num_iter=10, fixed_iters=1)
    prm.nearest_sq_dist = nearest
    return prm


@pytest.fixture(scope="module")
def small(host):
    """Y: the open scene with the wide prior (queries without a nearest neighbour at iteration 0 that gain one later);
    X: other scans (the room) with other surf / corner query counts in the same slots."""
    y = widen(host.synth_batch(48, start=31000, scene=1), 31000)
    x = host.synth_batch(48, start=33000, scene=0)
    return x, y


@pytest.fixture(scope="module")
def big(host):
    """1300 scans of the same families: beyond the device's workgroup slots (several-part updates, two launch queues)."""
    return widen(host.synth_batch(1300, start=35000, scene=1), 35000)


@pytest.fixture(scope="module")
def oracle_small(pkg, oracle, small):
    prm = _params(pkg)
    return [oracle.ieskf(prm, p, oracle.FORM_DENSE, oracle.NN_KDTREE, trace=True) for p in small[1]]


def _scratch(ieskf, ctx, which, write, offset, arr):
    L = ieskf.lib()
    L.lins_debug_scratch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p]
    L.lins_debug_scratch.restype = C.c_int
    assert arr.flags.c_contiguous
    assert L.lins_debug_scratch(ctx._h, which, int(write), offset, arr.nbytes, arr.ctypes.data) == 0


def _read_carry(ieskf, ctx, n):
    out = np.zeros((n, 4, LANES, 4), np.uint32)
    _scratch(ieskf, ctx, 0, False, 0, out)
    return out


def _write_carry(ieskf, ctx, recs):
    _scratch(ieskf, ctx, 0, True, 0, np.ascontiguousarray(recs, dtype=np.uint32))


def _clean(ieskf, ctx, n):
    """Empty carry records for n scans (what lins_create leaves): a "fresh" context that does not depend on what the
    allocator handed out."""
    _write_carry(ieskf, ctx, np.full((n, 4, LANES, 4), 0xFFFFFFFF, np.uint32))


def _lo16(w):
    return (w & 0xFFFF).astype(np.int16).astype(np.int64)


def _hi16(w):
    return (w >> 16).astype(np.int16).astype(np.int64)


def _pack16(a, b):
    return ((np.asarray(a, np.int64) & 0xFFFF) | ((np.asarray(b, np.int64) & 0xFFFF) << 16)).astype(np.uint32)


def _run(ieskf, prm, batch, search, prior=None, clean=True, poison=None):
    """A context of len(batch) scans: optionally `prior` batch first (uploaded, run, downloaded), then `batch`."""
    with ieskf.IeskfContext(prm, max_batch=len(batch), max_targets=16384, search=search) as c:
        if clean:
            _clean(ieskf, c, len(batch))
        if prior is not None:
            c.upload(prior)
            c.run()
            c.sync()
            c.download()
        c.upload(batch)
        if poison is not None:
            poison(c)
        c.run()
        c.sync()
        return c.download(), _read_carry(ieskf, c, len(batch))


def _final_records(recs, batch):
    """Per scan and query slot, from the carry records a run left: the last nearest neighbour (grid position, -1 = none)
    and the query's de-skewed position it was searched at (planes 0-1)."""
    out = []
    for s, p in enumerate(batch):
        n = len(p.surf_flat) + len(p.corner_sharp)
        p0, p1 = recs[s, 0, :n], recs[s, 1, :n]
        sel = np.where(p0[:, 0] == 0xFFFFFFFF, -1, _lo16(p0[:, 1]))
        anchor = np.stack([p0[:, 3], p1[:, 0], p1[:, 1]], axis=1)
        out.append((sel, anchor))
    return out


def _other_cloud_positions(p, sel, anchor):
    """For every query slot two grid positions of the scan's OTHER target cloud (corner positions come first in the grid:
    [0, n_corner_last), surf positions [n_corner_last, n_corner_last + n_surf_last)) — the nearest neighbours of the other
    kind's queries closest to this query, so that they lie near it; -1 where the other kind has none."""
    ns, nc = len(p.surf_flat), len(p.corner_sharp)
    nct, n_all = len(p.corner_last), len(p.corner_last) + len(p.surf_last)
    xyz = anchor.view(np.float32).astype(np.float64)
    pos = np.full((ns + nc, 2), -1, np.int64)
    for lo, hi, olo, ohi in ((0, ns, ns, ns + nc), (ns, ns + nc, 0, ns)):
        cand = np.arange(olo, ohi)
        cand = cand[sel[cand] >= 0]
        if hi == lo or cand.size == 0:
            continue
        d = ((xyz[lo:hi, None, :] - xyz[None, cand, :]) ** 2).sum(axis=2)
        order = np.argsort(d, axis=1, kind="stable")[:, :2]
        pos[lo:hi, : order.shape[1]] = sel[cand][order]
    # (in the other cloud's position range of this scan's grid, by construction)
    surf = (np.arange(ns + nc) < ns)[:, None]
    lo, hi = np.where(surf, 0, nct), np.where(surf, nct, n_all)
    assert n_all <= 12288 and ((pos == -1) | ((pos >= lo) & (pos < hi))).all()
    if pos.shape[0] and (pos[:, 1] < 0).all():
        pos[:, 1] = pos[:, 0]
    return pos


# ---- A: the input reaches the case (oracle only) -----------------------------------------------------------------------
def test_the_batch_has_queries_that_find_their_nearest_neighbour_only_after_the_first_iteration(pkg, oracle_small, small):
    """The precondition the history tests rest on, from the oracle's trace: queries with no nearest neighbour at iteration 0
    (ind1 == -1) that gain one at a later iteration — a few dozen of each kind across the batch — in scans whose queries
    all have carry records (at most 512)."""
    _, y = small
    n = {"surf": 0, "corner": 0}
    for (res, tr), p in zip(oracle_small, y):
        assert len(p.surf_flat) + len(p.corner_sharp) <= LANES
        for kind in n:
            i1 = tr[kind]["ind1"][: res.iters]
            n[kind] += int(((i1[0] < 0) & (i1[1:] >= 0).any(axis=0)).sum())
    assert n["surf"] >= 24 and n["corner"] >= 24, n
    x, _ = small
    assert sum((len(a.surf_flat), len(a.corner_sharp)) != (len(b.surf_flat), len(b.corner_sharp)) for a, b in zip(x, y)) >= 40


# ---- B: natural history --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("search", ["mr", "lds", "lds1", "auto"])
def test_a_batch_after_other_scans_in_the_same_slots_returns_a_fresh_contexts_bits(pkg, ieskf, small, oracle_small, search):
    prm = _params(pkg)
    x, y = small
    fresh, _ = _run(ieskf, prm, y, search)
    got, _ = _run(ieskf, prm, y, search, prior=x, clean=False)
    for k, (a, b, (want, _)) in enumerate(zip(got, fresh, oracle_small)):
        _same_bits(a, b)
        assert_result_close(b, want)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["relay", "two_queues"])
def test_large_batch_forms_after_other_scans_return_a_fresh_contexts_bits(pkg, ieskf, big, monkeypatch, form):
    """Several-part updates (LINS_RELAY_AT) and two launch queues (LINS_SPLIT_STREAMS=2) on 600 scans after 600 others."""
    prm = _params(pkg)
    y, x = big[:600], big[650:1250]
    monkeypatch.setenv("LINS_ENABLE_DEBUG_KNOBS", "1")
    monkeypatch.setenv("LINS_RELAY_AT" if form == "relay" else "LINS_SPLIT_STREAMS", "4" if form == "relay" else "2")
    fresh, _ = _run(ieskf, prm, y, "mr")
    got, _ = _run(ieskf, prm, y, "mr", prior=x, clean=False)
    for a, b in zip(got, fresh):
        _same_bits(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("search", ["mr", "lds1"])
def test_single_scan_update_after_another_scan_returns_a_fresh_contexts_bits(pkg, ieskf, small, oracle_small, search):
    """lins_ieskf_update, the live filter's call: one context, scan after scan."""
    prm = _params(pkg)
    x, y = small
    with ieskf.IeskfContext(prm, max_batch=1, max_targets=16384, search=search) as c:
        for k in range(12):
            c.update(x[k])
            got = c.update(y[k])
            with ieskf.IeskfContext(prm, max_batch=1, max_targets=16384, search=search) as f:
                _clean(ieskf, f, 1)
                _same_bits(got, f.update(y[k]))
            assert_result_close(got, oracle_small[k][0])


# ---- C: poisoned carry records -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("search", ["mr", "lds1"])
def test_poisoned_walk_parts_of_the_carry_records_change_no_bit(pkg, ieskf, small, oracle_small, search):
    """Planes 2-3 (second / third point) of every query slot written, before the run, with positions of the scan's other
    target cloud, with positions of the same cloud in the wrong ring class, each with a +inf certificate bound and an anchor
    at the query's own position.  Every poisoned position exists in that scan's grid: an unfixed kernel reads wrong data,
    never memory outside its allocations."""
    prm = _params(pkg)
    _, y = small
    clean, recs = _run(ieskf, prm, y, search)
    final = _final_records(recs, y)
    variants = {"other_cloud": np.full((len(y), 4, LANES, 4), 0xFFFFFFFF, np.uint32)}
    variants["wrong_class"] = variants["other_cloud"].copy()
    n_poisoned = 0
    for s, p in enumerate(y):
        sel, anchor = final[s]
        n, ns = len(sel), len(p.surf_flat)
        if n == 0:
            continue
        oc = _other_cloud_positions(p, sel, anchor)
        v = variants["other_cloud"][s]
        v[2, :n] = np.stack([_pack16(oc[:, 0], oc[:, 1]), _pack16(oc[:, 1], oc[:, 0]), np.full(n, INF), np.full(n, INF)], axis=1)
        v[3, :n, :3] = anchor
        # same cloud, wrong ring class: a plane's second point on another ring (its clean third point), its third point on
        # the nearest neighbour's ring (its clean second point); a line's second point on the nearest neighbour's own ring
        w2 = recs[s, 2, :n]
        a2, b2, a3, b3 = _lo16(w2[:, 0]), _hi16(w2[:, 0]), _lo16(w2[:, 1]), _hi16(w2[:, 1])
        p0 = recs[s, 0, :n]
        a1, b1 = _lo16(p0[:, 0]), _hi16(p0[:, 0])
        ra, rb = (p0[:, 1] >> 16) & 0xFF, p0[:, 1] >> 24
        line_wrong = np.where((b1 >= 0) & (ra == rb), b1, a1)
        surf = np.arange(n) < ns
        wc = variants["wrong_class"][s]
        wc[2, :n, 0] = np.where(surf, _pack16(a3, b3), _pack16(line_wrong, a1))
        wc[2, :n, 1] = np.where(surf, _pack16(a2, b2), _pack16(line_wrong, a1))
        wc[2, :n, 2:] = INF
        wc[3, :n, :3] = anchor
        n_poisoned += n
    assert n_poisoned > 5000
    for name, recs_p in variants.items():
        got, _ = _run(ieskf, prm, y, search, poison=lambda c: _write_carry(ieskf, c, recs_p))
        for k, (a, b, (want, _)) in enumerate(zip(got, clean, oracle_small)):
            _same_bits(a, b)
            assert_result_close(a, want)


# ---- D: device-resident streams ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("search", ["mr", "lds1"])
def test_streams_steps_equal_their_history_free_twins(pkg, ieskf, host, search):
    """Eight lins_streams_step_raw steps of one sequence on one context (every step's scan sits in the slot of the scan before,
    with other query counts).  Step k >= 2 is replayed on a fresh context that has only seen scan k - 1, bootstrapped with the
    long run's posterior of step k - 1 (the pose its clouds were re-projected with): same prior, same covariance, same bits."""
    prm = pkg.default_params(num_iter=30)
    raws = [host.synth_seq_raw_scan(11, k) for k in range(1, 9)]
    state = np.zeros(19)
    state[6] = 1.0
    cov = np.eye(18) * 1e-4
    priors, posts = [], []
    with ieskf.IeskfContext(prm, max_batch=1, max_targets=16 * 1800, search=search) as c:
        _clean(ieskf, c, 1)
        c.streams_init(1)
        for raw in raws:
            priors.append((state.copy(), cov.copy()))
            (r,), _ = c.streams_step_raw([raw], state[None], cov[None])
            posts.append(r)
            state, cov = np.array(r.state), np.array(r.cov).reshape(18, 18) + np.eye(18) * 1e-4  # (constant velocity)
    assert all(r.iters > 0 for r in posts[1:])
    for k in range(2, len(raws)):
        with ieskf.IeskfContext(prm, max_batch=1, max_targets=16 * 1800, search=search) as f:
            _clean(ieskf, f, 1)
            f.streams_init(1)
            f.streams_step_raw([raws[k - 1]], np.array(posts[k - 1].state)[None], priors[k - 1][1][None])
            (r,), _ = f.streams_step_raw([raws[k]], priors[k][0][None], priors[k][1][None])
        _same_bits(r, posts[k])


# ---- E: the walk cache's 16-bit wrap -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wrap_on", ["stream2", "stream"])
def test_runs_across_the_walk_cache_wrap_return_the_one_launch_bits(pkg, ieskf, big, monkeypatch, wrap_on):
    """1300 scans, LINS_SPLIT_STREAMS=2: three launches per run, on the context's stream, the second queue, the context's
    stream.  The context starts at a launch number (LINS_RUN_GEN0) that puts the wrap of the cache's 16-bit tags on the
    second launch (second queue) or the third (context's stream), and its cache holds, for every query, an entry tagged
    (0 << 16) | its final nearest neighbour: other-cloud positions, a +inf bound, an anchor at the query's own recorded
    position — what an entry of a launch 65 536 launches earlier could hold.  The run must not see any of it."""
    prm = _params(pkg)
    batch = big
    monkeypatch.setenv("LINS_ENABLE_DEBUG_KNOBS", "1")
    monkeypatch.setenv("LINS_SPLIT_STREAMS", "0")
    want, recs = _run(ieskf, prm, batch, "mr")
    final = _final_records(recs, batch)
    entries = []
    for s, p in enumerate(batch):
        sel, anchor = final[s]
        n = len(sel)
        e = np.full((n, 8), 0xFFFFFFFF, np.uint32)
        if n:
            oc = _other_cloud_positions(p, sel, anchor)
            has = sel >= 0
            e[has, 0] = (sel[has] & 0xFFFF).astype(np.uint32)  # (tag: generation 0 in the high half)
            e[has, 1] = _pack16(oc[has, 0], oc[has, 1])
            e[has, 2] = _pack16(oc[has, 1], oc[has, 0])
            e[has, 3] = e[has, 4] = INF
            e[has, 5:8] = anchor[has]
        entries.append(e)
    cache = np.ascontiguousarray(np.concatenate(entries))  # (query slots of the batch, in upload order)
    assert (cache[:, 0] != 0xFFFFFFFF).sum() > 100000
    monkeypatch.setenv("LINS_SPLIT_STREAMS", "2")
    monkeypatch.setenv("LINS_RUN_GEN0", str(65534 if wrap_on == "stream2" else 65533))
    with ieskf.IeskfContext(prm, max_batch=len(batch), max_targets=16384, search="mr") as c:
        _clean(ieskf, c, len(batch))
        c.upload(batch)
        _scratch(ieskf, c, 1, True, 0, cache)
        c.run()
        got = c.download()
        assert all(b > 0.0 for _, b in c.launch_ms_history(1))  # (the run went out on both queues)
        c.run()  # (and the run after the wrap)
        again = c.download()
    for a, b, w in zip(got, again, want):
        _same_bits(a, w)
        _same_bits(b, w)


# ---- F: the run-history ring ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_chunked_update_after_two_queue_runs_reports_one_launch(pkg, ieskf, big, monkeypatch):
    """Every slot of the 64-run history ring set by two-queue runs, then lins_ieskf_update_batch on >= 2 chunks (its
    pipelined path records the history itself): one launch is reported, the times are its own, and a following run of the
    resident batch returns that batch's bits."""
    prm = _params(pkg)
    monkeypatch.setenv("LINS_ENABLE_DEBUG_KNOBS", "1")
    monkeypatch.setenv("LINS_SPLIT_STREAMS", "2")
    monkeypatch.setenv("LINS_BATCH_CHUNK", "64")
    runs, small = big[:600], big[600:760]
    with ieskf.IeskfContext(prm, max_batch=len(runs), max_targets=16384, search="mr") as c:
        c.upload(runs)
        for _ in range(65):
            c.run()
        c.sync()
        assert all(b > 0.0 for _, b in c.launch_ms_history(64))
        res = c.update_batch(small)
        (first, second), = c.launch_ms_history(1)
        assert first > 0.0 and second == 0.0, (first, second)
        for v in (c.kernel_ms_history(1)[0], c.runs_span_ms(1)):
            assert np.isfinite(v) and v > 0.0
        c.run()
        c.sync()
        for a, b in zip(c.download(len(small)), res):
            _same_bits(a, b)
