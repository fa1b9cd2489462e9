"""Rendezvous (include/lins_team.h): the team search over the frames of many slots — the device calls on an
ieskf.IeskfContext, and their definition on the CPU (include/lins_host.h lins_host_place_team_topk) — and the team map
(include/lins_map.h lins_keyposes_team_select_batch; lins_host_team_select / _team_map): which key frames of a team of
slots a merged local map takes.  Rendezvous over a window: consensus_batch / rendezvous_window_step (the rule's definition on the
CPU is host.rendezvous_consensus).

A query is (query_slot, query_id, now, min_gap_s); a rank is a dict(slot, id, shift, distance (np.float32), dk,
candidates, status).  There is no fall-back: the device calls need liblins_ieskf.so and a GPU."""
import ctypes as C

import numpy as np

from . import host as _host
from . import ieskf as _ieskf
from ._ctypes_defs import (PLACE_RINGS, LoopStepParamsC, PlaceTeamParamsC, PlaceTeamQueryC, PlaceTeamResultC, RendezvousEntryC, RendezvousParamsC,
                           RendezvousResultC, loop_step_params, place_team_params, rendezvous_params)


def params(lib=None, **kw):
    """lins_place_team_default_params (shortlist 32, k 4, min_sep 0) overridden by keyword"""
    return place_team_params(lib if lib is not None else _host.lib(), **kw)


def _raw(out, k, filled):
    return [out[j].as_dict() for j in range(k)], int(filled)


def topk(ctx, queries, target_slots, raw=False, **kw):
    """lins_place_team_topk_batch on context `ctx`: per query the list of its filled ranks' dicts, or the C return code (a
    negative int) of a refused call.  raw: per query (all k records, ranks filled).  kw: shortlist=, k=, min_sep=."""
    L = _ieskf.lib()
    prm = place_team_params(L, **kw)
    n, k = len(queries), max(int(prm.k), 1)
    arr = (PlaceTeamQueryC * max(n, 1))(*[PlaceTeamQueryC(int(s), int(i), float(now), float(gap)) for s, i, now, gap in queries])
    slots = np.ascontiguousarray(target_slots, np.int32)
    out = (PlaceTeamResultC * max(n * k, 1))()
    counts = np.zeros(max(n, 1), np.int32)
    L.lins_place_team_topk_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(PlaceTeamQueryC), C.c_int, C.c_void_p, C.POINTER(PlaceTeamParamsC),
                                             C.POINTER(PlaceTeamResultC), C.c_void_p]
    rc = L.lins_place_team_topk_batch(ctx._h, n, arr, len(slots), slots.ctypes.data if len(slots) else None, C.byref(prm), out, counts.ctypes.data)
    if rc != 0:
        return rc
    res = [_raw(out[e * k:(e + 1) * k], k, counts[e]) for e in range(n)]
    return res if raw else [r[:f] for r, f in res]


def key(ctx, slot, id):
    """lins_place_team_key -> (occ (20,) uint8, sumsq, time) of one frame as the device holds it"""
    L = _ieskf.lib()
    occ, sq, t = np.zeros(PLACE_RINGS, np.uint8), C.c_uint32(0), C.c_double(0)
    L.lins_place_team_key.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    ctx._check(L.lins_place_team_key(ctx._h, int(slot), int(id), occ.ctypes.data, C.byref(sq), C.byref(t)))
    return occ, int(sq.value), float(t.value)


def set_chunk(ctx, chunk):
    """lins_place_team_set_chunk (test hook): candidates per workgroup of the shortlist; 0 = default"""
    L = _ieskf.lib()
    L.lins_place_team_set_chunk.argtypes = [C.c_void_p, C.c_int]
    return L.lins_place_team_set_chunk(ctx._h, int(chunk))


def stats(ctx):
    """dict(key_ms, shortlist_ms, pair_ms, frames_keyed, scanned) of the last team search"""
    L = _ieskf.lib()
    a, b, c, f, s = C.c_float(0), C.c_float(0), C.c_float(0), C.c_int32(0), C.c_uint64(0)
    L.lins_last_place_team_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_uint64)]
    ctx._check(L.lins_last_place_team_stats(ctx._h, C.byref(a), C.byref(b), C.byref(c), C.byref(f), C.byref(s)))
    return dict(key_ms=a.value, shortlist_ms=b.value, pair_ms=c.value, frames_keyed=int(f.value), scanned=int(s.value))


def rendezvous_step(ctx, entries, target_slots, params=None, **kw):
    """lins_rendezvous_step: entries [(slot, now)] against the frames of target_slots.  params: a LoopStepParamsC (default:
    lins_loop_step_default_params); kw: shortlist=, k=, min_sep=, max_distance=.  Returns the per-entry result dicts (outcome,
    status, latest_id, n_candidates, chosen, target_slot, target_id, latest, cand, target, icp, X (4 x 4 f64)), or the C
    return code (a negative int) of a refused call."""
    L = _ieskf.lib()
    prm = params if params is not None else loop_step_params(L)
    tp = rendezvous_params(L, **kw)
    n = len(entries)
    arr = (RendezvousEntryC * max(n, 1))(*[RendezvousEntryC(int(s), 0, float(now)) for s, now in entries])
    slots = np.ascontiguousarray(target_slots, np.int32)
    out = (RendezvousResultC * max(n, 1))()
    L.lins_rendezvous_step.argtypes = [C.c_void_p, C.c_int, C.POINTER(RendezvousEntryC), C.c_int, C.c_void_p, C.POINTER(LoopStepParamsC),
                                       C.POINTER(RendezvousParamsC), C.POINTER(RendezvousResultC)]
    rc = L.lins_rendezvous_step(ctx._h, n, arr, len(slots), slots.ctypes.data if len(slots) else None, C.byref(prm), C.byref(tp), out)
    return [out[k].as_dict() for k in range(n)] if rc == 0 else rc


def consensus_batch(ctx, tables, offsets=None, **kw):
    """lins_rendezvous_consensus_batch: one launch over `tables`, each a list of hypothesis dicts (X, p, fitness, query, rank,
    target_slot, admissible: host.rendezvous_consensus's).  offsets: the n + 1 offsets to pass instead of the tables' own
    (for the refusals); kw: fields of lins_consensus_params.  Returns per table dict(winner, support, n_admissible, members),
    or the C return code (a negative int) of a refused call."""
    from ._ctypes_defs import ConsensusHypC, ConsensusParamsC, ConsensusResultC, consensus_params, consensus_table

    L = _ieskf.lib()
    n = len(tables)
    arr = consensus_table([h for t in tables for h in t])
    off = np.ascontiguousarray(np.cumsum([0] + [len(t) for t in tables]) if offsets is None else offsets, np.int32)
    prm, out = consensus_params(L, **kw), (ConsensusResultC * max(n, 1))()
    L.lins_rendezvous_consensus_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(ConsensusHypC), C.c_void_p, C.POINTER(ConsensusParamsC),
                                                  C.POINTER(ConsensusResultC)]
    rc = L.lins_rendezvous_consensus_batch(ctx._h, n, arr, off.ctypes.data, C.byref(prm), out)
    return [out[e].as_dict() for e in range(n)] if rc == 0 else rc


def consensus_stats(ctx):
    """HIP-event ms of the last consensus launch"""
    L = _ieskf.lib()
    ms = C.c_float(0)
    L.lins_last_rendezvous_consensus_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    ctx._check(L.lins_last_rendezvous_consensus_stats(ctx._h, C.byref(ms)))
    return ms.value


def rendezvous_window_step(ctx, entries, target_slots, params=None, consensus=None, **kw):
    """lins_rendezvous_window_step: entries [(slot, now)] against the frames of target_slots; the last `window` frames of every
    entry ask, and a merge is FOUND only where min_support of them agree.  params: a LoopStepParamsC (default:
    lins_loop_step_default_params); consensus: a dict of lins_consensus_params fields (window=, stride=, min_support=,
    max_translation=, min_cos_rotation=) over the defaults; kw: shortlist=, k=, min_sep=, max_distance=.  Returns the per-entry
    result dicts (outcome, status, n_queries, n_hypotheses, winner, support, n_admissible, target_slot, target_id, members,
    query_id, n_ranks, source, X (4 x 4 f64), hyp: the entry's hypotheses as dicts query, rank, admissible, member, cand,
    target, icp), or the C return code (a negative int) of a refused call."""
    from ._ctypes_defs import ConsensusParamsC, RendezvousHypothesisC, RendezvousWindowResultC, consensus_params

    L = _ieskf.lib()
    prm = params if params is not None else loop_step_params(L)
    tp = rendezvous_params(L, **kw)
    cp = consensus_params(L, **(consensus or {}))
    n = len(entries)
    per = max(int(cp.window), 1) * max(int(tp.team.k), 1)
    arr = (RendezvousEntryC * max(n, 1))(*[RendezvousEntryC(int(s), 0, float(now)) for s, now in entries])
    slots = np.ascontiguousarray(target_slots, np.int32)
    out = (RendezvousWindowResultC * max(n, 1))()
    hyp = (RendezvousHypothesisC * max(n * per, 1))()
    L.lins_rendezvous_window_step.argtypes = [C.c_void_p, C.c_int, C.POINTER(RendezvousEntryC), C.c_int, C.c_void_p, C.POINTER(LoopStepParamsC),
                                              C.POINTER(RendezvousParamsC), C.POINTER(ConsensusParamsC), C.POINTER(RendezvousWindowResultC),
                                              C.POINTER(RendezvousHypothesisC)]
    rc = L.lins_rendezvous_window_step(ctx._h, n, arr, len(slots), slots.ctypes.data if len(slots) else None, C.byref(prm), C.byref(tp),
                                       C.byref(cp), out, hyp)
    if rc != 0:
        return rc
    res = []
    for e in range(n):
        r = out[e].as_dict()
        r["hyp"] = [hyp[e * per + x].as_dict() for x in range(r["n_hypotheses"])]
        res.append(r)
    return res


def rendezvous_window_stats(ctx):
    """dict(detect_ms, assemble_ms, align_ms, consensus_ms, total_ms) of the last window step (host clock)"""
    L = _ieskf.lib()
    v = [C.c_float(0) for _ in range(5)]
    L.lins_last_rendezvous_window_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_float)] * 5
    ctx._check(L.lins_last_rendezvous_window_stats(ctx._h, *[C.byref(x) for x in v]))
    return dict(zip(("detect_ms", "assemble_ms", "align_ms", "consensus_ms", "total_ms"), [x.value for x in v]))


def _xs(X, n):
    return np.ascontiguousarray(X, np.float64).reshape(n, 16)


def pose_graph_rebase(ctx, slots, X):
    """lins_pose_graph_rebase_batch: the graphs of `slots` move into the frames X (one 4 x 4 f64 per slot, in the archive's
    axes, as rendezvous_step's X) -> the C return code"""
    L = _ieskf.lib()
    s = np.ascontiguousarray(slots, np.int32)
    x = _xs(X, len(s)) if len(s) else np.zeros((1, 16))
    L.lins_pose_graph_rebase_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return L.lins_pose_graph_rebase_batch(ctx._h, len(s), s.ctypes.data if len(s) else None, x.ctypes.data if len(s) else None)


def rebase(ctx, slots, X, streams=None):
    """lins_team_rebase: pose_graph_rebase, then the archive, the ring and the map poses of `streams` (default: none, -1)
    follow -> the C return code"""
    L = _ieskf.lib()
    s = np.ascontiguousarray(slots, np.int32)
    t = np.ascontiguousarray(streams if streams is not None else [-1] * len(s), np.int32)
    assert len(t) == len(s)
    x = _xs(X, len(s)) if len(s) else np.zeros((1, 16))
    L.lins_team_rebase.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L.lins_team_rebase(ctx._h, len(s), s.ctypes.data if len(s) else None, t.ctypes.data if len(s) else None, x.ctypes.data if len(s) else None)


# ---- the team graph ----
def factor_from_alignment(ctx, slot_b, id_b, slot_a, id_a, X=None, fitness=1.0):
    """lins_team_factor_from_alignment: the team factor Z = (X T_b)^-1 T_a of the two graphs' estimates as they stand (X: 4 x 4
    f64 in the archive's axes, None: the identity) -> a TeamFactorC, or the C return code of a refused call"""
    from ._ctypes_defs import TeamFactorC

    L, out = _ieskf.lib(), TeamFactorC()
    x = None if X is None else np.ascontiguousarray(X, np.float64).reshape(16)
    L.lins_team_factor_from_alignment.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.POINTER(TeamFactorC)]
    rc = L.lins_team_factor_from_alignment(ctx._h, int(slot_b), int(id_b), int(slot_a), int(id_a), x.ctypes.data if x is not None else None,
                                           float(fitness), C.byref(out))
    return rc if rc else out


def graph_solve(ctx, groups, params=None, root_variance=None):
    """lins_team_graph_solve.  groups: tuples (slots, factors) — slots[0] is the anchor; factors: TeamFactorC records, dicts or
    tuples (slot_b, id_b, slot_a, id_a, Z, var).  root_variance: six variances (rotation first) for every non-anchor member,
    or a dict slot -> six variances; default the odometry factor's (1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6).  Returns the
    per-group result dicts, or the C return code of a refused call."""
    from ._ctypes_defs import PoseGraphParamsC, TeamFactorC, TeamGraphResultC, TeamMemberC, pose_graph_params, team_factor

    L = _ieskf.lib()
    prm = params if params is not None else pose_graph_params(L)
    default = (1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6)
    mem, fac, moff, foff = [], [], [0], [0]
    for slots, factors in groups:
        for s in slots:
            v = root_variance.get(int(s), default) if isinstance(root_variance, dict) else (root_variance if root_variance is not None else default)
            m = TeamMemberC(int(s), 0)
            m.root_variance[:] = [float(x) for x in v]
            mem.append(m)
        fac += [team_factor(f) for f in factors]
        moff.append(len(mem)), foff.append(len(fac))
    n = len(groups)
    marr, farr = (TeamMemberC * max(len(mem), 1))(*mem), (TeamFactorC * max(len(fac), 1))(*fac)
    mo, fo = np.ascontiguousarray(moff, np.int32), np.ascontiguousarray(foff, np.int32)
    out = (TeamGraphResultC * max(n, 1))()
    L.lins_team_graph_solve.argtypes = [C.c_void_p, C.c_int, C.POINTER(TeamMemberC), C.c_void_p, C.POINTER(TeamFactorC), C.c_void_p,
                                        C.POINTER(PoseGraphParamsC), C.POINTER(TeamGraphResultC)]
    rc = L.lins_team_graph_solve(ctx._h, n, marr, mo.ctypes.data, farr, fo.ctypes.data, C.byref(prm), out)
    return rc if rc else [out[k].as_dict() for k in range(n)]


def graph_stats(ctx):
    """(HIP-event ms of the last graph_solve, trials it ran over all groups)"""
    L, ms, it = _ieskf.lib(), C.c_float(0), C.c_uint64(0)
    L.lins_last_team_graph_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    ctx._check(L.lins_last_team_graph_stats(ctx._h, C.byref(ms), C.byref(it)))
    return float(ms.value), int(it.value)


# ---- pairwise-consistent team factors ----
def factors_consistent(ctx, groups, member_offsets=None, factor_offsets=None, out=None, **kw):
    """lins_team_factors_consistent_batch.  groups: tuples (slots, factors) as graph_solve's; kw: fields of
    lins_team_pcm_params over the defaults (max_translation=, min_cos_rotation=, translation_per_frame=, min_support=,
    max_nodes=).  member_offsets / factor_offsets: the n + 1 offsets to pass instead of the groups' own, out: a
    TeamPcmResultC array to write into (for the refusals).  Returns per group dict(n_factors, n_kept, n_pairs, n_pairs_kept,
    exact, nodes_max, kept: the indices of the kept factors inside the group), or the C return code of a refused call."""
    from ._ctypes_defs import TeamFactorC, TeamMemberC, TeamPcmParamsC, TeamPcmResultC, team_factor, team_pcm_params

    L = _ieskf.lib()
    mem, fac, moff, foff = [], [], [0], [0]
    for slots, factors in groups:
        mem += [TeamMemberC(int(s), 0) for s in slots]
        fac += [team_factor(f) for f in factors]
        moff.append(len(mem)), foff.append(len(fac))
    n = len(groups)
    marr, farr = (TeamMemberC * max(len(mem), 1))(*mem), (TeamFactorC * max(len(fac), 1))(*fac)
    mo = np.ascontiguousarray(moff if member_offsets is None else member_offsets, np.int32)
    fo = np.ascontiguousarray(foff if factor_offsets is None else factor_offsets, np.int32)
    prm = team_pcm_params(L, **kw)
    res = out if out is not None else (TeamPcmResultC * max(n, 1))()
    L.lins_team_factors_consistent_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(TeamMemberC), C.c_void_p, C.POINTER(TeamFactorC), C.c_void_p,
                                                     C.POINTER(TeamPcmParamsC), C.POINTER(TeamPcmResultC)]
    rc = L.lins_team_factors_consistent_batch(ctx._h, n, marr, mo.ctypes.data, farr, fo.ctypes.data, C.byref(prm), res)
    return rc if rc else [res[k].as_dict() for k in range(n)]


def keep_factors(factors, factor_offsets, results):
    """the factors that factors_consistent kept, compacted in the caller's order: (factors, factor_offsets) ready for
    lins_team_graph_solve.  factors: the call's factors back to back; factor_offsets: its n + 1 offsets; results: its
    per-group dicts (or TeamPcmResultC records)."""
    kept, off = [], [0]
    for g, r in enumerate(results):
        idx = r["kept"] if isinstance(r, dict) else r.as_dict()["kept"]
        first, count = int(factor_offsets[g]), int(factor_offsets[g + 1]) - int(factor_offsets[g])
        assert all(0 <= i < count for i in idx)
        kept += [factors[first + i] for i in sorted(idx)]
        off.append(len(kept))
    return kept, np.ascontiguousarray(off, np.int32)


def pcm_stats(ctx):
    """HIP-event ms of the last factors_consistent launch"""
    L, ms = _ieskf.lib(), C.c_float(0)
    L.lins_last_team_pcm_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    ctx._check(L.lins_last_team_pcm_stats(ctx._h, C.byref(ms)))
    return ms.value


def debug_pcm_clique(ctx, adj, pair=None, out=None, **kw):
    """lins_debug_team_pcm_clique: the device's search stage alone on given rows, the twin of host.team_pcm_clique"""
    from ._ctypes_defs import TeamPcmParamsC, TeamPcmResultC, team_pcm_params

    L = _ieskf.lib()
    rows = np.ascontiguousarray(adj, np.uint64)
    n = len(rows)
    keys = np.ascontiguousarray(pair if pair is not None else np.zeros(n), np.int32)
    assert len(keys) == n
    prm = team_pcm_params(L, **kw)
    res = out if out is not None else TeamPcmResultC()
    L.lins_debug_team_pcm_clique.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(TeamPcmParamsC), C.POINTER(TeamPcmResultC)]
    L.lins_debug_team_pcm_clique.restype = C.c_int
    rc = L.lins_debug_team_pcm_clique(ctx._h, n, rows.ctypes.data if n else None, keys.ctypes.data if n else None, C.byref(prm), C.byref(res))
    return rc if rc else res.as_dict()


# ---- the team map ----
def select(ctx, queries, stride=None):
    """lins_keyposes_team_select_batch.  queries: tuples (centre, radius, pose_leaf, target slots); stride: pairs an entry
    may return (default: the frames of the largest team).  Returns (pairs, results): per entry its (slot, id) pairs as an
    (n, 2) int32 array (None with a status) and dict(n, hits, status, host) — or the C return code of a refused call."""
    from ._ctypes_defs import KeyposesResultC, KeyposesTeamQueryC, keyposes_team_query

    L = _ieskf.lib()
    n = len(queries)
    table, arr = [], (KeyposesTeamQueryC * max(n, 1))()
    for k, (centre, radius, leaf, slots) in enumerate(queries):
        arr[k] = keyposes_team_query(centre, radius, leaf, len(slots), len(table))
        table += [int(s) for s in slots]
    if stride is None:
        L.lins_archive_count.argtypes = [C.c_void_p, C.c_int]
        stride = max([sum(max(L.lins_archive_count(ctx._h, int(s)), 0) for s in set(q[3])) for q in queries] + [1])
    tab = np.ascontiguousarray(table, np.int32)
    pairs = np.full((max(n, 1), max(int(stride), 1), 2), -1, np.int32)
    out = (KeyposesResultC * max(n, 1))()
    L.lins_keyposes_team_select_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(KeyposesTeamQueryC), C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                  C.POINTER(KeyposesResultC)]
    rc = L.lins_keyposes_team_select_batch(ctx._h, n, arr, tab.ctypes.data if len(tab) else None, len(tab), pairs.ctypes.data, int(stride), out)
    if rc != 0:
        return rc
    res = [out[k].as_dict() for k in range(n)]
    return [None if r["status"] else pairs[k, :r["n"]].copy() for k, r in enumerate(res)], res


def select_stats(ctx):
    """dict(device_ms, host_entries, hits) of the last team selection"""
    L = _ieskf.lib()
    ms, hst, hits = C.c_float(0), C.c_int32(0), C.c_uint64(0)
    L.lins_last_keyposes_team_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
    ctx._check(L.lins_last_keyposes_team_stats(ctx._h, C.byref(ms), C.byref(hst), C.byref(hits)))
    return dict(device_ms=ms.value, host_entries=hst.value, hits=hits.value)


def host_select(targets, centre, radius, pose_leaf, cap=None):
    """lins_host_team_select.  targets: [(slot, key poses (n, 6))] -> the (slot, id) pairs as an (n, 2) int32 array, or the C
    return code (a negative int) of a refusal.  cap: the room of the caller's array (default: every candidate)."""
    from ._ctypes_defs import KeyPoseC

    L = _host.lib()
    n = len(targets)
    slots, cnt = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    pp, keep = (C.c_void_p * max(n, 1))(), []
    for t, (slot, poses) in enumerate(targets):
        kp = _host._key_poses(poses)
        keep.append(kp)
        slots[t], cnt[t], pp[t] = slot, len(poses), C.addressof(kp)
    cap = int(cnt[:n].sum()) if cap is None else int(cap)
    pairs = np.full((max(cap, 1), 2), -1, np.int32)
    c = (C.c_float * 3)(*[float(v) for v in centre])
    L.lins_host_team_select.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_void_p, C.c_int]
    L.lins_host_team_select.restype = C.c_int
    rc = L.lins_host_team_select(n, slots.ctypes.data, pp, cnt.ctypes.data, c, float(radius), float(pose_leaf), pairs.ctypes.data, cap)
    return pairs[:rc].copy() if rc >= 0 else rc


def host_map(frames, pairs, scan):
    """lins_host_team_map: the CPU restatement of the team build for one entry.  frames: per slot [(corner, surf, outlier,
    pose)] by frame id; pairs: the listed (slot, id); scan: (corner, surf, outlier) raw.  Returns (the six clouds in LOCAL_*
    order, sizes dict), or the C return code of a refusal."""
    from ._ctypes_defs import KeyframeC, LocalMapSizesC, Point, keyframe_c, local_scan_c

    L = _host.lib()
    ns = len(frames)
    arrs, keep = [], []
    fp, cnt = (C.c_void_p * max(ns, 1))(), np.zeros(max(ns, 1), np.int32)
    for s, fs in enumerate(frames):
        fr = (KeyframeC * max(len(fs), 1))()
        for k, f in enumerate(fs):
            fr[k], kk = keyframe_c(*f)
            keep.append(kk)
        arrs.append(fr)
        fp[s], cnt[s] = C.addressof(fr), len(fs)
    sc, skeep = local_scan_c(*scan)
    pv = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    used = [frames[s][i] for s, i in pv if 0 <= s < ns and 0 <= i < len(frames[s])]
    caps = [sum(len(f[0]) for f in used), sum(len(f[1]) + len(f[2]) for f in used), len(skeep[0]), len(skeep[1]), len(skeep[2]),
            len(skeep[1]) + len(skeep[2])]
    outs = [np.zeros((max(c, 1), 4), np.float32) for c in caps]
    ptrs = (C.POINTER(Point) * 6)(*[o.ctypes.data_as(C.POINTER(Point)) for o in outs])
    sizes = LocalMapSizesC()
    L.lins_host_team_map.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(type(sc)), C.POINTER(C.POINTER(Point)),
                                     C.POINTER(LocalMapSizesC)]
    L.lins_host_team_map.restype = C.c_int
    rc = L.lins_host_team_map(ns, fp, cnt.ctypes.data, pv.ctypes.data, len(pv), C.byref(sc), ptrs, C.byref(sizes))
    if rc != 0:
        return rc
    d = sizes.as_dict()
    return [o[:n].copy() for o, n in zip(outs, d["n"])], d


# ---- the definition on the CPU ----
def host_ring_key(desc):
    """lins_host_place_ring_key -> (occ (20,) uint8, sumsq)"""
    L = _host.lib()
    d = np.ascontiguousarray(desc, np.float32).reshape(1200)
    occ, sq = np.zeros(PLACE_RINGS, np.uint8), C.c_uint32(0)
    L.lins_host_place_ring_key.argtypes, L.lins_host_place_ring_key.restype = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)], C.c_int
    rc = L.lins_host_place_ring_key(d.ctypes.data, occ.ctypes.data, C.byref(sq))
    if rc != 0:
        raise RuntimeError(f"lins_host_place_ring_key: {rc}")
    return occ, int(sq.value)


def host_guess(pose_q, pose_c, shift, up_axis=1):
    """lins_host_place_team_guess -> T0 (4 x 4 f64): the start of lins_rendezvous_step's alignments, or the C return code"""
    from ._ctypes_defs import KeyPoseC, key_pose

    L = _host.lib()
    T = np.zeros(16, np.float64)
    pq, pc = key_pose(pose_q), key_pose(pose_c)
    L.lins_host_place_team_guess.argtypes, L.lins_host_place_team_guess.restype = [C.POINTER(KeyPoseC), C.POINTER(KeyPoseC), C.c_int, C.c_int, C.c_void_p], C.c_int
    rc = L.lins_host_place_team_guess(C.byref(pq), C.byref(pc), int(shift), int(up_axis), T.ctypes.data)
    return T.reshape(4, 4) if rc == 0 else rc


def host_topk(query, query_slot, query_id, now, min_gap_s, targets, raw=False, **kw):
    """lins_host_place_team_topk.  targets: [(slot, descs (n x 1200 or a list of (20, 60)), times)] -> the filled ranks'
    dicts, or the C return code (a negative int) of a refusal.  raw: (all k records, ranks filled)."""
    L = _host.lib()
    prm = place_team_params(L, **kw)
    k, n = max(int(prm.k), 1), len(targets)
    q = np.ascontiguousarray(query, np.float32).reshape(1200)
    keep = []
    slots, cnt = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    dp, tp = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))()
    for t, (slot, descs, times) in enumerate(targets):
        m = len(descs)
        D = np.ascontiguousarray(descs, np.float32).reshape(m, 1200) if m else np.zeros((1, 1200), np.float32)
        T = np.ascontiguousarray(times, np.float64) if m else np.zeros(1)
        assert len(T) >= m
        keep += [D, T]
        slots[t], cnt[t], dp[t], tp[t] = slot, m, D.ctypes.data, T.ctypes.data
    out = (PlaceTeamResultC * k)()
    L.lins_host_place_team_topk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.POINTER(PlaceTeamParamsC), C.POINTER(PlaceTeamResultC)]
    L.lins_host_place_team_topk.restype = C.c_int
    rc = L.lins_host_place_team_topk(q.ctypes.data, int(query_slot), int(query_id), float(now), float(min_gap_s), n, slots.ctypes.data, dp, tp,
                                     cnt.ctypes.data, C.byref(prm), out)
    if rc < 0:
        return rc
    res = _raw(out, k, rc)
    return res if raw else res[0][:rc]
