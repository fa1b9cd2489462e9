"""Hand-built scan pairs for tests/test_gpu_search_spans.py: the smallest inputs on which the bounds of a search window —
read on clamped cells, several windows to a trip, packed two positions to a word (csrc/ieskf_lds_impl.h spans_read /
spans_pack / scan_packed) — can go wrong.  Conventions and helpers are those of tests/cert_fetch_cases.py; every builder
returns (pair, critical, check): `critical` lists the (kind, query index) pairs the case is about, check(result, traces)
asserts ON THE ORACLE'S OWN TRACE that the input does what it was built for and that the oracle accepts at least one row, so
that no case passes vacuously.

The packed spans are used where a cold search has ONE lane (nn_lean, ln == 1): in a wave that holds more than 32 queries
(coop_lanes: 64 / n rounded down to a power of two).  The batch shape deals a scan's plane queries to five waves in
contiguous blocks by the weights LINS_SPREAD_WS, its line queries to three waves in equal blocks (wr_layout of
csrc/ieskf_lds_impl.h); one_lane() restates that arithmetic, and the test asserts for every case that its critical
queries sit in such a wave — a case built with a handful of queries would run the untouched two-lane path."""
import os
import re

import numpy as np

from cert_fetch_cases import EMPTY, F, _cov, _pt, _state, mr_resident_positions

AZ_SURF = 128  # azimuth columns of the plane cloud's grid (csrc/ieskf_binned.h kAzSurf): 2 pi / 128 rad each
PLANE_WAVES, LINE_WAVES = 5, 3


def _col(x, y, naz=AZ_SURF):
    return int(np.floor((np.arctan2(y, x) + np.pi) * naz / (2 * np.pi)))


# ---- which queries search with one lane in the cold iteration -----------------------------------------------------------------
def spread_weights():
    """LINS_SPREAD_WS of csrc/ieskf_lds_impl.h: the weights of the five plane shares."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lins---lidar-inertial-slam_amd", "csrc", "ieskf_lds_impl.h")
    m = re.search(r"#define LINS_SPREAD_WS ([\d, ]+?)\s*//", open(src).read())
    w = [int(x) for x in m.group(1).split(",")]
    assert len(w) == PLANE_WAVES
    return w


def shares(n, weights):
    """[first, last) query of every wave of a kind with n queries: floor(n * cumulated weight / total weight)."""
    tot, cum, out = sum(weights), 0, []
    for w in weights:
        out.append((n * cum // tot, n * (cum + w) // tot))
        cum += w
    return out


def one_lane(n_planes, n_lines):
    """{"surf": set of plane query indices, "corner": set of line query indices} whose wave holds more than 32 queries.  (Every
    share must fit a wave, or the kernel falls back to another layout.)"""
    out = {}
    for kind, n, wts in (("surf", n_planes, spread_weights()), ("corner", n_lines, [1] * LINE_WAVES)):
        sh = shares(n, wts)
        assert all(b - a <= 64 for a, b in sh), (kind, sh)
        out[kind] = {q for a, b in sh if b - a > 32 for q in range(a, b)}
    return out


# ---- a wall at x = +-5 m: rings of 21 points 10 cm apart, plane queries on it ------------------------------------------------------
def _z_wall(ring):
    return -0.4 + 0.2 * ring


def _wall(x, rings, z_of):
    return [_pt(x, -1.0 + 0.1 * k, z_of(ring), ring, 0.5) for ring in rings for k in range(21)]


def _wall_queries(x, n, rings, z_of):
    return [_pt(x, -0.93 + 1.86 * (k + 0.5) / n, z_of(rings[k % len(rings)]) + 0.04, rings[k % len(rings)], 1.0) for k in range(n)]


def wall_pair(pkg, x=5.0, rings=(0, 1, 2, 3, 4), query_rings=(1, 2, 3), n_queries=200, tx=0.6, first_queries=(), z_of=_z_wall, line_queries=0):
    """n_queries plane queries on the wall at `x` (behind `first_queries`), the prior translation `tx` off along x (the first
    iteration takes it back).  200 queries: the first three plane waves hold 60, 48 and 40 — one lane per cold search for
    queries 0..147.  x = -5: the wall lies across azimuth +-pi, where the last column is followed by column 0 — seeds and
    windows of every ring are two spans.  line_queries > 0 adds line queries over an EMPTY line cloud."""
    nf = len(first_queries)
    q = list(first_queries) + _wall_queries(x, n_queries, query_rings, z_of)
    cq = np.array([_pt(4.0, -1.0 + 0.02 * k, 0.0, 2, 1.0) for k in range(line_queries)], dtype=F).reshape(-1, 4)
    pair = pkg.ScanPair(np.array(q, dtype=F), cq, np.array(_wall(x, rings, z_of), dtype=F), EMPTY, _state(tx=tx), _cov(0))

    def check(want, tr):
        s = tr["surf"][:want.iters]
        assert want.iters >= 4 and (s["ind1"][:, nf:] >= 0).all() and want.m_surf >= n_queries and want.m_corner == 0, (want.iters, want.m_surf)

    return pair, [("surf", k) for k in range(nf + min(n_queries, 30))], check


def wrap_pair(pkg):
    pair, _, base = wall_pair(pkg, x=-5.0, tx=-0.6)
    qcol = [_col(p[0], p[1]) for p in pair.surf_flat]
    critical = [("surf", k) for k, a in enumerate(qcol) if a in (0, AZ_SURF - 1)]  # their own seed a0 - 1 .. a0 + 1 wraps

    def check(want, tr):
        base(want, tr)
        cols = {_col(p[0], p[1]) for p in pair.surf_last}
        assert 0 in cols and AZ_SURF - 1 in cols  # the wall straddles the seam: on every ring, own and neighbour
        assert {qcol[k] for _, k in critical} == {0, AZ_SURF - 1} and len(critical) >= 20

    return pair, critical, check


def outer_rings_pair(pkg):
    """A low wall on rings 0-2 and a high one on rings 13-15; the queries sit on ring 0 and on ring 15: rq - 1, rho - 1 and
    rho - 2 (rq + 1, rho + 1, rho + 2) name rings that do not exist."""
    z_of = lambda ring: _z_wall(ring) if ring < 8 else (0.6 + 0.2 * (ring - 13))
    pair, _, check = wall_pair(pkg, rings=(0, 1, 2, 13, 14, 15), query_rings=(0, 15), z_of=z_of)
    return pair, [("surf", k) for k in range(40)], check  # (rings alternate: twenty of each)


def gap_ring_pair(pkg):
    """Ring 2 of the wall is empty: the neighbour ring of the queries on rings 1 and 3."""
    pair, _, check = wall_pair(pkg, rings=(1, 3, 4, 5), query_rings=(1, 3))
    return pair, [("surf", k) for k in range(40)], check


def deferred_pair(pkg):
    """The FIRST query stands 3 m to the side of the wall: its seed (three columns on three rings) is empty, the bound it
    leaves is the 5 m threshold, the window of that bound at rho = 6.4 m is every column: wider than LINS_HARD_COLS, the
    cold search is deferred.  Its nearest neighbour is the wall's end."""
    pair, _, base = wall_pair(pkg, first_queries=[_pt(5.0, 4.0, 0.04, 2, 1.0)])

    def check(want, tr):
        base(want, tr)
        s = tr["surf"][:want.iters, 0]
        assert (s["ind1"] >= 0).all()
        nn = pair.surf_last[int(s["ind1"][0])]
        assert abs(_col(5.6, 4.0) - _col(nn[0], nn[1])) > 4 and np.hypot(5.6 - nn[0], 4.0 - nn[1]) > 2.5

    return pair, [("surf", 0)], check


def no_lines_pair(pkg):
    """99 line queries over an EMPTY line cloud (33 to a wave: one lane each), beside the wall's plane queries."""
    pair, crit, check = wall_pair(pkg, line_queries=99)
    return pair, crit + [("corner", k) for k in range(99)], check


def wave_fill_pair(pkg, n_planes):
    """107 plane queries: the first plane wave of the batch shape (30 % of them) holds 32 — two lanes per cold search; 110: 33
    — one lane, the three seed rings in one trip."""
    pair, _, check = wall_pair(pkg, n_queries=n_planes)
    return pair, [("surf", k) for k in range(n_planes * 30 // 100)], check


# ---- poles: line queries, and plane queries over an empty plane cloud ------------------------------------------------------------
_POLES = ((4.0, -1.0), (4.0, 0.0), (4.5, 1.0))


def _pole_targets():
    return [_pt(x, y, -0.3 + 0.2 * ring, ring, 0.5) for ring in range(4) for x, y in _POLES]


def _pole_queries(n):
    return [_pt(_POLES[k % 3][0] + 0.02 + 0.0002 * (k // 6), _POLES[k % 3][1] + 0.01, -0.3 + 0.2 * (1 + k % 2) + 0.05, 1 + k % 2, 1.0) for k in range(n)]


def no_planes_pair(pkg, ty=0.3):
    """99 line queries on three vertical poles (33 to a wave) and 110 plane queries over an EMPTY plane cloud (33 in the
    first wave)."""
    sq = np.array([_pt(4.0, -1.0 + 0.02 * k, 0.0, 1, 1.0) for k in range(110)], dtype=F)
    pair = pkg.ScanPair(sq, np.array(_pole_queries(99), dtype=F), EMPTY, np.array(_pole_targets(), dtype=F), _state(ty=ty), _cov(1))

    def check(want, tr):
        c = tr["corner"][:want.iters]
        assert want.iters >= 4 and (c["ind1"] >= 0).all() and (c["ind2"] >= 0).all() and want.m_corner >= 90 and want.m_surf == 0

    return pair, [("surf", k) for k in range(33)] + [("corner", k) for k in range(99)], check


# ---- a horizontal plane of 1, 2 or 3 target points under 120 plane queries, and the poles ----------------------------------------
def tiny_pair(pkg, n_targets, tz=0.05):
    """120 plane queries (36 in the first wave) over a plane cloud of n_targets points (ring 0: the third point, ring 1: second,
    first).  One point: position 0 is the only valid one, every other cell the seed names is empty or clamped; two: no third
    point; three: one plane.  99 line queries on the poles give the oracle rows to accept whatever the plane cloud holds."""
    a, b, d = (0.0, 0.0, -1.5), (-0.4, 0.35, -1.5), (0.45, 0.3, -1.5)
    targets = [_pt(*d, 0, 0.5), _pt(*b, 1, 0.5), _pt(*a, 1, 0.5)][3 - n_targets:]
    queries = [_pt(a[0] + 0.08 * np.cos(0.7 * k), a[1] + 0.08 * np.sin(0.7 * k) * (1 + k % 3) / 3, a[2], 1, 1.0) for k in range(120)]
    pair = pkg.ScanPair(np.array(queries, dtype=F), np.array(_pole_queries(99), dtype=F), np.array(targets, dtype=F), np.array(_pole_targets(), dtype=F),
                        _state(tz=tz), _cov(2))

    def check(want, tr):
        s = tr["surf"][:want.iters]
        assert (s["ind1"] >= 0).all()  # every query has its nearest neighbour in every iteration
        assert ((s["ind2"] >= 0) == (n_targets >= 2)).all() and ((s["ind3"] >= 0) == (n_targets >= 3)).all()
        assert (want.m_surf > 0) == (n_targets == 3) and want.m_corner >= 90

    return pair, [("surf", k) for k in range(36)] + [("corner", k) for k in range(99)], check


# ---- a floor under the sensor: a query with rho = 0 -----------------------------------------------------------------------------------
def nadir_pair(pkg, tz=0.05):
    """A floor 1.5 m under the sensor: the nadir point and three rings around it (no three points in a line: a plane of
    collinear points has no normal); the first query is raw (0, 0, z): with a prior that is off along z only its rho is
    exactly 0 in every iteration — reach_cols' quotient is inf, the window every column.  122 queries: 36 in the first wave."""
    polar = [(0, 0.0, 0.0)] + [(0, 0.12 + 0.01 * i, 90.0 + 90.0 * i) for i in range(4)]
    polar += [(1, 0.30 + 0.01 * i, 45.0 * i) for i in range(8)] + [(2, 0.50 + 0.005 * i, 7.0 + 30.0 * i) for i in range(12)]
    t = [_pt(r * np.cos(np.radians(a)), r * np.sin(np.radians(a)), -1.5, ring, 0.5) for ring, r, a in polar]
    q = [_pt(0.0, 0.0, -1.5, 0, 1.0), _pt(0.03, 0.02, -1.5, 0, 1.0)]
    for rep in range(5):
        f, da = 0.9 - 0.04 * rep, 5.0 + 3.0 * rep
        q += [_pt(f * r * np.cos(np.radians(a + da)), f * r * np.sin(np.radians(a + da)), -1.5, ring, 1.0) for ring, r, a in polar[1:]]
    pair = pkg.ScanPair(np.array(q, dtype=F), EMPTY, np.array(t, dtype=F), EMPTY, _state(tz=tz), _cov(2))

    def check(want, tr):
        s = tr["surf"][:want.iters]
        assert want.iters >= 4 and (s["ind1"] >= 0).all() and (s["ind3"][:, 0] >= 0).all() and want.m_surf >= 100, (want.iters, want.m_surf)
        assert tr["surf"]["accepted"][want.iters - 1, 0]  # the query at the nadir has its row
        assert pair.surf_flat[0, 0] == 0 and pair.surf_flat[0, 1] == 0

    return pair, [("surf", 0)], check


# ---- a room scan cut at the edge of the resident positions ------------------------------------------------------------------------
def resident_edge_pair(pkg, host, oracle, prm, steps, index=32000):
    """Room scan `index` with its plane targets cut so that the scan has n_lds + 1 grid positions, the last three of which are
    a ring of their own: u, v and w in ascending azimuth, `steps` columns apart, above a point of the ring below.  Positions
    are sorted corner cloud first, then planes by ring and column: the three are positions n_lds - 2, n_lds - 1 (the last
    resident record) and n_lds (the only global one).  u is the LAST target (the reference's forward walk ends at the number
    of queries, SE:859: only the backward walk reaches these indices).  The FIRST plane query stands next to u.
      steps (0, 0.3, 0.6)   all three inside the seed's columns a0 - 1 .. a0 + 1: the seed window of the query's own ring
                            starts resident and ends global;
      steps (0, 3.2, 4.2)   v and w outside the seed: the second point, on the same ring, is found by the widening round to
                            the right, which reads v and w in ONE window across the last resident record."""
    cap = mr_resident_positions()
    p = host.synth_pair(index)
    keep = cap + 1 - len(p.corner_last) - 3
    assert 0 < keep < len(p.surf_last)
    surf_last = p.surf_last[:keep]
    top = int(surf_last[-1, 3])
    assert 2 <= top < 15
    below = surf_last[surf_last[:, 3].astype(int) == top]
    anchor = below[len(below) // 2]
    r = np.hypot(anchor[0], anchor[1])
    tang = np.array([-anchor[1], anchor[0], 0.0]) / r  # along the ring, towards larger azimuth
    w_col = 2 * np.pi / AZ_SURF * r
    up = np.array([0.0, 0.0, 0.25])
    u, v, w = (anchor[:3] + up + s * w_col * tang for s in steps)
    surf_last = np.vstack([surf_last, np.array([_pt(*v, top + 1, 0.5), _pt(*w, top + 1, 0.5), _pt(*u, top + 1, 0.5)], dtype=F)])
    goal = u + 0.1 * (v - u) + np.array([0.0, 0.0, 0.01])
    raw = np.array(_pt(*goal, top + 1, 1.0), dtype=F)
    for _ in range(3):
        got = oracle.transform_to_start(prm, p.state, raw.reshape(1, 4))[0]
        raw[:3] += (goal - got[:3]).astype(F)
    pair = pkg.ScanPair(np.vstack([raw.reshape(1, 4), p.surf_flat]), p.corner_sharp, surf_last, p.corner_last, p.state, p.cov)
    iv, iw, iu = len(surf_last) - 3, len(surf_last) - 2, len(surf_last) - 1

    def check(want, tr):
        assert len(pair.surf_last) + len(pair.corner_last) == cap + 1
        cu, cv, cw = (_col(q[0], q[1]) for q in (u, v, w))
        if steps[1] >= 2:
            assert cu + 2 <= cv <= cw < AZ_SURF - 1, (cu, cv, cw)  # ascending positions, v and w outside the seed of a query at u
        else:
            assert cu <= cv <= cw <= cu + 1 < AZ_SURF - 1, (cu, cv, cw)  # ascending positions, all in the seed of a query at u
        s = tr["surf"][:want.iters, 0]
        assert want.iters >= 4 and (s["ind1"] == iu).all() and np.isin(s["ind2"], (iv, iw)).all() and (s["ind3"] >= 0).all() and want.m_surf > 0

    return pair, [("surf", 0)], check
