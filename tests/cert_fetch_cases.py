"""Hand-built scan pairs for tests/test_gpu_cert_fetch.py (in the style of _big_turn_pair of tests/test_gpu_tail.py): the
smallest inputs on which a candidate fetch on a clamped grid position (csrc/ieskf_lds_impl.h pt_rec) can go wrong.  Every
builder returns (pair, check): check(result, traces) asserts ON THE ORACLE'S OWN TRACE that the input does what it was
built for, so that a change of the generator or of a default cannot quietly turn a case into an ordinary scan.

Conventions: a point is (x, y, z, ring + 0.1 * relative time); targets are sorted by ring; the prior state is the identity
but for a translation that is off, and the prior covariance frees that translation only — the update is a one-dimensional,
well-conditioned problem whatever the handful of rows."""
import os
import re

import numpy as np

F = np.float32
# Variance of the freed translation.  The rows leave a variance of 1e-5; (I - K H) P loses prior / posterior digits to
# cancellation whatever sums the rows: from a prior of 1.0 the oracle's own dense and reduced forms end 2.6e-11 apart in the
# state (a bar of 1e-12 on the covariance would measure the input); from 1e-3 they agree to 4e-15 / 3e-16.
PRIOR_VAR = 1e-3
EMPTY = np.zeros((0, 4), dtype=F)


def _pt(x, y, z, ring, rel_time):
    return [x, y, z, F(ring) + F(0.1 * rel_time)]


def _state(tx=0.0, ty=0.0, tz=0.0):
    s = np.zeros(19)
    s[0:3] = (tx, ty, tz)
    s[6] = 1.0
    s[18] = -9.81
    return s


def _cov(*free):
    c = np.zeros((18, 18))
    for k in free:
        c[k, k] = PRIOR_VAR
    return c


def mr_resident_positions():
    """LINS_MR_CAP of csrc/ieskf_lds_mr.hip: grid positions of a scan the batch kernel keeps in LDS (n_lds = min(n, that))."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lins---lidar-inertial-slam_amd", "csrc", "ieskf_lds_mr.hip")
    return int(re.search(r"#define LINS_MR_CAP (\d+)", open(src).read()).group(1))


# ---- a horizontal plane of 1, 2 or 3 target points -----------------------------------------------------------------------------
def tiny_plane_pair(pkg, n_targets, tz=0.05):
    """Three plane queries over a target cloud of n_targets points (ring 0: the third point, ring 1: second, first).  One
    point: position 0 is the only valid one, there is no runner-up; two: no third point; three: one plane, rows accepted."""
    a, b, d = (0.0, 0.0, -1.5), (-0.4, 0.35, -1.5), (0.45, 0.3, -1.5)
    targets = [_pt(*d, 0, 0.5), _pt(*b, 1, 0.5), _pt(*a, 1, 0.5)][3 - n_targets:]
    queries = [_pt(a[0] + dx, a[1] + dy, a[2], 1, 1.0) for dx, dy in ((0.03, 0.02), (-0.05, 0.04), (0.06, -0.03))]
    pair = pkg.ScanPair(np.array(queries, dtype=F), EMPTY, np.array(targets, dtype=F), EMPTY, _state(tz=tz), _cov(2))

    def check(want, tr):
        s = tr["surf"][:want.iters]
        assert (s["ind1"] >= 0).all()  # every query has its nearest neighbour in every iteration
        assert ((s["ind2"] >= 0) == (n_targets >= 2)).all() and ((s["ind3"] >= 0) == (n_targets >= 3)).all()
        assert (want.m_surf > 0) == (n_targets == 3)

    return pair, check


# ---- a wall: plane queries only, one of which finds its first neighbour late -----------------------------------------------------
def _wall_targets():
    t = []
    for ring in range(5):
        t += [_pt(5.0, -1.0 + 0.1 * k, -0.4 + 0.2 * ring, ring, 0.5) for k in range(21)]
        if ring == 2:  # a cluster far to the side: ring 2 twice, ring 3 once
            t += [_pt(5.0, 20.0, 0.0, 2, 0.5), _pt(5.0, 20.1, 0.0, 2, 0.5)]
        if ring == 3:
            t += [_pt(5.0, 20.05, 0.2, 3, 0.5)]
    return np.array(t, dtype=F)


def late_neighbour_pair(pkg, corner_queries=0, tx=0.6):
    """Ten plane queries on the wall x = 5 and a prior translation that is `tx` off along x: the first iteration takes it
    back.  An eleventh query stands 4.7 m in front of the far cluster: with the prior's translation it is 5.3 m away — beyond
    the 5 m threshold, no neighbour in iteration 0, its carry record never gets a walk part — and from iteration 1 on it
    has one.  corner_queries > 0 adds line queries over an EMPTY line cloud."""
    q = [_pt(5.0, -0.93 + 0.19 * k, -0.4 + 0.2 * (1 + k % 3) + 0.04, 1 + k % 3, 1.0) for k in range(10)]
    q.append(_pt(9.7, 20.0, 0.0, 2, 1.0))
    cq = np.array([_pt(4.0, 0.1 * k, 0.0, 2, 1.0) for k in range(corner_queries)], dtype=F).reshape(-1, 4)
    pair = pkg.ScanPair(np.array(q, dtype=F), cq, _wall_targets(), EMPTY, _state(tx=tx), _cov(0))

    def check(want, tr):
        s = tr["surf"][:want.iters]
        assert want.iters >= 4 and (s["ind1"][:, :10] >= 0).all() and want.m_surf >= 10
        assert s["ind1"][0, 10] < 0 and (s["ind1"][1:, 10] >= 0).all()  # p1 < 0 -> >= 0
        assert want.m_corner == 0

    return pair, check


# ---- poles: line queries only -------------------------------------------------------------------------------------------------------
def poles_pair(pkg, surf_queries=0, ty=0.3):
    """Eight line queries on three vertical poles (four rings each), the plane cloud empty; surf_queries > 0 adds plane
    queries over that EMPTY plane cloud."""
    poles = ((4.0, -1.0), (4.0, 0.0), (4.5, 1.0))
    t = [_pt(x, y, -0.3 + 0.2 * ring, ring, 0.5) for ring in range(4) for x, y in poles]
    q = [_pt(poles[k % 3][0] + 0.02, poles[k % 3][1] + 0.01, -0.3 + 0.2 * (1 + k % 2) + 0.05, 1 + k % 2, 1.0) for k in range(8)]
    sq = np.array([_pt(4.0, 0.1 * k, 0.0, 1, 1.0) for k in range(surf_queries)], dtype=F).reshape(-1, 4)
    pair = pkg.ScanPair(sq, np.array(q, dtype=F), EMPTY, np.array(t, dtype=F), _state(ty=ty), _cov(1))

    def check(want, tr):
        c = tr["corner"][:want.iters]
        assert want.iters >= 4 and (c["ind1"] >= 0).all() and (c["ind2"] >= 0).all() and want.m_corner >= 6 and want.m_surf == 0

    return pair, check


# ---- a room scan cut at the edge of the resident positions ------------------------------------------------------------------
def resident_edge_pair(pkg, host, oracle, prm, index=32000):
    """Room scan `index` with its plane targets cut so that the scan has n_lds + 1 grid positions, the last two of which
    are a ring of their own: two points 12 cm apart on a new top ring, above a point of the ring below.  Positions are
    sorted corner cloud first, then planes by ring: the two are positions n_lds - 1 — the last resident record — and n_lds
    — the only record read from global memory.  A plane query between them tracks both: nearest neighbour and runner-up,
    then second point (same ring)."""
    cap = mr_resident_positions()
    p = host.synth_pair(index)
    keep = cap + 1 - len(p.corner_last) - 2
    assert 0 < keep < len(p.surf_last)
    surf_last = p.surf_last[:keep]
    top = int(surf_last[-1, 3])  # (ring ids truncate)
    assert top < 15 and top >= 2
    below = surf_last[surf_last[:, 3].astype(int) == top]
    anchor = below[len(below) // 2]
    r = np.hypot(anchor[0], anchor[1])
    tang = np.array([-anchor[1], anchor[0], 0.0]) / r  # along the ring
    a = anchor[:3] + np.array([0.0, 0.0, 0.25]) - 0.06 * tang
    b = anchor[:3] + np.array([0.0, 0.0, 0.25]) + 0.06 * tang
    surf_last = np.vstack([surf_last, np.array([_pt(*a, top + 1, 0.5), _pt(*b, top + 1, 0.5)], dtype=F)])
    # the query: a raw point that the prior's de-skew puts 2 cm from b, towards a (fixed-point rounds on the transform).  Next to
    # b, the LAST target: the reference's forward walk ends at the number of QUERIES (SE:859), so only the backward walk
    # — from b to a, then down to the ring below — reaches these indices
    goal = b - 0.02 * tang + np.array([0.0, 0.0, 0.01])
    raw = np.array(_pt(*goal, top + 1, 1.0), dtype=F)
    for _ in range(3):
        got = oracle.transform_to_start(prm, p.state, raw.reshape(1, 4))[0]
        raw[:3] += (goal - got[:3]).astype(F)
    pair = pkg.ScanPair(np.vstack([p.surf_flat, raw.reshape(1, 4)]), p.corner_sharp, surf_last, p.corner_last, p.state, p.cov)
    ia, ib = len(surf_last) - 2, len(surf_last) - 1

    def check(want, tr):
        assert len(pair.surf_last) + len(pair.corner_last) == cap + 1
        s = tr["surf"][:want.iters, -1]
        # (the two change places as the state moves: the nearest neighbour is b in all but an iteration or two, then a)
        assert want.iters >= 4 and np.isin(s["ind1"], (ia, ib)).all() and (s["ind3"] >= 0).all()
        assert ((s["ind1"] == ib) & (s["ind2"] == ia)).sum() >= 3

    return pair, check
