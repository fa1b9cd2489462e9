"""Seeded groups of the pairwise-consistency tests (tests/test_team_pcm_host.py, tests/test_gpu_team_pcm.py), built on
pose_graph_cases.trajectory and team_graph_cases.member: the smallest shapes at which the text of csrc/host/team_pcm.h
can go wrong.

A case is a dict: name, members (pose_graph_cases cases; member m is index m), factors: tuples (member_b, id_b, member_a,
id_a, Z (12,) f64, var), params: fields of lins_team_pcm_params over the defaults, want: the fields of the result the
issue states outright (the checker of tests/team_pcm_np.py is asked for all of them).

A factor is built from the transform X it is to CLAIM — from the map frame of its larger member into that of its smaller
one — and a small seeded perturbation on the right of Z (metres along and degrees about seeded unit vectors): with X the
identity and no perturbation the factor is the two frames' relative pose as pushed."""
import numpy as np

import pose_graph_np as pnp
import team_graph_cases as tgc

VAR = 1e-4


def transform(metres, degrees, seed):
    """a rigid transform of `degrees` about a seeded axis through the origin and `metres` along a seeded direction"""
    rng = np.random.default_rng(seed)
    ax, dr = rng.normal(size=3), rng.normal(size=3)
    return pnp.so3_exp(np.deg2rad(degrees) * ax / np.linalg.norm(ax)), metres * dr / np.linalg.norm(dr)


IDENT = (np.eye(3), np.zeros(3))


def factor(members, mb, ib, ma, ia, X=IDENT, metres=0.0, degrees=0.0, seed=0, var=VAR):
    Tb, Ta = pnp.pose_from6(members[mb]["aft"][ib]), pnp.pose_from6(members[ma]["aft"][ia])
    G = X if mb < ma else pnp.inv(X)  # a's map frame into b's
    Z = pnp.mul(pnp.inv(Tb), pnp.mul(G, Ta))
    if metres or degrees:
        R, t = transform(metres, degrees, 9000 + seed)
        Z = pnp.mul(Z, (R, t))
    return (mb, ib, ma, ia, pnp.flat([Z])[0], var)


def case(name, members, factors, want=None, **params):
    return dict(name=name, members=members, factors=factors, params=params, want=want or {})


def pair_members(n=64):
    return [tgc.member(201, n), tgc.member(202, n)]


def near(members, i, seed, mb=0, ma=1, ib=None):
    """a factor on frames (i, i) that claims the identity within 0.02 m and 0.1 degrees"""
    return factor(members, mb, i if ib is None else ib, ma, i, IDENT, 0.02, 0.1, seed)


def duplicates(k, **params):
    """k frame pairs x 3 identical factors: the complete k-partite graph with parts of 3"""
    m = pair_members()
    fs = []
    for i in range(k):
        f = near(m, 2 * i, 100 + i)
        fs += [f, f, f]
    return m, fs


def planted():
    """11: 8 factors on a pair of 130-frame members: 6 inliers (<= 0.05 m, <= 0.2 degrees) on the near side of the arc, 2
    outliers that claim a frame 2 m and 10 degrees off, on its far side — where 10 degrees about the map origin is metres"""
    m = [tgc.member(211, 130), tgc.member(212, 130)]
    out_x = [transform(2.0, 10.0, 31), transform(2.0, 10.0, 32)]
    fs = [
        factor(m, 0, 2, 1, 3, IDENT, 0.05, 0.2, 1),
        factor(m, 0, 70, 1, 71, out_x[0], 0.0, 0.0, 2),
        factor(m, 1, 8, 0, 6, IDENT, 0.04, 0.15, 3),  # (listed from the higher member)
        factor(m, 0, 10, 1, 10, IDENT, 0.05, 0.1, 4),
        factor(m, 0, 14, 1, 15, IDENT, 0.03, 0.2, 5),
        factor(m, 0, 80, 1, 78, out_x[1], 0.0, 0.0, 6),
        factor(m, 0, 18, 1, 18, IDENT, 0.02, 0.2, 7),
        factor(m, 0, 22, 1, 21, IDENT, 0.05, 0.05, 8),
    ]
    return case("planted", m, fs, dict(kept=[0, 2, 3, 4, 6, 7], n_pairs=1, n_pairs_kept=1, exact=1))


PLANTED_INLIERS, PLANTED_OUTLIERS = [0, 2, 3, 4, 6, 7], [1, 5]


def cases():
    """the cases 1 .. 9 and 11 of the issue's list, by name (10 is the planted case behind a rebase: the tests build it)"""
    m = pair_members()
    out = [
        # 1
        case("empty", m, [], dict(kept=[], n_pairs=0, n_pairs_kept=0, exact=1, nodes_max=0)),
        case("one_kept", m, [near(m, 3, 1)], dict(kept=[0], n_pairs=1, n_pairs_kept=1, nodes_max=1), min_support=1),
        case("one_dropped", m, [near(m, 3, 1)], dict(kept=[], n_pairs=1, n_pairs_kept=0), min_support=2),
        # 2
        case("two_inside", m, [near(m, 3, 1), near(m, 9, 2)], dict(kept=[0, 1]), min_support=2),
        case("two_outside", m, [near(m, 3, 1), factor(m, 0, 9, 1, 9, transform(3.0, 0.0, 5))], dict(kept=[]), min_support=2),
        case("two_turned", m, [near(m, 3, 1), factor(m, 0, 4, 1, 4, transform(0.0, 12.0, 6))], dict(kept=[]), min_support=2),
        # 3
        case("all_64", m, [near(m, i, 10 + i) for i in range(64)], dict(kept=list(range(64)), nodes_max=64, exact=1)),
        case("all_33", m, [near(m, i, 10 + i) for i in range(33)], dict(kept=list(range(33)), nodes_max=33, exact=1)),
        # 4
        case("one_frame_pair_twice", m, [near(m, 5, 1), near(m, 5, 2), near(m, 9, 3), near(m, 12, 4)], dict(kept=[0, 2, 3])),
    ]
    # 5
    m3 = [tgc.member(203, 20), tgc.member(204, 20), tgc.member(205, 20)]
    f5 = [near(m3, 2, 1), near(m3, 5, 2), near(m3, 6, 3, mb=1, ma=0), near(m3, 4, 4, mb=1, ma=2), near(m3, 9, 5), near(m3, 8, 6, mb=1, ma=2)]
    out += [
        case("three_members_support_3", m3, f5, dict(kept=[0, 1, 2, 4], n_pairs=2, n_pairs_kept=1)),
        case("three_members_support_2", m3, f5, dict(kept=[0, 1, 2, 3, 4, 5], n_pairs=2, n_pairs_kept=2), min_support=2),
    ]
    # 6
    far = transform(4.0, 0.0, 7)
    f6 = [factor(m, 0, 2 + 3 * i, 1, 2 + 3 * i, far if i % 2 == 0 else IDENT, 0.02, 0.1, 40 + i) for i in range(6)]
    out.append(case("two_cliques_of_3", m, f6, dict(kept=[0, 2, 4], n_pairs=1)))
    # 7 (the arc's frames are about 2 m apart: 1.5 m is a claim about the map frames, not the frames' distance)
    f7 = [factor(m, 0, 5, 1, 5), factor(m, 0, 15, 1, 15, transform(1.5, 0.0, 8))]
    out += [
        case("drift_off", m, f7, dict(kept=[]), min_support=2),
        case("drift_on", m, f7, dict(kept=[0, 1]), min_support=2, translation_per_frame=0.03),
    ]
    # 8
    m9, f9 = duplicates(9)
    m10, f10 = duplicates(10)
    out += [
        case("dup_9", m9, f9, dict(kept=list(range(0, 27, 3)), exact=1, nodes_max=23087)),
        case("dup_10_enough", m10, f10, dict(kept=list(range(0, 30, 3)), exact=1, nodes_max=81739), max_nodes=81739),
        case("dup_10_one_short", m10, f10, dict(kept=list(range(0, 30, 3)), exact=0), max_nodes=81738),
        case("dup_10_default", m10, f10, dict(kept=list(range(0, 30, 3)), exact=0)),
    ]
    # 9
    m21, f21 = duplicates(21)
    out.append(case("dup_21", m21, f21, dict(n_kept=21, exact=0, kept=list(range(0, 63, 3)))))
    out.append(planted())
    return out


def random_graph(seed, density, n=64):
    """adjacency rows (python ints) of a seeded graph"""
    rng = np.random.default_rng(seed)
    adj = [0] * n
    for a in range(n):
        for b in range(a + 1, n):
            if rng.random() < density:
                adj[a] |= 1 << b
                adj[b] |= 1 << a
    return adj


# seeds the checker shows exact under the default budget (tests/test_team_pcm_host.py asserts it)
RANDOM_GRAPHS = [(1, 0.5), (2, 0.5), (1, 0.8), (2, 0.8)]
