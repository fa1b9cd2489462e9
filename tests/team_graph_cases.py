"""Seeded groups of the team-graph tests (tests/test_team_graph_host.py, tests/test_gpu_team_graph.py), built from
pose_graph_cases.trajectory / corrected: the smallest shapes at which the text of csrc/pose_graph_team.h can go wrong.

A group is a dict: name, members (pose_graph_cases cases, member 0 the anchor), root_variance (6,), factors: tuples
(member_b, id_b, member_a, id_a, Z (12,) f64, variance).  A factor's Z is the relative pose T_b^-1 T_a of the two frames AS
PUSHED moved by a stated perturbation: metres along and degrees about seeded unit vectors, applied on the right."""
import numpy as np

import pose_graph_cases as pgc
import pose_graph_np as pnp

ROOT_VARIANCE = np.array([1e-4, 1e-4, 1e-4, 1e-2, 1e-2, 1e-2])  # a root may turn by 0.01 rad and move by 0.1 m (1 sigma)


def member(seed, n, loops=(), **kw):
    return pgc.case("m%d" % seed, seed, n, list(loops), **kw)


def factor(members, mb, ib, ma, ia, metres, degrees, var, seed):
    rng = np.random.default_rng(seed)
    ax, dr = rng.normal(size=3), rng.normal(size=3)
    d = np.concatenate([np.deg2rad(degrees) * ax / np.linalg.norm(ax), metres * dr / np.linalg.norm(dr)])
    Tb, Ta = pnp.pose_from6(members[mb]["aft"][ib]), pnp.pose_from6(members[ma]["aft"][ia])
    Z = pnp.retract(pnp.mul(pnp.inv(Tb), Ta), d)
    return (mb, ib, ma, ia, pnp.flat([Z])[0], var)


def group(name, members, factors, root_variance=ROOT_VARIANCE):
    """factors: (member_b, id_b, member_a, id_a, metres, degrees, variance)"""
    return dict(name=name, members=members, root_variance=np.asarray(root_variance, np.float64),
                factors=[factor(members, *f, seed=7000 + 10 * len(name) + i) for i, f in enumerate(factors)])


def cases():
    """the groups 1 .. 10 of the issue's list, by name"""
    B = pgc.PREFIX_BLOCK
    out = [
        # 1 two members, N = 3 and 5, one factor
        group("n3_n5", [member(101, 3, turn=0.3), member(102, 5, turn=0.4)], [(1, 4, 0, 2, 0.05, 0.5, 1e-4)]),
        # 2 a non-anchor member that is a root alone
        group("root_alone", [member(103, 6, turn=0.5), member(104, 1)], [(1, 0, 0, 3, 0.05, 0.5, 1e-4)]),
        # 3 a factor at the anchor's frame 0: the anchor's side of the support is empty
        group("anchor_frame_0", [member(105, 5, turn=0.4), member(106, 7, turn=0.5)], [(1, 3, 0, 0, 0.05, 0.5, 1e-4)]),
        # 4 members of 33 and 65 frames, factors on the edges of the prefix blocks
        group("block_edges", [member(107, B + 1), member(108, 2 * B + 1)],
              [(1, B - 1, 0, B, 0.1, 0.5, 1e-4), (0, B - 1, 1, B, 0.05, 0.3, 1e-4), (1, B + 1, 0, B, 0.05, 0.3, 1e-4),
               (1, 2 * B, 0, B - 1, 0.1, 0.5, 1e-4)]),
        # 5 the group runs past 256 lanes
        group("n130_n130", [member(109, 130), member(110, 130)], [(1, 129, 0, 5, 0.2, 1.0, 1e-4), (0, 120, 1, 10, 0.1, 0.5, 1e-4)]),
        # 6 two factors between the same pair: two-interval intersections in S
        group("same_pair_twice", [member(111, 12, turn=1.0), member(112, 14, turn=1.0)],
              [(1, 10, 0, 4, 0.1, 0.5, 1e-4), (1, 3, 0, 9, 0.05, 0.5, 1e-4)]),
        # 7 a member's own loops overlapping a team factor's support from either side
        group("own_loops_overlap", [member(113, 20, [(15, 2, 0.1, 0.5, 1e-6)]), member(114, 20, [(18, 8, 0.1, 0.5, 1e-6)])],
              [(1, 12, 0, 10, 0.1, 0.5, 1e-4)]),
        # 8 three members chained A-B and B-C: C has no factor to the anchor
        group("chain_of_three", [member(115, 8, turn=0.8), member(116, 9, turn=0.8), member(117, 7, turn=0.8)],
              [(1, 7, 0, 3, 0.1, 0.5, 1e-4), (2, 4, 1, 2, 0.1, 0.5, 1e-4)]),
        # 9 a non-anchor member with no factor at all (and one loop of its own)
        group("member_without_factor", [member(118, 8, turn=0.8), member(119, 9, turn=0.8), member(120, 10, [(9, 1, 0.1, 0.5, 1e-6)], turn=0.8)],
              [(1, 7, 0, 3, 0.1, 0.5, 1e-4)]),
        # 10 no loops and no factors
        group("nothing_to_solve", [member(121, 4, turn=0.3), member(122, 5, turn=0.3)], []),
    ]
    return out


def capacity_case(max_loops):
    """11: two members with one loop each and 2 * max_loops - 2 factors — exactly the cap of a group of two under
    lins_pose_graph_init(.., max_loops) — and one factor more"""
    members = [member(123, 10, [(9, 1, 0.05, 0.3, 1e-6)], turn=0.8), member(124, 10, [(8, 0, 0.05, 0.3, 1e-6)], turn=0.8)]
    n = 2 * max_loops - 2
    full = group("at_the_cap", members, [(1, 1 + i % 8, 0, 9 - i % 8, 0.05, 0.3, 1e-4) for i in range(n)])
    over = group("over_the_cap", members, [(1, 1 + i % 8, 0, 9 - i % 8, 0.05, 0.3, 1e-4) for i in range(n + 1)])
    return full, over


def checker_group(g):
    """the group as tests/team_graph_np.py takes it"""
    return dict(members=[pgc.graph_of(c) for c in g["members"]], root_variance=g["root_variance"],
                factors=[(mb, ib, ma, ia, pnp.unflat(Z)[0], var) for mb, ib, ma, ia, Z, var in g["factors"]])
