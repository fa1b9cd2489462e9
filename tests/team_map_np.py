"""The team selection's contract (csrc/host/team_select.h, DESIGN.md §5.3 "Team map") stated independently in numpy, and
the cases the CPU and the GPU tests share.  A target is (slot, key poses (n, 6) f32); a case is a dict(name, targets,
centre, radius, leaf)."""
import itertools

import numpy as np

F = np.float32
E_ARG, E_CAPACITY = -1, -3


def poses6(xyz):
    p = np.zeros((len(xyz), 6), F)
    if len(xyz):
        p[:, :3] = np.asarray(xyz, F).reshape(-1, 3)
    return p


def team_select(targets, centre, radius, leaf):
    """-> the surviving (slot, id) pairs as a sorted list, E_ARG for a slot named twice, E_CAPACITY for a box of more
    than 2^31 cells.  A dictionary per cell and Python's tuple order: no sort by cell, no packed keys."""
    slots = [s for s, _ in targets]
    if len(set(slots)) != len(slots):
        return E_ARG
    c = np.asarray(centre, F)
    r2 = F(radius) * F(radius)
    inv = F(1.0) / F(leaf)
    best = {}
    for slot, poses in targets:
        p = np.asarray(poses, F).reshape(-1, 6)
        for i in range(len(p)):
            dx, dy, dz = p[i, 0] - c[0], p[i, 1] - c[1], p[i, 2] - c[2]
            d = F(F(dx * dx) + F(dy * dy)) + F(dz * dz)
            if not d <= r2:
                continue
            cell = tuple(int(np.floor(F(p[i, a] * inv))) for a in range(3))
            cand = (float(d), int(slot), i)
            if cell not in best or cand < best[cell]:
                best[cell] = cand
    if best:
        div = [max(k[a] for k in best) - min(k[a] for k in best) + 1 for a in range(3)]
        if div[0] * div[1] > 2 ** 31 or div[0] * div[1] * div[2] > 2 ** 31:
            return E_CAPACITY
    return sorted((s, i) for _, s, i in best.values())


def hits_of(targets, centre, radius):
    c, r2, n = np.asarray(centre, F), F(radius) * F(radius), 0
    for _, poses in targets:
        p = np.asarray(poses, F).reshape(-1, 6)
        d = ((p[:, 0] - c[0]) ** 2 + (p[:, 1] - c[1]) ** 2) + (p[:, 2] - c[2]) ** 2
        n += int((d <= r2).sum())
    return n


def lattice(n, seed):
    """n poses on a 0.5 m lattice in [-8, 8]^2 x [-1, 1]: equal distances, coincident poses, negative coordinates"""
    rng = np.random.default_rng(seed)
    return poses6(np.stack([0.5 * rng.integers(-16, 17, n), 0.5 * rng.integers(-16, 17, n), 0.5 * rng.integers(-2, 3, n)], 1))


def case(name, targets, centre, radius, leaf, want=None):
    return dict(name=name, targets=[(s, poses6(p) if not isinstance(p, np.ndarray) else p) for s, p in targets], centre=centre, radius=radius,
                leaf=leaf, want=want)


# want: the pairs by hand where they can be read off (None: the numpy statement decides alone)
CRAFTED = [
    case("no targets", [], (0, 0, 0), 5.0, 1.0, []),
    case("a target without frames", [(0, [(0.2, 0.2, 0)]), (1, []), (2, [(3.2, 0.2, 0)])], (0, 0, 0), 5.0, 1.0, [(0, 0), (2, 0)]),
    case("only targets without frames", [(0, []), (2, [])], (0, 0, 0), 5.0, 1.0, []),
    case("one pose", [(1, [(1, 2, 3)])], (1, 2, 3), 1.0, 1.0, [(1, 0)]),
    case("one pose out of reach", [(1, [(1, 2, 3)])], (9, 2, 3), 1.0, 1.0, []),
    # 3-4-5: d == r2 == 25 exactly; the second pose is just beyond
    case("a hit exactly on d == r2", [(0, [(3, 4, 0), (3, 4, 0.01)]), (1, [(0, 0, 9)])], (0, 0, 0), 5.0, 0.001, [(0, 0)]),
    case("radius 0", [(0, [(1, 2, 3), (1, 2, 3.5)]), (3, [(1, 2, 3)])], (1, 2, 3), 0.0, 0.1, [(0, 0)]),
    # x = -0.5, -1.0, -0.25 -> cell -1 (floor, not truncation: -0.25 does not share cell 0 with 0.5); -1.5 -> cell -2
    case("negative coordinates", [(0, [(-0.5, 0, 0), (-1.0, 0, 0), (-1.5, 0, 0)]), (1, [(0.5, 0, 0), (-0.25, 0, 0)])], (0, 0, 0), 3.0, 1.0,
         [(0, 2), (1, 0), (1, 1)]),
    # (0.25, 0.25) and (0.75, 0.75) are equally far from (0.5, 0.5) and share cell 0
    case("two slots at equal d in one cell", [(2, [(0.25, 0.25, 0)]), (1, [(0.75, 0.75, 0)])], (0.5, 0.5, 0), 2.0, 1.0, [(1, 0)]),
    case("the same slot at equal d", [(1, [(9, 9, 9), (0.75, 0.75, 0), (0.25, 0.25, 0)])], (0.5, 0.5, 0), 2.0, 1.0, [(1, 1)]),
    case("the nearer pose wins over the lower slot", [(0, [(0.9, 0.9, 0)]), (4, [(0.5, 0.5, 0)])], (0.5, 0.5, 0), 2.0, 1.0, [(4, 0)]),
    case("coincident poses in three slots", [(2, [(0.5, 0.5, 0.5)] * 3), (0, [(7, 7, 7), (0.5, 0.5, 0.5)]), (1, [(0.5, 0.5, 0.5)] * 2)], (0, 0, 0),
         2.0, 1.0, [(0, 1)]),
    # |coord| <= 1e6 and leaf 1e-3: 2e9 + 1 cells along x alone fit (<= 2^31), the plane with y does not
    case("2^31 cells: one axis fits", [(0, [(-1e6, 0, 0)]), (1, [(1e6, 0, 0)])], (0, 0, 0), 2e6, 1e-3, [(0, 0), (1, 0)]),
    case("2^31 cells: the plane does not", [(0, [(-1e6, 0, 0)]), (1, [(1e6, 1, 0)])], (0, 0, 0), 2e6, 1e-3, E_CAPACITY),
    case("2^31 cells: the volume does not", [(0, [(0, 0, 0)]), (1, [(40, 40, 2)])], (0, 0, 0), 100.0, 1e-3, E_CAPACITY),
    case("a slot named twice", [(1, [(0, 0, 0)]), (0, [(1, 0, 0)]), (1, [(0, 0, 0)])], (0, 0, 0), 2.0, 1.0, E_ARG),
]
THREE = [(0, lattice(40, 1)), (1, lattice(25, 2)), (2, lattice(33, 3))]
PERMUTED = [case("permutation %s" % (p,), [THREE[i] for i in p], (0.25, -0.25, 0), 4.0, 1.0) for p in itertools.permutations(range(3))]


def random_cases(n=200, seed=7):
    """seeded cases on the 0.5 m lattice, so that ties are frequent: 1 to 4 slots of 0 to 150 poses, shuffled slot numbers"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        slots = rng.permutation(6)[: int(rng.integers(1, 5))].tolist()
        targets = [(s, lattice(int(rng.integers(0, 151)), 1000 * seed + 10 * k + s)) for s in slots]
        centre = tuple(float(v) for v in 0.25 * rng.integers(-8, 9, 3) * np.array([1, 1, 0.25]))
        out.append(case("random %d" % k, targets, centre, float(rng.choice([1.0, 2.5, 6.0, 12.0])), float(rng.choice([0.5, 1.0, 1.5, 2.0]))))
    return out
