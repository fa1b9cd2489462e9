"""The consensus rule of a rendezvous over a window (include/lins_host.h lins_host_rendezvous_consensus) stated a second
time, independently, in numpy — dense 4 x 4 products, np.trace, norms — and the tables the host and the device tests
share (not a test).

The restatement rounds differently from the scalar text, so it can only be held to equal DECISIONS, and only on tables
where no pair lies on a bar: near_bars() counts the comparable pairs within a relative 1e-9 of either bar, and the tests
assert that count to be 0 on the seeded tables — a condition on the inputs, not a tolerance.

A hypothesis is a dict(X (4, 4) f64, p (3,), fitness, query, rank, target_slot, admissible)."""
import functools

import numpy as np

MAX_T, MIN_COS = 1.0, 0.99619469809174555  # the defaults: 1 m, cos 5 degrees
N_TABLES = 200


def comparable(a, b):
    return bool(a["admissible"] and b["admissible"] and a["target_slot"] == b["target_slot"] and a["query"] != b["query"])


def measures(a, b):
    """(trace of Ra^T Rb, the larger of |Xa p - Xb p| at p_a and p_b)"""
    Xa, Xb = np.asarray(a["X"], np.float64).reshape(4, 4), np.asarray(b["X"], np.float64).reshape(4, 4)
    tr = float(np.trace(Xa[:3, :3].T @ Xb[:3, :3]))
    far = max(float(np.linalg.norm((Xa @ np.append(p, 1.0))[:3] - (Xb @ np.append(p, 1.0))[:3])) for p in (np.asarray(a["p"], np.float64), np.asarray(b["p"], np.float64)))
    return tr, far


def consistent(a, b, max_t=MAX_T, min_cos=MIN_COS):
    if not comparable(a, b):
        return False
    tr, far = measures(a, b)
    return tr >= 1.0 + 2.0 * min_cos and far <= max_t


def near_bars(hyps, max_t=MAX_T, min_cos=MIN_COS, rel=1e-9):
    """comparable pairs whose trace or distance lies within `rel` (relative) of its bar"""
    n = 0
    for i, a in enumerate(hyps):
        for b in hyps[i + 1:]:
            if comparable(a, b):
                tr, far = measures(a, b)
                bar = 1.0 + 2.0 * min_cos
                n += int(abs(tr - bar) <= rel * abs(bar) or abs(far - max_t) <= rel * max_t)
    return n


def consensus(hyps, max_t=MAX_T, min_cos=MIN_COS):
    """dict(winner, support, n_admissible, members) as host.rendezvous_consensus gives it"""
    H = len(hyps)
    star = [[b for b in range(H) if b != a and consistent(hyps[a], hyps[b], max_t, min_cos)] for a in range(H)]
    support = [len({hyps[a]["query"]} | {hyps[b]["query"] for b in star[a]}) if hyps[a]["admissible"] else 0 for a in range(H)]
    adm = [a for a in range(H) if hyps[a]["admissible"]]
    if not adm:
        return dict(winner=-1, support=0, n_admissible=0, members=[])
    w = min(adm, key=lambda a: (-support[a], hyps[a]["fitness"], -hyps[a]["query"], hyps[a]["rank"]))
    return dict(winner=w, support=support[w], n_admissible=len(adm), members=sorted([w] + star[w]))


# ---- the tables --------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def transform(R, t):
    X = np.eye(4)
    X[:3, :3], X[:3, 3] = R, t
    return X


def hyp(X, p=(0, 0, 0), fitness=0.1, query=0, rank=0, target_slot=0, admissible=1):
    return dict(X=np.asarray(X, np.float64).reshape(4, 4), p=np.asarray(p, np.float64), fitness=float(fitness), query=int(query), rank=int(rank),
                target_slot=int(target_slot), admissible=int(admissible))


def shift(t, **kw):
    """the identity rotation with translation t"""
    return hyp(transform(np.eye(3), t), **kw)


def table(seed):
    """two or three clusters of X with noise on both sides of the bars: up to 8 degrees and 1.6 m about a cluster's centre, so
    pairs of one cluster fall inside and outside; H between 2 and 128 distinct (query, rank); three target slots; one in five
    inadmissible, half of those with NaN where nothing may read them"""
    rng = np.random.default_rng(1000 + seed)
    H = int(rng.choice([2, 5, 17, 40, 63, 64, 65, 100, 127, 128]))
    centres = [(rotation(rng.normal(size=3), rng.uniform(0, 3.0)), rng.uniform(-20, 20, 3), int(rng.integers(0, 3))) for _ in range(int(rng.integers(2, 4)))]
    out = []
    for qr in rng.permutation(128)[:H]:
        R, t, slot = centres[int(rng.integers(0, len(centres)))]
        X = transform(rotation(rng.normal(size=3), np.deg2rad(rng.uniform(0, 4.0))) @ R, t + rng.normal(size=3) * rng.uniform(0, 0.8))
        h = hyp(X, p=rng.uniform(-20, 20, 3), fitness=rng.uniform(0, 0.3), query=int(qr) // 8, rank=int(qr) % 8,
                target_slot=slot if rng.uniform() < 0.9 else int(rng.integers(0, 3)), admissible=int(rng.uniform() < 0.8))
        if not h["admissible"] and rng.uniform() < 0.5:
            h["X"] = np.full((4, 4), np.nan)
            h["fitness"] = float("inf")
        out.append(h)
    return out


@functools.lru_cache(maxsize=None)
def tables():
    return [table(s) for s in range(N_TABLES)]


def permuted(hyps, seed=0):
    """(the table in another order, perm): permuted[i] = hyps[perm[i]]"""
    perm = [int(i) for i in np.random.default_rng(seed).permutation(len(hyps))]
    return [hyps[i] for i in perm], perm


def corners():
    """name -> (hyps, params kw, expectation: a dict of the fields it pins, or None where only host == numpy == device is asked)"""
    one = np.nextafter(1.0, 2.0)
    c = {}
    c["empty"] = ([], {}, dict(winner=-1, support=0, n_admissible=0, members=[]))
    c["one"] = ([shift((1, 2, 3), query=4, rank=2)], {}, dict(winner=0, support=1, n_admissible=1, members=[0]))
    c["one, inadmissible"] = ([shift((1, 2, 3), admissible=0)], {}, dict(winner=-1, support=0, n_admissible=0, members=[]))
    # all of one query: support 1 however well they agree; the smallest fitness wins
    c["one query"] = ([shift((0, 0, 0), query=3, rank=r, fitness=0.2 - 0.01 * r) for r in range(8)], {}, dict(winner=7, support=1, n_admissible=8, members=[7]))
    # two target slots interleaved: the same X into another map frame is no witness
    c["two slots"] = ([shift((0, 0, 0), query=q, target_slot=q % 2, fitness=0.1 + 0.01 * q) for q in range(5)], {},
                      dict(winner=0, support=3, n_admissible=5, members=[0, 2, 4]))
    # exact ties in support and fitness: the larger query, then the smaller rank
    c["tie by query"] = ([shift((0, 0, 0), query=q, fitness=0.125) for q in (2, 7, 5)], {}, dict(winner=1, support=3, members=[0, 1, 2]))
    c["tie by rank"] = ([shift((0, 0, 0), query=1, rank=3, fitness=0.125), shift((0, 0, 0), query=6, rank=5, fitness=0.125),
                         shift((0, 0, 0), query=6, rank=2, fitness=0.125), shift((9, 9, 9), query=6, rank=0, fitness=0.125)], {},
                        dict(winner=2, support=2, n_admissible=4, members=[0, 2]))
    # a pair exactly on the translation bar: identity rotations, integer translations and positions, max_translation 1
    c["on the translation bar"] = ([shift((3, 0, 0), p=(1, 2, 3), query=0, fitness=0.1), shift((4, 0, 0), p=(-2, 0, 5), query=1, fitness=0.2)],
                                   dict(max_translation=1.0), dict(winner=0, support=2, members=[0, 1]))
    # (one nextafter beyond: px = 0, so that a coordinate of X p is 0 + t, exactly t)
    c["beyond the translation bar"] = ([shift((0, 0, 0), p=(0, 2, 3), query=0, fitness=0.1), shift((one, 0, 0), p=(0, 0, 5), query=1, fitness=0.2)],
                                       dict(max_translation=1.0), dict(winner=0, support=1, members=[0]))
    # ... and on the rotation bar: the trace of I^T I is 3 = 1 + 2 * 1
    c["on the rotation bar"] = ([shift((0, 0, 0), query=0, fitness=0.1), shift((0, 0, 0), query=1, fitness=0.2)], dict(min_cos_rotation=1.0),
                                dict(winner=0, support=2, members=[0, 1]))
    c["beyond the rotation bar"] = ([shift((0, 0, 0), query=0, fitness=0.1), shift((0, 0, 0), query=1, fitness=0.2)], dict(min_cos_rotation=one),
                                    dict(winner=0, support=1, members=[0]))
    # the bar holds where the robot stood, not at the origin: 0.4 degrees apart is 0.07 m at 10 m and 1.4 m at 200 m
    near, far = (10.0, 0, 0), (200.0, 0, 0)
    turned = transform(rotation((0, 0, 1), np.deg2rad(0.4)), (0, 0, 0))
    c["lever arm, near"] = ([shift((0, 0, 0), p=near, query=0), hyp(turned, p=near, query=1, fitness=0.2)], {}, dict(winner=0, support=2))
    c["lever arm, far"] = ([shift((0, 0, 0), p=near, query=0), hyp(turned, p=far, query=1, fitness=0.2)], {}, dict(winner=0, support=1))
    # a star, not a clique: 0.8 m either side of the winner are 1.6 m from each other and both are members
    c["star"] = ([shift((0, 0, 0), query=0, fitness=0.05), shift((0.8, 0, 0), query=1, fitness=0.2), shift((-0.8, 0, 0), query=2, fitness=0.2)], {},
                 dict(winner=0, support=3, members=[0, 1, 2]))
    # a full table, every (query, rank) once: ranks 0 agree, the rest scatter
    c["full"] = ([shift((0.01 * q, 0, 0) if r == 0 else (50.0 * r, 7.0 * q, 0), query=q, rank=r, fitness=0.1 + 0.001 * q + 0.01 * r) for q in range(16)
                  for r in range(8)], {}, dict(winner=0, support=16, n_admissible=128, members=list(range(0, 128, 8))))
    return c


def sized(H, seed=5):
    """a table of exactly H hypotheses (the wave and workgroup edges): two clusters, all admissible"""
    rng = np.random.default_rng(seed + H)
    out = []
    for qr in rng.permutation(128)[:H]:
        out.append(shift(np.array([30.0 * int(rng.integers(0, 2)), 0, 0]) + rng.normal(size=3) * 0.3, p=rng.uniform(-5, 5, 3), fitness=rng.uniform(0, 0.3),
                         query=int(qr) // 8, rank=int(qr) % 8))
    return out
