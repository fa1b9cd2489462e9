"""Pairwise-consistent team factors (include/lins_host.h lins_host_team_factors_consistent) stated a second time, for the
tests: X by 4 x 4 numpy products, the angle by arccos, the distance by norm, the clique by brute force over all subsets
where a pair has at most 16 factors, and — for every size — by a Python statement of the contract's recursive search that
counts nodes the same way.  Nothing here shares code with csrc/host/team_pcm.h.

A factor is a tuple (member_b, id_b, member_a, id_a, Z (12,), var); Tb, Ta are (n, 12) poses, R row-major then t."""
import numpy as np

DEFAULTS = dict(max_translation=1.0, min_cos_rotation=0.99619469809174555, translation_per_frame=0.0, min_support=3, max_nodes=65536)


def mat4(T):
    T = np.asarray(T, np.float64).reshape(12)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = T[:9].reshape(3, 3), T[9:]
    return M


def records(factors, Tb, Ta):
    """per factor dict(u, v, iu, iv, X (4, 4): v's map frame to u's, p (3,): where robot v stood)"""
    out = []
    for (mb, ib, ma, ia, Z, _), tb, ta in zip(factors, Tb, Ta):
        B, A, Z4 = mat4(tb), mat4(ta), mat4(Z)
        if mb < ma:
            out.append(dict(u=mb, v=ma, iu=ib, iv=ia, X=B @ Z4 @ np.linalg.inv(A), p=A[:3, 3].copy()))
        else:
            out.append(dict(u=ma, v=mb, iu=ia, iv=ib, X=A @ np.linalg.inv(Z4) @ np.linalg.inv(B), p=B[:3, 3].copy()))
    return out


def angle(a, b):
    """the rotation between the two transforms, radians"""
    return float(np.arccos(np.clip((np.trace(a["X"][:3, :3].T @ b["X"][:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))


def apart(a, b):
    """the larger of the two distances |X_a p - X_b p|, p where either robot stood"""
    return max(float(np.linalg.norm((a["X"] - b["X"]) @ np.append(p, 1.0))) for p in (a["p"], b["p"]))


def bar(a, b, prm):
    return prm["max_translation"] + prm["translation_per_frame"] * float(abs(a["iu"] - b["iu"]) + abs(a["iv"] - b["iv"]))


def consistent(a, b, prm):
    if (a["u"], a["v"]) != (b["u"], b["v"]) or (a["iu"], a["iv"]) == (b["iu"], b["iv"]):
        return False
    return angle(a, b) <= np.arccos(prm["min_cos_rotation"]) and apart(a, b) <= bar(a, b, prm)


def adjacency(recs, prm):
    n = len(recs)
    adj = [0] * n
    for l in range(n):
        for m in range(l + 1, n):
            if consistent(recs[l], recs[m], prm):
                adj[l] |= 1 << m
                adj[m] |= 1 << l
    return adj


class _Exhausted(Exception):
    pass


def subproblem(s, adj, max_nodes):
    """the contract's visit(R, |R|, P) for the cliques whose smallest member is s -> (mask, size, nodes, exhausted)"""
    best = [1 << s, 1]
    nodes = [0]

    def visit(R, nR, P):
        nodes[0] += 1
        if nodes[0] > max_nodes:
            raise _Exhausted
        if P == 0:
            if nR > best[1]:
                best[:] = [R, nR]
            return
        while P:
            if nR + bin(P).count("1") <= best[1]:
                return
            w = P & -P
            P ^= w
            visit(R | w, nR + 1, P & adj[w.bit_length() - 1])

    try:
        visit(1 << s, 1, adj[s] & ~((2 << s) - 1))
        exhausted = False
    except _Exhausted:
        exhausted = True
    return best[0], best[1], nodes[0], exhausted


def brute_force(vertices, adj):
    """the maximum clique among `vertices` with the lexicographically smallest ascending index list, over all subsets"""
    k = len(vertices)
    assert k <= 16
    best = ()
    for sub in range(1, 1 << k):
        pick = [vertices[i] for i in range(k) if (sub >> i) & 1]
        if len(pick) < len(best) or (len(pick) == len(best) and pick >= list(best)):
            continue
        mask = sum(1 << v for v in pick)
        if all((adj[v] | (1 << v)) & mask == mask for v in pick):
            best = tuple(pick)
    return best


def clique(adj, pair, prm, brute=True):
    """the result record of a graph: adj rows as ints, pair keys"""
    n = len(adj)
    subs = [subproblem(s, adj, prm["max_nodes"]) for s in range(n)]
    kept, n_pairs, n_pairs_kept = [], 0, 0
    for key in sorted(set(pair), key=list(pair).index):
        vs = [l for l in range(n) if pair[l] == key]
        w = min(vs, key=lambda s: (-subs[s][1], s))
        members = [l for l in range(n) if (subs[w][0] >> l) & 1]
        if brute and len(vs) <= 16 and not any(subs[s][3] for s in vs):
            assert tuple(members) == brute_force(vs, adj), (members, brute_force(vs, adj))
        n_pairs += 1
        if len(members) >= prm["min_support"]:
            n_pairs_kept += 1
            kept += members
    return dict(n_factors=n, n_kept=len(kept), n_pairs=n_pairs, n_pairs_kept=n_pairs_kept, exact=int(not any(s[3] for s in subs)),
                nodes_max=max([s[2] for s in subs] + [0]), kept=sorted(kept))


def evaluate(factors, Tb, Ta, **kw):
    prm = dict(DEFAULTS, **kw)
    recs = records(factors, Tb, Ta)
    return clique(adjacency(recs, prm), [(r["u"], r["v"]) for r in recs], prm)
