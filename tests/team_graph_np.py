"""An independent checker of the team graph, written from the contract (include/lins_team.h "team graph", DESIGN.md §5.3
"Team graph") on the primitives of tests/pose_graph_np.py and not from csrc/pose_graph_team.h: a dense numpy f64
Levenberg-Marquardt over the ABSOLUTE poses of all members, every Jacobian from central differences.

A group is a dict
    members        list of pose_graph_np graphs (aft, last, loops), member 0 the anchor
    root_variance  (6,) the variances of every non-anchor member's root factor, rotation first
    factors        list of (member_b, id_b, member_a, id_a, Z (R, t), variance)
The anchor's frame 0 is held FIXED by leaving its six columns out.  It must not be a weighed factor: the root priors of
the other members are absolute, so the gauge argument of the single checker (a prior that is met exactly costs nothing)
no longer holds — a weighed anchor would share the team factors' pull with the other roots."""
import numpy as np

import pose_graph_np as pnp


def offsets(group):
    n = [len(g["aft"]) for g in group["members"]]
    return np.concatenate([[0], np.cumsum(n)]).astype(int)


def build(group):
    """the factors over the concatenated poses: list of (i, j, Z, variances); i = -1: a root factor E = Z^-1 T_j"""
    off, F = offsets(group), []
    for m, g in enumerate(group["members"]):
        for i, j, Z, var in pnp.build(g):
            if i < 0:
                if m == 0:
                    continue  # the anchor's prior holds exactly: its frame 0 is no unknown
                var = np.asarray(group["root_variance"], np.float64)
            F.append((i + off[m] if i >= 0 else -1, j + off[m], Z, var))
    for mb, ib, ma, ia, Z, var in group["factors"]:
        F.append((off[mb] + ib, off[ma] + ia, Z, np.full(6, np.float64(var))))
    return F


def initial(group):
    return [T for g in group["members"] for T in pnp.initial(g)]


def free_columns(n_poses):
    return np.arange(6, 6 * n_poses)  # all but the anchor's frame 0


def gradient_with_scale(F, T):
    J, r = pnp.jacobian(F, T), pnp.residuals(F, T)
    keep = free_columns(len(T))
    return (J.T @ r)[keep], (np.abs(J).T @ np.abs(r))[keep]


def step(F, T, lam=0.0):
    J, r = pnp.jacobian(F, T), pnp.residuals(F, T)
    keep = free_columns(len(T))
    J = J[:, keep]
    d = np.zeros(6 * len(T))
    d[keep] = np.linalg.solve(J.T @ J + lam * np.eye(len(keep)), -J.T @ r)
    return d


def solve(F, T0, max_iter=100, tol=1e-13):
    """pose_graph_np.solve with the anchor's frame 0 fixed -> (poses, iterations)"""
    T, lam, c = list(T0), 1e-9, pnp.cost(F, T0)
    for it in range(max_iter):
        d = step(F, T, lam)
        Tn = [pnp.retract(T[k], d[6 * k:6 * k + 6]) for k in range(len(T))]
        cn = pnp.cost(F, Tn)
        if cn < c:
            T, lam = Tn, lam * 0.1
            small = np.abs(d).max() < tol or c - cn <= 1e-15 * c
            c = cn
            if small:
                return T, it + 1
        else:
            lam *= 10
            if np.abs(d).max() < tol or lam > 1e12:
                return T, it + 1
    return T, max_iter
