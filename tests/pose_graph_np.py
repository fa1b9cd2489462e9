"""An independent checker of the pose graph, written from the contract (include/lins_map.h "the pose graph", DESIGN.md
§5.3 "Pose graph") and not from csrc/pose_graph_math.h: a dense numpy f64 Levenberg-Marquardt over ABSOLUTE poses with the
full 6 N Jacobian, the prior included as a factor, every Jacobian from central differences of the residual.

A pose is (R, t): R (3, 3), t (3,).  A graph is a dict
    aft    (N, 6) f32   the six floats (pitch, yaw, roll, y, z, x) each frame was pushed with (frame 0: the prior)
    last   (N, 6) f32   the six floats each frame's odometry factor was formed against (row 0 unused)
    loops  list of (latest, closest, Z (R, t), variance)
Residual of a between-factor Z on (Ti, Tj): E = Z^-1 Ti^-1 Tj, r = (Log R_E, t_E); retraction (R Exp(w), t + R v)."""
import numpy as np

ODO_VAR = np.array([1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6])


def rot_axis(axis, a):
    c, s = np.cos(a), np.sin(a)
    if axis == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == 1:
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def rzryrx(x, y, z):
    return rot_axis(2, np.float64(z)) @ rot_axis(1, np.float64(y)) @ rot_axis(0, np.float64(x))


def pose_from6(p):
    p = np.asarray(p, np.float32).astype(np.float64)
    return rzryrx(p[2], p[0], p[1]), np.array([p[5], p[3], p[4]])


def pose_from_lidar(k):
    """(x, y, z, roll, pitch, yaw) as lins_host_loop_pose_from returns it"""
    k = np.asarray(k, np.float32).astype(np.float64)
    return rzryrx(k[3], k[4], k[5]), k[:3].copy()


def angles_of(R):
    return np.arctan2(R[2, 1], R[2, 2]), np.arcsin(-R[2, 0]), np.arctan2(R[1, 0], R[0, 0])


def pose_to6(T):
    x, y, z = angles_of(T[0])
    return np.array([y, z, x, T[1][1], T[1][2], T[1][0]]).astype(np.float32)


def key_pose_of6(p):
    """six floats -> PointTypePose (x, y, z, roll, pitch, yaw) as LM:1721-1733"""
    return np.array([p[3], p[4], p[5], p[0], p[1], p[2]], np.float32)


def lidar_of_pose(T):
    """pose -> (x, y, z, roll, pitch, yaw) with R = RzRyRx(roll, pitch, yaw), rounded to f32"""
    x, y, z = angles_of(T[0])
    return np.array([T[1][0], T[1][1], T[1][2], x, y, z]).astype(np.float32)


def mul(A, B):
    return A[0] @ B[0], A[0] @ B[1] + A[1]


def inv(A):
    return A[0].T, -A[0].T @ A[1]


def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def so3_exp(w):
    th = np.linalg.norm(w)
    K = hat(w)
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def so3_log(R):
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.linalg.norm(v), 0.5 * (np.trace(R) - 1)
    if s < 1e-8:
        return v * (1 + s * s / 6)
    return v * (np.arctan2(s, c) / s)


def retract(T, d):
    return T[0] @ so3_exp(d[:3]), T[1] + T[0] @ d[3:]


def between_residual(Z, Ti, Tj):
    E = mul(inv(Z), mul(inv(Ti), Tj))
    return np.concatenate([so3_log(E[0]), E[1]])


def build(graph, estimate=None):
    """the factors of a graph: list of (i, j, Z, variances (6,)), i = -1 for the prior (E = Z^-1 Tj)"""
    aft, last = graph["aft"], graph["last"]
    F = [(-1, 0, pose_from6(aft[0]), ODO_VAR)]
    for k in range(1, len(aft)):
        F.append((k - 1, k, mul(inv(pose_from6(last[k])), pose_from6(aft[k])), ODO_VAR))
    for b, a, Z, var in graph["loops"]:
        F.append((b, a, Z, np.full(6, np.float64(np.float32(var)))))
    return F


def loop_measurement(pose_from_lidar6, closest6):
    """Z_l = pose_from^-1 T_a with T_a from the six floats the estimate of the closest frame is held as"""
    return mul(inv(pose_from_lidar(pose_from_lidar6)), pose_from6(closest6))


IDENT = (np.eye(3), np.zeros(3))


def factor_residual(f, T):
    i, j, Z, var = f
    return between_residual(Z, IDENT if i < 0 else T[i], T[j]) / np.sqrt(var)


def residuals(F, T):
    return np.concatenate([factor_residual(f, T) for f in F])


def cost(F, T):
    r = residuals(F, T)
    return 0.5 * r @ r


def jacobian(F, T, h=1e-3):
    """(6 |F|, 6 N) by central differences of the whitened residual along the retraction: the five-point stencil
    (-f(2h) + 8 f(h) - 8 f(-h) + f(-2h)) / 12 h.  With h = 1e-3 its truncation, h^4 f^(5) / 30 with f^(5) of the order of
    the lever arm (<= 100 m), is about 3e-12, and its rounding, 1e-14 / h for residuals formed from coordinates <= 100 m,
    about 1e-11 — against 5e-9 for the three-point stencil at its best step."""
    J = np.zeros((6 * len(F), 6 * len(T)))
    for n, f in enumerate(F):
        for v in {f[0], f[1]} - {-1}:
            for c in range(6):
                d = np.zeros(6)
                d[c] = h

                def at(s):
                    Ts = list(T)
                    Ts[v] = retract(T[v], s * d)
                    return factor_residual(f, Ts)

                J[6 * n:6 * n + 6, 6 * v + c] = (-at(2) + 8 * at(1) - 8 * at(-1) + at(-2)) / (12 * h)
    return J


def gradient(F, T):
    return jacobian(F, T).T @ residuals(F, T)


def gradient_with_scale(F, T):
    """(J^T r, |J|^T |r|): the gradient and the size of the terms that cancel in it, component by component"""
    J, r = jacobian(F, T), residuals(F, T)
    return J.T @ r, np.abs(J).T @ np.abs(r)


def gauss_newton_step(F, T, lam=0.0):
    J, r = jacobian(F, T), residuals(F, T)
    H = J.T @ J + lam * np.eye(J.shape[1])
    return np.linalg.solve(H, -J.T @ r)


def solve(F, T0, max_iter=100, tol=1e-13):
    """Levenberg-Marquardt; stops when the step is below tol or the cost no longer falls.  -> (poses, iterations)"""
    T, lam, c = list(T0), 1e-9, cost(F, T0)
    for it in range(max_iter):
        d = gauss_newton_step(F, T, lam)
        Tn = [retract(T[k], d[6 * k:6 * k + 6]) for k in range(len(T))]
        cn = cost(F, Tn)
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


def initial(graph):
    return [pose_from6(p) for p in graph["aft"]]


def flat(T):
    """list of (R, t) -> (N, 12): R row-major, t"""
    return np.array([np.concatenate([R.reshape(9), t]) for R, t in T])


def unflat(A):
    return [(np.asarray(a[:9]).reshape(3, 3), np.asarray(a[9:12])) for a in np.asarray(A).reshape(-1, 12)]
