"""Built correspondence sets for the loop-closure ICP's fit and stop step (csrc/loop_icp_math.h fit_from_sums,
kabsch_rotation, compose, step_from_sums), their 17 sums and an exact reference of the fit.

A case is a small set of pairs (x'_k, g_k) of f32 points.  From it come
  the sums       sums() in plain numpy f64, split() over 1, 2 or 5 tiles; a case marked dyadic has coordinates k 2^-j
                 and exact sums and means whatever the order (asserted by tests/test_loop_fit_inputs.py);
  the reference  reference(): the CENTRED H in fractions.Fraction over the f32 inputs (products of floats are exact
                 rationals), rounded once to f64, np.linalg.svd, R = V diag(1, 1, sign det(V U^T)) U^T, t = mu_g - R mu_s.
                 No text of loop_icp_math.h, no cancellation.

The forward bar on R (Frobenius norm of the difference) is
    bar_R = K 2^-53 (m + sigma1) / (sigma2 + d sigma3),    m = S |x'_k| |g_k| + n |mu_s| |mu_g|
from the perturbation bound of the constrained Procrustes rotation, |dR| <= 2 |dH| / (sigma2 + d sigma3), with |dH| the
rounding of an n-term f64 sum of magnitude m plus a backward-stable 3 x 3 SVD.  The bar on t is bar_R (|mu_s| + 1) +
2^-52 |mu_g|.  K is calibrated against references only (calibrate(): the raw-moment H in plain numpy f64 followed by
LAPACK, held against the exact reference over every case with a determined rotation): the worst ratio of the difference
to bar_R / K measured 1.333 (case rotations/yaw90; numpy's LAPACK on x86-64), K = 8 x that: K = 10.7.
|R^T R - I| (largest entry) is held to ORTHO = 256 x 2^-53: 30 plane rotations and one cross product, each orthogonal to a
few units in the last place.

A case's `gap` is (sigma2 + d sigma3) / sigma1 of its reference; the cases called well-posed have gap >= 1e-3 — every
case but the rank < 2 ones (collinear_*, coincident: the contract promises the identity, no bar applies) and the 1e-6
and 1e-9 rungs of gap_ladder, which are held to their (wider) bars all the same.

Rank < 2: the contract treats sigma2 <= C_RANK 2^-53 sigma1 as rank < 2.  collinear_floor() measures what the reference
computation (raw moments in numpy f64, LAPACK) leaves as sigma2 / sigma1 for EXACTLY collinear f32 points — lines of at
least 1 m within 100 m of the origin: at most 1.66e3 x 2^-53; C_RANK = 2^14 is 8 x that rounded up to a power of two."""
from fractions import Fraction

import numpy as np

import loop_icp_np as lnp

F = np.float32
U53 = 2.0 ** -53
K = 10.7
C_RANK = 2.0 ** 14  # loop_icp_math.h kRankFloor = C_RANK x 2^-53: see collinear_floor()
ORTHO = 256 * U53
T_GEN = np.array([0.3, 0.2, 0.1])


def rot_axis(axis, deg):
    """Rodrigues, f64"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def base_cloud(n=64):
    """the fixed generic cloud: a room's worth of spread, different on every axis (f64; cases round it to f32)"""
    rng = np.random.default_rng(41)
    return rng.uniform(-1, 1, (n, 3)) * np.array([9.0, 6.0, 2.5]) + np.array([1.0, -2.0, 0.5])


def case(name, X, G, **kw):
    X, G = np.ascontiguousarray(X, F).reshape(-1, 3), np.ascontiguousarray(G, F).reshape(-1, 3)
    assert len(X) == len(G) and 3 <= len(X) <= 320
    c = dict(name=name, X=X, G=G, tiles=1, rank=3, dyadic=False, exact=False, identity=False, perm=None, mirror=False)
    c.update(kw)
    return c


def rigid(name, s64, R, t=T_GEN, **kw):
    return case(name, s64.astype(F), (s64 @ R.T + t).astype(F), **kw)


# ---- the cases --------------------------------------------------------------------------------------------------------
def rotations():
    """g = R s + t: yaw, pitch and roll of 0 .. 180 degrees and a generic axis at 120 — large-angle fits, trace R = -1"""
    s, out = base_cloud(), []
    for an, ax in (("yaw", (0, 0, 1)), ("pitch", (0, 1, 0)), ("roll", (1, 0, 0))):
        for deg in (0.0, 1e-9, 2.0, 45.0, 90.0, 179.9, 180.0):
            out.append(rigid(f"rotations/{an}{deg:g}", s, rot_axis(ax, deg), tiles=2 if deg == 2.0 else 1, angle=deg))
    out.append(rigid("rotations/generic120", s, rot_axis((1.0, -2.0, 0.7), 120.0), angle=120.0))
    return out


def lattice_cloud(n, z):
    """the first n nodes of an 8 x 5 lattice of 1 m spacing in x, y (row by row) with the heights z[k] — dyadic"""
    k = np.arange(n)
    return np.stack([(k % 8).astype(np.float64), (k // 8).astype(np.float64), np.asarray(z, np.float64)[:n]], 1)


def mirror_pairs(n=32):
    """`mirror` (also run end to end, at n = 31, 32, 33): lattice nodes 1/16 m above or below z = 0 in a fixed irregular
    pattern, g = s with z negated — 1/8 m apart, so that nearest-neighbour pairing is the identity pairing.  H is about
    diag(a, b, -c), c = n / 256 far below b: the unconstrained optimum is the reflection, the answer a proper rotation
    within 1e-2 rad of the identity.  Dyadic: every sum is exact in any order."""
    z = np.where(np.random.default_rng(7).random(40) < 0.5, -0.0625, 0.0625)
    s = lattice_cloud(n, z)
    return s.astype(F), (s * np.array([1.0, 1.0, -1.0])).astype(F)


def planar_pairs(n=32):
    """`planar/z0` (also run end to end): lattice nodes in z = 0 exactly, g = Rz(1 degree) s + (0.1, 0.05, 0): rank 2"""
    s = lattice_cloud(n, np.zeros(40))
    g = s @ rot_axis((0, 0, 1), 1.0).T + np.array([0.1, 0.05, 0.0])
    g[:, 2] = 0.0
    return s.astype(F), g.astype(F)


def mirror():
    X, G = mirror_pairs(32)
    return [case("mirror", X, G, mirror=True, dyadic=True, tiles=2)]


def aniso_cloud(spreads, n=32, seed=3):
    """a cloud with the given spreads per axis and small cross moments: orthogonal sign columns, generic magnitudes"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    signs = np.stack([1 - 2 * ((k >> b) & 1) for b in (0, 1, 2)], 1).astype(np.float64)
    return signs * np.asarray(spreads) * (1 + 0.3 * rng.uniform(-1, 1, (n, 3))) + 0.05 * rng.normal(size=(n, 3)) + np.array([0.4, -0.3, 0.2])


def mirror_each_axis():
    """g = s with one axis negated, for each axis and each order of the spreads (weak axis first, second, third in H): the
    sign must land on the smallest singular direction whatever the column order; perm[k] = the axis the k-th largest
    singular value belongs to — all six orders occur"""
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        spreads = np.empty(3)
        spreads[list(perm)] = (8.0, 3.5, 1.2)
        s = aniso_cloud(spreads)
        for ax in range(3):
            flip = np.ones(3)
            flip[ax] = -1.0
            out.append(case(f"mirror_each_axis/flip{'xyz'[ax]}_order{''.join(map(str, perm))}", s.astype(F), (s.astype(F) * flip.astype(F)),
                            mirror=True, perm=perm))
    return out


E1, E2 = np.array([1.0, 2.0, -1.0]), np.array([3.0, -1.0, 2.0])       # a generic plane, integer directions
E1G, E2G = np.array([2.0, 1.0, 1.0]), np.array([-1.0, -2.0, 3.0])     # the same lengths and angle: an exact rigid image


def plane_uv(n=24):
    rng = np.random.default_rng(11)
    return rng.integers(-12, 13, (n, 2)).astype(np.float64) / 4.0


def planar():
    """rank 2 exactly: z = 0, and a generic plane spanned by integer vectors with g in its exact rigid image"""
    X, G = planar_pairs(32)
    uv = plane_uv()
    s = np.array([0.5, -1.25, 2.0]) + uv[:, :1] * E1 + uv[:, 1:] * E2
    g = np.array([-0.75, 1.5, 0.25]) + uv[:, :1] * E1G + uv[:, 1:] * E2G
    return [case("planar/z0", X, G, rank=2, tiles=2, plane=(0.0, 0.0, 1.0), flips_plane=False), case("planar/generic", s, g, rank=2, dyadic=True)]


def planar_mirror():
    """rank 2 and the in-plane optimum has a negative determinant — g is the mirror image of s within their common plane —
    so the answer turns the plane over: half a turn about an in-plane axis"""
    X, _ = planar_pairs(32)
    G = X * np.array([1.0, -1.0, 1.0], F) + np.array([0.25, 0.5, 0.0], F)
    uv = plane_uv() * np.array([1.0, 3.0])
    s = np.array([0.5, -1.25, 2.0]) + uv[:, :1] * E1 + uv[:, 1:] * E2
    # the mirror image across E1 within the plane: E2 -> 2 (E1 . E2) / |E1|^2 E1 - E2 = -E1 / 3 - E2 (v is a multiple of 3 / 4)
    g = np.array([-0.75, 1.5, 0.25]) + (uv[:, :1] - uv[:, 1:] / 3.0) * E1 - uv[:, 1:] * E2
    return [case("planar_mirror/z0", X, G, rank=2, dyadic=True, plane=(0.0, 0.0, 1.0), flips_plane=True),
            case("planar_mirror/generic", s, g, rank=2, dyadic=True, plane=tuple(np.cross(E1, E2)), flips_plane=True)]


def rank_below_2():
    """the contract: an H of rank < 2 gives the identity rotation"""
    k = np.arange(8, dtype=np.float64)
    axis = np.stack([k * 0.25, 0 * k, 0 * k], 1)
    u = np.array([-7, -3, -2, 0, 1, 4, 6, 9], np.float64)[:, None]
    line = np.array([0.5, 1.0, -0.25]) + u * np.array([1.0, 2.0, -1.0]) / 8.0          # exactly collinear, dyadic
    # exactly collinear and far from the origin, n = 12: the sums are exact, the means and so the f64 H are not
    u12 = np.array([-11, -9, -6, -5, -2, 0, 1, 3, 4, 8, 10, 13], np.float64)[:, None]
    gen = np.array([3.125, -1.75, 0.875]) + u12 * np.array([1517.0, -3318.0, 1802.0]) / 4096.0
    far = np.array([40.0, -30.5, 2.25]) + u12[::2] * np.array([37.0, -81.0, 44.0]) / 512.0  # a 2 m line 50 m out
    same = np.tile(np.array([[1.5, -2.25, 0.75]]), (8, 1))
    return [case("collinear_axis", axis, axis + np.array([0.5, 0, 0]), rank=1, dyadic=True, identity=True, exact=True),
            # (along z the one column that is not 0 is the LAST: every compare-and-swap has to run for the rank test to see it)
            case("collinear_axis/z", axis[:, ::-1], axis[:, ::-1] + np.array([0, 0.25, 0.5]), rank=1, dyadic=True, identity=True, exact=True),
            case("collinear_generic/dyadic", line, line + np.array([0.25, -0.5, 0.125]), rank=1, dyadic=True, identity=True),
            case("collinear_generic/n12", gen, gen + np.array([0.3, -0.2, 0.1]), rank=1, identity=True),
            case("collinear_generic/far", far, far + np.array([0.3, -0.2, 0.1]), rank=1, identity=True),
            case("coincident", same, same + np.array([0.5, 0.25, -1.0]), rank=0, dyadic=True, identity=True, exact=True)]


def isotropic():
    """H = c I exactly (octahedron vertices, g = s) and H = diag(a, a, b): gamma == 0 throughout, equal singular values;
    R must be I exactly — resp. the quarter turn"""
    o = np.concatenate([np.eye(3), -np.eye(3)])
    o2 = o * np.array([2.0, 2.0, 1.0])
    # (a quarter turn about z of the second: the columns of H are orthogonal and two are equally long — gamma == 0 with
    # alpha == beta — yet the answer is not the identity)
    return [case("isotropic/cI", o, o, dyadic=True, exact=True, identity=True), case("isotropic/aab", o2, o2, dyadic=True, exact=True, identity=True),
            case("isotropic/aab_turned", o2, o2 @ np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), dyadic=True, angle=90.0)]


def three_points():
    s = np.array([[1.0, 0.5, -0.25], [-2.0, 1.5, 0.75], [0.25, -3.0, 1.0]])
    return [rigid("three_points", s, rot_axis((0.3, 1.0, -0.5), 25.0), rank=2)]


QA, QB, QC = np.array([1.0, 2.0, 2.0]), np.array([2.0, 1.0, -2.0]), np.array([2.0, -2.0, 1.0])  # orthogonal, length 3


def gap_ladder():
    """pairs +-2a -> +-2a, +-b -> +-b, +-c -> -+c (mirrored along c), +-e b -> +-e b over the orthogonal integer vectors a,
    b, c: H = 8 a a^T + 2 (1 + e^2) b b^T - 2 c c^T, sigma = 72, 18 (1 + e^2), 18, d = -1: gap = e^2 / 4"""
    out = []
    for gap in (1e-3, 1e-6, 1e-9):
        e = F(2.0 * np.sqrt(gap))
        e = np.float64(e if np.float64(e) ** 2 / 4.0 >= gap else np.nextafter(e, F(1.0)))  # (the f32 at or above 2 sqrt(gap))
        s = np.stack([2 * QA, -2 * QA, QB, -QB, QC, -QC, e * QB, -e * QB])
        g = np.stack([2 * QA, -2 * QA, QB, -QB, -QC, QC, e * QB, -e * QB])
        out.append(case(f"gap_ladder/{gap:g}", s, g, mirror=True, want_gap=float(e * e / 4.0)))
    return out


def far_origin():
    """the 2 degree yaw case with the world's origin moved away by (1, 1, 0.1) x scale before the rounding to f32: what
    forming H from raw moments costs — m grows with the square of the offset"""
    s, R = base_cloud(), rot_axis((0, 0, 1), 2.0)
    out = []
    for scale in (0.0, 1e3, 1e5, 1e6):
        off = np.array([1.0, 1.0, 0.1]) * scale
        out.append(case(f"far_origin/{scale:g}", (s + off).astype(F), (s @ R.T + T_GEN + off).astype(F), tiles=5, far=scale))
    return out


def scales():
    """the 2 degree yaw case and the mirror of a generic cloud, x 1e-3 and x 1e3: no absolute threshold hides in the fit"""
    s, R = base_cloud(), rot_axis((0, 0, 1), 2.0)
    a = aniso_cloud((8.0, 3.5, 1.2))
    out = []
    for f in (1e-3, 1e3):
        out.append(case(f"scales/yaw2_x{f:g}", (f * s).astype(F), (f * (s @ R.T + T_GEN)).astype(F)))
        out.append(case(f"scales/mirror_x{f:g}", (f * a).astype(F), (f * a).astype(F) * np.array([1, 1, -1], F), mirror=True))
    return out


_CASES = None


def fit_cases():
    global _CASES
    if _CASES is None:
        _CASES = (rotations() + mirror() + mirror_each_axis() + planar() + planar_mirror() + rank_below_2() + isotropic() + three_points()
                  + gap_ladder() + far_origin() + scales())
        for c in _CASES:
            c["ref"] = reference(c["X"], c["G"])
            c["sums"] = sums(c["X"], c["G"])
    return _CASES


def by_name(name):
    return next(c for c in fit_cases() if c["name"] == name)


# ---- sums ---------------------------------------------------------------------------------------------------------------
def sqd(X, G):
    """the contract's f32 squared distance of each pair"""
    dx, dy, dz = (np.ascontiguousarray(X[:, k], F) - np.ascontiguousarray(G[:, k], F) for k in range(3))
    return ((dx * dx + dy * dy) + dz * dz).astype(F)


def sums(X, G):
    """the 17 sums in plain numpy f64: count, S x', S g, S x'_i g_j (7 + 3 i + j), S d"""
    x, g = X.astype(np.float64), G.astype(np.float64)
    out = np.zeros(17)
    out[0], out[1:4], out[4:7] = len(x), x.sum(0), g.sum(0)
    out[7:16] = (x[:, :, None] * g[:, None, :]).sum(0).reshape(9)
    out[16] = sqd(X, G).astype(np.float64).sum()
    return out


def split(X, G, tiles, pad=0, fill=np.nan):
    """the sums as `tiles` tile partials over consecutive runs of the pairs (they add up to sums() within rounding,
    exactly for a dyadic case), then `pad` tiles of `fill` no kernel may read: (tiles + pad, 17)"""
    cuts = np.linspace(0, len(X), tiles + 1).astype(int)
    parts = [sums(X[a:b], G[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return np.stack(parts + [np.full(17, fill)] * pad)


# ---- the reference ------------------------------------------------------------------------------------------------------
def _fr(a):
    return [[Fraction(float(v)) for v in row] for row in np.asarray(a, np.float64)]


def reference(X, G):
    """the exact centred H, rounded once; LAPACK's SVD; the constrained optimum"""
    x, g, n = _fr(X), _fr(G), len(X)
    ms = [sum(p[i] for p in x) / n for i in range(3)]
    mg = [sum(p[i] for p in g) / n for i in range(3)]
    Hx = [[sum((p[i] - ms[i]) * (q[j] - mg[j]) for p, q in zip(x, g)) for j in range(3)] for i in range(3)]
    H = np.array([[float(v) for v in row] for row in Hx])
    mu_s, mu_g = np.array([float(v) for v in ms]), np.array([float(v) for v in mg])
    U, sig, Vt = np.linalg.svd(H)
    V = Vt.T
    d = 1.0 if np.linalg.det(V @ U.T) >= 0 else -1.0
    R = V @ np.diag([1.0, 1.0, d]) @ U.T
    x64, g64 = X.astype(np.float64), G.astype(np.float64)
    m = float((np.linalg.norm(x64, axis=1) * np.linalg.norm(g64, axis=1)).sum() + n * np.linalg.norm(mu_s) * np.linalg.norm(mu_g))
    # the exact rank: of the exact rational H, by fraction arithmetic (no threshold)
    return dict(H=H, Hx=Hx, U=U, V=V, sig=sig, d=d, R=R, t=mu_g - R @ mu_s, mu_s=mu_s, mu_g=mu_g, m=m, rank=rank_exact(Hx),
                det_sign=int(np.sign(det_exact(Hx))))


def det_exact(M):
    return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])
            + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))


def rank_exact(M):
    M, r = [row[:] for row in M], 0
    for col in range(3):
        piv = next((i for i in range(r, 3) if M[i][col] != 0), None)
        if piv is None:
            continue
        M[r], M[piv] = M[piv], M[r]
        for i in range(r + 1, 3):
            f = M[i][col] / M[r][col]
            M[i] = [a - f * b for a, b in zip(M[i], M[r])]
        r += 1
    return r


def gap(ref):
    return float((ref["sig"][1] + ref["d"] * ref["sig"][2]) / ref["sig"][0]) if ref["sig"][0] > 0 else 0.0


def well_posed(c):
    """every determined case but the two narrow rungs of the ladder: gap >= 1e-3 (asserted)"""
    return determined(c) and c.get("want_gap", 1.0) >= 0.99e-3


def bar_R(ref, k=K):
    return k * U53 * (ref["m"] + ref["sig"][0]) / (ref["sig"][1] + ref["d"] * ref["sig"][2])


def bar_t(ref, k=K):
    return bar_R(ref, k) * (np.linalg.norm(ref["mu_s"]) + 1.0) + 2.0 ** -52 * np.linalg.norm(ref["mu_g"])


def determined(c):
    """the cases whose rotation the pairs determine (every case but the rank < 2 ones)"""
    return c["rank"] >= 2


def residual_exact(D, X, G):
    """S |R x' + t - g|^2 of a fit (the f64 entries of D taken as exact rationals), as a Fraction"""
    R, t = _fr(np.asarray(D)[:3, :3]), [Fraction(float(v)) for v in np.asarray(D)[:3, 3]]
    tot = Fraction(0)
    for p, q in zip(_fr(X), _fr(G)):
        for i in range(3):
            e = R[i][0] * p[0] + R[i][1] * p[1] + R[i][2] * p[2] + t[i] - q[i]
            tot += e * e
    return tot


def raw_moment_fit(X, G):
    """the second correct f64 algorithm the bar's K is calibrated with: raw moments in plain numpy f64, LAPACK"""
    v = sums(X, G)
    n, ms, mg = v[0], v[1:4] / v[0], v[4:7] / v[0]
    H = v[7:16].reshape(3, 3) - n * np.outer(ms, mg)
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    d = 1.0 if np.linalg.det(V @ U.T) >= 0 else -1.0
    R = V @ np.diag([1.0, 1.0, d]) @ U.T
    return R, mg - R @ ms


def calibrate():
    """-> (worst ratio of |R_raw - R_ref| to bar_R / K over the determined cases, its case): K is 8 x the ratio"""
    worst = (0.0, "")
    for c in fit_cases():
        if determined(c):
            R, _ = raw_moment_fit(c["X"], c["G"])
            ratio = np.linalg.norm(R - c["ref"]["R"]) / bar_R(c["ref"], 1.0)
            worst = max(worst, (float(ratio), c["name"]))
    return worst


def collinear_floor():
    """the largest sigma2 / sigma1, in units of 2^-53, the reference computation shows for exactly collinear pairs: 300
    seeded lines a distance class, points c + k d exactly representable in f32, spans of at least 1 m"""
    rng, worst = np.random.default_rng(0), 0.0
    for off in (0, 1, 10, 50, 100):
        for _ in range(300):
            n = int(rng.integers(3, 300))
            d = np.round(rng.uniform(-1, 1, 3) * 256) / 256
            k = rng.integers(-256, 256, n).astype(np.float64) / 16
            s = np.round(rng.uniform(-1, 1, 3) * off * 16) / 16 + k[:, None] * d
            g = s + np.round(rng.uniform(-1, 1, 3) * 64) / 64
            assert np.array_equal(s.astype(F).astype(np.float64), s) and np.array_equal(g.astype(F).astype(np.float64), g)
            if (k.max() - k.min()) * np.linalg.norm(d) < 1.0:
                continue
            v = sums(s.astype(F), g.astype(F))
            H = v[7:16].reshape(3, 3) - v[0] * np.outer(v[1:4] / v[0], v[4:7] / v[0])
            sig = np.linalg.svd(H)[1]
            worst = max(worst, float(sig[1] / sig[0] / U53))
    return worst


def numpy_round(c, T=None, mse_prev=lnp.DBL_MAX, iterations=0, **kw):
    """the numpy statement's round over the case's pairs (loop_icp_np.round_from_pairs)"""
    return lnp.round_from_pairs(c["X"], c["G"], sqd(c["X"], c["G"]), np.eye(4) if T is None else T, mse_prev, iterations, **kw)


# ---- stop_edges ----------------------------------------------------------------------------------------------------------
T_IN = np.array([[0.5, -0.75, 0.25, 3.0], [0.125, 0.5, -0.875, -1.5], [0.625, 0.25, 0.5, 0.75], [0.0, 0.0, 0.0, 1.0]])  # dyadic, generic
STOP_T = np.array([2.0 ** -10, 0.0, 0.0])   # the fitted translation: |t|^2 = 2^-20 exactly
STOP_T2 = 2.0 ** -20


def stop_sums(mse, n=8, t=STOP_T):
    """the sums of the cube's vertices (+-1, +-1, +-1) paired with themselves + t: S x' = 0, S g = n t, S x' g^T = 8 I — H = 8 I
    with every Jacobi gamma 0, so R = I and the fitted translation is t, exactly; sums[16] = n mse for a dyadic mse"""
    v = np.zeros(17)
    v[0], v[4:7], v[16] = n, n * np.asarray(t), n * mse
    v[[7, 11, 15]] = 8.0
    return v


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def stop_edges():
    """[(name, sums, params, incoming state, expected reason)]: mse = 1/4 after mse_prev = 1/2 — ad = 1/4, rel = 1/2, rot = 1,
    t2 = 2^-20, all exact — and every comparison of the rule at equality and one unit in the last place either side.
    `never`: the thresholds of the rules not under test put out of reach."""
    N, IT, TR, AB, RE, NC = lnp.NONE, lnp.ITERATIONS, lnp.TRANSFORM, lnp.ABS_MSE, lnp.REL_MSE, lnp.NO_CORRESPONDENCES
    st = dict(T=T_IN, mse_prev=0.5, mse=0.5, iterations=3)
    v = stop_sums(0.25)
    no_b, no_c, no_d = dict(rotation_threshold=2.0), dict(fitness_epsilon=0.0), dict(rel_mse=0.0)
    never = dict(no_b, **no_c, **no_d)
    out = [
        ("abs: ad == epsilon goes on", v, dict(never, fitness_epsilon=0.25), st, N),
        ("abs: epsilon one below ad goes on", v, dict(never, fitness_epsilon=down(0.25)), st, N),
        ("abs: epsilon one above ad stops", v, dict(never, fitness_epsilon=up(0.25)), st, AB),
        ("abs: ad one below epsilon stops", stop_sums(up(0.25)), dict(never, fitness_epsilon=0.25), st, AB),
        ("abs: ad one above epsilon goes on", stop_sums(down(0.25)), dict(never, fitness_epsilon=0.25), st, N),
        ("abs: a rising mse counts by its size", stop_sums(0.75), dict(never, fitness_epsilon=up(0.25)), st, AB),
        ("rel: rel == rel_mse goes on", v, dict(never, rel_mse=0.5), st, N),
        ("rel: rel_mse one below rel goes on", v, dict(never, rel_mse=down(0.5)), st, N),
        ("rel: rel_mse one above rel stops", v, dict(never, rel_mse=up(0.5)), st, RE),
        ("abs goes before rel", v, dict(no_b, fitness_epsilon=1.0, rel_mse=1.0), st, AB),
        ("transform: t2 == epsilon stops", v, dict(never, rotation_threshold=0.99999, transformation_epsilon=STOP_T2), st, TR),
        ("transform: t2 one above epsilon goes on", v, dict(never, rotation_threshold=0.99999, transformation_epsilon=down(STOP_T2)), st, N),
        ("transform: rot == threshold == 1 stops", v, dict(never, rotation_threshold=1.0, transformation_epsilon=STOP_T2), st, TR),
        ("transform: threshold one above rot goes on", v, dict(never, rotation_threshold=up(1.0), transformation_epsilon=STOP_T2), st, N),
        ("transform goes before abs and rel", v, dict(rotation_threshold=1.0, transformation_epsilon=1.0, fitness_epsilon=1.0, rel_mse=1.0), st, TR),
        ("iterations: k + 1 == max goes before every rule", v,
         dict(max_iterations=4, rotation_threshold=1.0, transformation_epsilon=1.0, fitness_epsilon=1.0, rel_mse=1.0), st, IT),
        ("iterations: k + 1 == max - 1 goes on", v, dict(never, max_iterations=5), st, N),
        ("too few: n == min - 1 keeps T", v, dict(min_correspondences=9, max_iterations=4), st, NC),
        ("too few: n == min fits", v, dict(never, min_correspondences=8), st, N),
        ("round 0: mse_prev = DBL_MAX fires neither mse rule", v, dict(no_b, fitness_epsilon=1e300, rel_mse=down(1.0)), dict(T=T_IN), N),
    ]
    return out


# ---- what both the CPU and the GPU test assert of a fit ----------------------------------------------------------------
def check_fit(c, st, label, prev=None):
    """a round-0 step of case c from T = I left the state st: the property checks and the reference within the case's bar;
    returns got / bar of R (0 where no bar applies)"""
    name, r, T = (label, c["name"]), c["ref"], st["T"]
    R, t = T[:3, :3], T[:3, 3]
    want = numpy_round(c)
    # (rank < 2: the numpy statement's rotation is arbitrary; the contract's identity with these cases' translations of more
    # than 0.1 m cannot fire the transform rule, and round 0 fires neither mse rule)
    reason = want["reason"] if determined(c) else lnp.NONE
    assert (st["iterations"], st["n_corr"], st["reason"]) == (1, want["n_corr"], reason), (name, st, reason)
    assert (st["converged"], st["active"]) == (int(reason != lnp.NONE), int(reason == lnp.NONE)), (name, st)
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]), name
    assert np.array_equal(st["move"], T[:3].astype(F)), name
    assert st["mse"] == c["sums"][16] / c["sums"][0] == st["mse_prev"], name
    ortho = np.abs(R.T @ R - np.eye(3)).max()
    assert ortho <= ORTHO and np.linalg.det(R) > 0, (name, ortho, np.linalg.det(R))
    if c["identity"]:
        assert np.array_equal(R, np.eye(3)), (name, R)
    if not determined(c):
        lim = 2.0 ** -52 * (np.linalg.norm(r["mu_g"]) + np.linalg.norm(r["mu_s"]))
        assert np.linalg.norm(t - (r["mu_g"] - r["mu_s"])) <= lim, name
        return 0.0, ortho
    if c["exact"]:
        assert np.array_equal(R, r["R"]) and np.array_equal(t, r["t"]), name
    eR, et = np.linalg.norm(R - r["R"]), np.linalg.norm(t - r["t"])
    assert eR <= bar_R(r) and et <= bar_t(r), (name, eR, bar_R(r), et, bar_t(r))
    return eR / bar_R(r), ortho


def check_stop_edge(edge, st, label):
    """the state a stop_edges entry must leave, exactly"""
    name, v, kw, st_in, reason = edge
    tag, T_in = (label, name), np.asarray(st_in["T"], np.float64)
    it_in, prev_in = st_in.get("iterations", 0), st_in.get("mse_prev", lnp.DBL_MAX)
    assert st["reason"] == reason and st["n_corr"] == 8, (tag, st)
    if reason == lnp.NO_CORRESPONDENCES:
        assert (st["iterations"], st["converged"], st["active"]) == (it_in, 0, 0), (tag, st)
        assert st["T"].tobytes() == T_in.tobytes() and st["mse_prev"] == prev_in, tag
        return
    D = np.eye(4)
    D[:3, 3] = STOP_T
    assert st["T"].tobytes() == (D @ T_in).tobytes(), (tag, st["T"])  # (dyadic entries: the product is exact in any order)
    assert np.array_equal(st["move"], st["T"][:3].astype(F)), tag
    assert (st["iterations"], st["converged"], st["active"]) == (it_in + 1, int(reason != lnp.NONE), int(reason == lnp.NONE)), (tag, st)
    assert st["mse"] == v[16] / 8 == st["mse_prev"], (tag, st)
