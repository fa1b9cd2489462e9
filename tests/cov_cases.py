"""Built priors and information matrices for the covariance update of the iterated update (SE:594-598) alone, a plain
reference of it and the error model every update path is held to (tests/test_cov_inputs.py, tests/test_gpu_cov_update.py).

A case is (P, sums, r2, diverged) with what it claims:
  P      the prior, D Corr D with Corr built from fixed loadings (corr()): exactly symmetric, every block correlated with
         every other unless the case says otherwise;
  H      m x 18, non-zero in the columns S = {0, 1, 2, 6, 7, 8} only: rows (n, p x n) of built planes with normal n
         through points p at a stated range, weighted, and put on a fixed-point grid of 24 bits so that A = H^T H — the
         21 sums the kernels read, upper triangle row by row — is EXACT in f64: reference (from H) and kernels (from the
         sums) see the same information, to the bit;
  r2     sigma^2 = lidar_std * lidar_std.

The reference (reference()) is the textbook form,  K = P H^T (H P H^T + sigma^2 I)^-1,  P+ = sym((I - K H) P (I - K H)^T
+ sigma^2 K K^T),  in np.longdouble (64-bit significand), the m x m system by Cholesky: written from the two equations,
nothing of csrc/ or of the oracle.  The same function in f64 must agree with it to 8 eps (tests/test_cov_inputs.py).

Metric: e = max_ij |got_ij - ref_ij| / sqrt(ref_ii ref_jj); rows and columns of zero reference variance must be equal.
Error model: with shrink = min over the observed states i of P+_ii / P_ii (states of zero prior variance left out), a
form that reaches the posterior by subtracting quantities of the prior's size — the rank-6 form of joseph_epilogue —
has e of order eps / shrink, eps = 2^-52.  rank6_f64() is that form in plain numpy; on these cases its e is at most
RANK6_C x eps / shrink (the measured constant is in test_cov_inputs.py's output), and the kernels are given
bar(shrink) = 16 eps / shrink + 16 eps."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
S = np.array([0, 1, 2, 6, 7, 8])
LIDAR_STD = 0.01  # exp_port.yaml
PATHS_DEVICE = ("lds", "lds1", "mr", "joseph")


def bar(shrink):
    return 16 * EPS / shrink + 16 * EPS


# ---- priors -------------------------------------------------------------------------------------------------------------
def loadings(cross=0.35):
    """18 x 4 fixed loadings: generic, no two rows alike"""
    i, f = np.arange(18.0)[:, None], np.arange(4.0)[None, :]
    return cross * np.cos(0.7 * (i + 1) * (f + 1) + 0.3 * f)


def corr(W, B=None):
    """the correlation matrix of W W^T + B (B: identity), exactly symmetric with a unit diagonal"""
    C = W @ W.T + (np.eye(18) if B is None else B)
    s = 1.0 / np.sqrt(np.diag(C))
    C = np.triu(C * s[:, None] * s[None, :], 1)
    return C + C.T + np.eye(18)


def prior(std, C):
    """D Corr D: (d_i d_j) c_ij, the same product either side of the diagonal; no negative zeros"""
    d = np.repeat(np.asarray(std, np.float64), 3) if len(std) == 6 else np.asarray(std, np.float64)
    P = (d[:, None] * d[None, :]) * C + 0.0
    assert np.array_equal(P, P.T)
    return P


def corr_uncorrelated_gyro_bias():
    """the gyro bias block (12:15) loads on the last factor only, the observed states not at all: exactly uncorrelated with S,
    correlated with velocity, accelerometer bias and gravity — which are correlated with S"""
    W = loadings()
    W[12:15, :3] = 0.0
    W[S, 3] = 0.0
    return corr(W)


def corr_pairs(rho):
    """S-S correlations of +rho (x, roll), -rho (y, pitch), +rho (z, yaw) and small generic ones to everything else: the
    paired states share their loadings up to the sign, the pair term makes the normalised correlation rho"""
    W = loadings(0.05)
    B = np.eye(18)
    for a, (i, j) in enumerate(((0, 6), (1, 7), (2, 8))):
        sg = -1.0 if a == 1 else 1.0
        W[j] = sg * W[i]
        w2 = W[i] @ W[i]
        B[i, j] = B[j, i] = sg * (rho * (1 + w2) - w2)
    return corr(W, B)


# ---- information --------------------------------------------------------------------------------------------------------
def plane_rows(m, rng_m, shift=0.0):
    """m rows (n, p x n): normals on a golden-angle spiral over the sphere, points at range rng_m in other directions"""
    k = np.arange(m) + shift
    az, el = 2.399963 * k, np.arcsin(-0.8 + 1.6 * (k - shift + 0.5) / m)
    n = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    az2, el2 = az + 1.3, 0.3 * np.cos(k)
    p = rng_m * np.stack([np.cos(el2) * np.cos(az2), np.cos(el2) * np.sin(az2), np.sin(el2)], 1)
    return np.concatenate([n, np.cross(p, n)], 1)


def on_grid(H6):
    """every entry a multiple of one power of two, 24 bits below the largest: products and sums of <= 16 of them are exact"""
    top = np.abs(H6).max()
    if top == 0:
        return H6
    g = 2.0 ** (np.ceil(np.log2(top)) - 24)
    return np.round(H6 / g) * g


def H18_of(H6):
    H6 = on_grid(np.atleast_2d(np.asarray(H6, np.float64)))
    assert len(H6) <= 16
    H = np.zeros((len(H6), 18))
    H[:, S] = H6
    return H


def information(A_size, m=6, rng_m=30.0):
    """m planes at rng_m, weighted so that the largest entry of A is about A_size (2000 features at 30 m: 2e6)"""
    R = plane_rows(m, rng_m)
    return H18_of(R * np.sqrt(A_size / np.abs(R.T @ R).max()))


def sums_of(H):
    A = H[:, S].T @ H[:, S]
    return A[np.triu_indices(6)].copy()  # (row-major upper triangle: tri6 of csrc/ieskf_device.h)


def A_of(sums):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums
    return A + np.triu(A, 1).T


# ---- the model ------------------------------------------------------------------------------------------------------------
def chol_solve(M, B):
    """M^-1 B for a symmetric positive definite M, in M's dtype"""
    n = len(M)
    L = np.zeros_like(M)
    for j in range(n):
        L[j, j] = np.sqrt(M[j, j] - L[j, :j] @ L[j, :j])
        for i in range(j + 1, n):
            L[i, j] = (M[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    X = B.copy()
    for i in range(n):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def reference(P, H, r2, dtype=LD):
    """the textbook Joseph form (see the module's text)"""
    P, H, r2 = np.asarray(P, dtype), np.asarray(H, dtype), dtype(r2)
    K = chol_solve(H @ P @ H.T + r2 * np.eye(len(H), dtype=dtype), H @ P).T
    IKH = np.eye(18, dtype=dtype) - K @ H
    O = IKH @ P @ IKH.T + r2 * (K @ K.T)
    return (O + O.T) / dtype(2)


def rank6_f64(P, sums, r2):
    """the expanded rank-6 form of joseph_epilogue's header in plain numpy f64"""
    A, C, R, PSS = A_of(sums), P[:, S], P[S, :], P[np.ix_(S, S)]
    N = r2 * np.eye(6) + A @ PSS
    Y = np.linalg.solve(N, A)
    Z = np.linalg.solve(N, Y.T).T
    O = P - C @ Y @ R - C @ Y.T @ C.T + C @ (Y @ PSS @ Y.T + r2 * Z) @ C.T
    return 0.5 * (O + O.T)


def err(got, ref):
    """e of the module's text (inf where a row of zero reference variance is not reproduced exactly)"""
    ref = np.asarray(ref, LD)
    d = np.diag(ref)
    z = d == 0
    if z.any() and not (np.array_equal(np.asarray(got)[z], ref[z].astype(np.float64)) and np.array_equal(np.asarray(got)[:, z], ref[:, z].astype(np.float64))):
        return np.inf
    s = np.sqrt(np.where(z, LD(1), d))
    e = np.abs(np.asarray(got, LD) - ref) / (s[:, None] * s[None, :])
    return float(e[np.ix_(~z, ~z)].max()) if (~z).any() else 0.0


def diff(a, b, ref):
    """max |a_ij - b_ij| / sqrt(ref_ii ref_jj) over the rows of non-zero reference variance"""
    d = np.diag(np.asarray(ref, np.float64))
    k = d > 0
    if not k.any():
        return 0.0
    s = np.sqrt(d[k])
    return float((np.abs(np.asarray(a) - np.asarray(b))[np.ix_(k, k)] / np.outer(s, s)).max())


def shrink_of(P, ref):
    i = S[np.diag(P)[S] > 0]
    return float((np.diag(ref)[i] / np.diag(P).astype(LD)[i]).min()) if len(i) else 1.0


def min_eig_corr(M, ref):
    """smallest eigenvalue of M in the correlation scaling of ref (rows of zero reference variance left out)"""
    d = np.diag(np.asarray(ref, np.float64))
    k = d > 0
    if not k.any():
        return 1.0
    s = 1.0 / np.sqrt(d[k])
    return float(np.linalg.eigvalsh(np.asarray(M, np.float64)[np.ix_(k, k)] * s[:, None] * s[None, :]).min())


def pivot_order(P, sums, r2):
    """the rows partial pivoting (largest magnitude in the column, the first of equals, rows exchanged) picks in N =
    sigma^2 I + A P_SS, as positions at the time of the pick; and whether a pick had an equal rival"""
    N = r2 * np.eye(6) + A_of(sums) @ P[np.ix_(S, S)]
    order, tie = [], False
    for k in range(6):
        col = np.abs(N[k:, k])
        p = k + int(np.argmax(col))
        tie = tie or int((col == col.max()).sum()) > 1
        order.append(p)
        N[[k, p]] = N[[p, k]]
        N[k + 1:] -= np.outer(N[k + 1:, k] / N[k, k], N[k])
    return order, tie


# ---- the cases ------------------------------------------------------------------------------------------------------------
STD = (0.01, 0.1, 0.01, 1e-3, 1e-4, 0.05)  # position, velocity, attitude, accelerometer bias, gyro bias, gravity


def case(name, P, H, lidar_std=LIDAR_STD, diverged=0, **claims):
    c = dict(name=name, P=P, H=H, sums=sums_of(H), r2=lidar_std * lidar_std, lidar_std=lidar_std, diverged=diverged,
             shrink_target=None, rank=None, pivot=None, tie=False, returns_prior=False, kept_rows=None, zero_rows=(), rho=None)
    c.update(claims)
    return c


def scaled_prior(s_obs):
    """STD with the observed blocks' standard deviations multiplied by s_obs"""
    std = list(STD)
    std[0], std[2] = std[0] * s_obs, std[2] * s_obs
    return prior(std, corr(loadings()))


LADDER = [10.0 ** -k for k in range(2, 11)]
PRIOR_TRIM = 1.4  # (the built planes' A and the correlated prior give sigma^2 / (|A| var) x 1.1 .. 1.42 untrimmed)
A_PRIOR_LADDER = 1e4


def shrink_ladder():
    """shrink 1e-2 .. 1e-10, each by the prior's scale at one A (|A| = 1e4) and by |A| at one of two priors; r2 = lidar_std^2
    and, at 1e-6, another.  shrink is about sigma^2 / (|A| var(attitude)): the rotation columns carry |A|."""
    out = []
    for t in LADDER:
        var = LIDAR_STD ** 2 / (A_PRIOR_LADDER * t) * PRIOR_TRIM
        out.append(case(f"ladder/prior/{t:.0e}", scaled_prior(np.sqrt(var) / STD[2]), information(A_PRIOR_LADDER), shrink_target=t))
    for t in LADDER:
        s_obs = 1.0 if t >= 1e-5 else 100.0  # attitude std 0.01 or 1
        a = LIDAR_STD ** 2 / ((STD[2] * s_obs) ** 2 * t) * PRIOR_TRIM
        out.append(case(f"ladder/info/{t:.0e}", scaled_prior(s_obs), information(a), shrink_target=t, A_size=a))
    a = 0.05 ** 2 / (1.0 * 1e-6) * PRIOR_TRIM
    out.append(case("ladder/r2/1e-06", scaled_prior(100.0), information(a), lidar_std=0.05, shrink_target=1e-6, A_size=a))
    return out


def block_scales():
    """standard deviations over eight decades, block by block; every block correlated with S — and the variant whose gyro
    bias block is exactly uncorrelated with S: its rows and columns are the prior's, bit for bit"""
    std = (1.0, 10.0, 0.1, 1e-4, 1e-7, 1e-2)
    H = information(1e4)
    return [case("blocks/all_correlated", prior(std, corr(loadings())), H),
            case("blocks/gyro_bias_uncorrelated", prior(std, corr_uncorrelated_gyro_bias()), H, kept_rows=(12, 13, 14))]


def zero_blocks():
    """the state after reset: zero position and attitude variance (rows and columns zero), one of them, the other"""
    C, H, out = corr(loadings()), information(1e4), []
    for name, z in (("both", (0, 2)), ("position", (0,)), ("attitude", (2,))):
        std = list(STD)
        for b in z:
            std[b] = 0.0
        rows = tuple(int(r) for b in z for r in range(3 * b, 3 * b + 3))
        out.append(case(f"zero/{name}", prior(std, C), H, zero_rows=rows, returns_prior=name == "both"))
    return out


def rank_deficient():
    """A of rank 1, 3 (three planes: a corridor's floor and walls), 5 and A = 0"""
    P, R = prior(STD, corr(loadings())), plane_rows(12, 30.0) * 20.0
    R[0] = (0, 0, 400.0, 0, 0, 0)  # rank 1: the ground plane straight below (p x n = 0) — z alone is observed
    out = [case(f"rank/{r}", P, H18_of(R[:r] if r == 1 else R[1:r + 1]), rank=r) for r in (1, 3, 5)]
    out.append(case("rank/0", P, np.zeros((1, 18)), rank=0, returns_prior=True))
    return out


def pivoting():
    """S-S correlations of +-0.999: the largest entry of N's column k lies below row k — at k = 0 (the rotation rows carry
    |A|), at a later k only (information on x above everything else), and with two equal candidates (dyadic A and P_SS)"""
    C = corr_pairs(0.999)
    P = prior(STD, C)
    out = [case("pivot/k0", P, information(30.0, rng_m=5.0), pivot="k0", rho=0.999)]
    # x observed far above everything else, pitch three times as well as y: N's row 0 leads column 0, then -0.999 puts row 4 above row 1
    H6 = np.diag(np.sqrt([20.0, 1.0, 1.0, 1.0, 3.0, 1.0])) + 0.05 * plane_rows(6, 1.0)
    out.append(case("pivot/later", P, H18_of(H6), pivot="later", rho=0.999))
    # two equal candidates in column 0: rows 3 and 4 of A mirror each other, P_SS has equal covariances of x with roll and pitch
    H6 = np.array([[1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 8, 2, 0], [0, 0, 0, 2, 8, 0], [0, 0, 0, 0, 0, 4], [1, 0, 0, 4, 4, 0]], np.float64)
    Ct = np.eye(18)
    for i, j, v in ((0, 6, 0.5), (0, 7, 0.5), (6, 7, 0.25), (3, 0, 0.25), (9, 6, 0.25), (12, 7, -0.25), (15, 8, 0.5)):
        Ct[i, j] = Ct[j, i] = v
    out.append(case("pivot/tie", prior((0.25, 0.5, 0.25, 2.0 ** -6, 2.0 ** -10, 2.0 ** -3), Ct), H18_of(H6), pivot="k0", tie=True))
    return out


def diverged():
    """a diverged update keeps its prior, bit for bit — whatever the prior holds"""
    P = prior(STD, corr(loadings()))
    Pn = P.copy()
    Pn[4, 11] = np.nan
    Pn[17, 0] = -np.inf
    return [case("diverged/plain", P, information(1e4), diverged=1, returns_prior=True),
            case("diverged/nan", Pn, information(1e4), diverged=1, returns_prior=True)]


_CASES = None


def cases():
    """every case, with its reference, shrink, bar and the reference's smallest eigenvalue in correlation form (computed once)"""
    global _CASES
    if _CASES is None:
        _CASES = shrink_ladder() + block_scales() + zero_blocks() + rank_deficient() + pivoting() + diverged()
        for c in _CASES:
            if c["diverged"]:
                c.update(ref=None, shrink=1.0, bar=0.0, min_eig=None)
                continue
            ref = reference(c["P"], c["H"], c["r2"])
            sh = shrink_of(c["P"], ref)
            c.update(ref=ref, shrink=sh, bar=bar(sh), min_eig=min_eig_corr(ref, ref))
        assert len({c["name"] for c in _CASES}) == len(_CASES)
    return _CASES


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def batch(cs):
    return np.stack([c["P"] for c in cs]), np.stack([c["sums"] for c in cs]), np.array([c["diverged"] for c in cs], np.int32)


def check_output(c, got, who):
    """everything a path's output is held to for case c -> its e (None for a diverged case)"""
    if c["diverged"]:
        assert got.tobytes() == c["P"].tobytes(), (c["name"], who, "a diverged update's prior is passed through bit for bit")
        return None
    assert np.isfinite(got).all(), (c["name"], who)
    assert np.array_equal(got, got.T), (c["name"], who, "not exactly symmetric")
    e = err(got, c["ref"])
    assert e <= c["bar"], (c["name"], who, f"e = {e:.3e} > bar = {c['bar']:.3e} (shrink {c['shrink']:.3e})")
    lam = min_eig_corr(got, c["ref"])
    assert lam >= c["min_eig"] - 18 * c["bar"], (c["name"], who, lam, c["min_eig"])
    if c["returns_prior"]:
        assert np.array_equal(got, c["P"]), (c["name"], who, "the prior must come back exactly")
    if c["kept_rows"]:
        k = list(c["kept_rows"])
        assert np.array_equal(got[k], c["P"][k]) and np.array_equal(got[:, k], c["P"][:, k]), (c["name"], who, "the uncorrelated block moved")
    if c["zero_rows"]:
        z = list(c["zero_rows"])
        assert not got[z].any() and not got[:, z].any(), (c["name"], who, "a zero-variance row is not zero")
    return e
