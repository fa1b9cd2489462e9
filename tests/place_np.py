"""An independent numpy statement of place recognition (DESIGN.md §5.3 "Place recognition"), f64 throughout, np.arctan2
for the azimuth, nothing shared with csrc/host/place_math.h.  The one f32 operation is the height h = p[up] + lift: the
descriptor STORES it, so it is formed as the contract forms it (one f32 add)."""
import numpy as np

NR, NS = 20, 60
FLOOR = 2.0 ** -10


def descriptor(points, r_max=80.0, lift=2.0, up=1):
    """points: (n, >= 3) -> D[ring][sector], f32 (the stored heights), cells decided in f64"""
    D = np.zeros((NR, NS), np.float32)
    p = np.asarray(points, np.float32).reshape(-1, np.shape(points)[-1] if np.size(points) else 4)
    if len(p) == 0:
        return D
    a, b = (up + 1) % 3, (up + 2) % 3
    h = p[:, up] + np.float32(lift)
    pa, pb = p[:, a].astype(np.float64), p[:, b].astype(np.float64)
    rho = np.hypot(pa, pb)
    ok = (rho < r_max) & (h >= np.float32(FLOOR))
    ring = np.minimum(NR - 1, np.floor(rho * NR / r_max)).astype(int)
    sec = np.minimum(NS - 1, np.floor((np.arctan2(pb, pa) + np.pi) * NS / (2 * np.pi))).astype(int)
    for i in np.nonzero(ok)[0]:
        D[ring[i], sec[i]] = max(D[ring[i], sec[i]], h[i])
    return D


def distances(Dq, Dc):
    """d[k] for k < 60, f64"""
    Dq, Dc = np.asarray(Dq, np.float64).reshape(NR, NS), np.asarray(Dc, np.float64).reshape(NR, NS)
    nq, nc = np.sqrt((Dq * Dq).sum(0)), np.sqrt((Dc * Dc).sum(0))
    Uq = np.divide(Dq, nq, out=np.zeros_like(Dq), where=nq > 0)
    Uc = np.divide(Dc, nc, out=np.zeros_like(Dc), where=nc > 0)
    G = Uq.T @ Uc  # G[j][jc]
    j = np.arange(NS)
    d = np.ones(NS)
    for k in range(NS):
        jc = (j + k) % NS
        both = (nq > 0) & (nc[jc] > 0)
        if both.any():
            d[k] = max(0.0, 1.0 - G[j, jc][both].sum() / both.sum())
    return d


def search(Dq, descs, times, now, gap, skip_id=-1):
    """-> (id, shift, d, candidates, runner_up_d): the minimum of (d, id, shift); runner_up_d: the smallest d of any
    OTHER admissible candidate (inf without one)"""
    rows = []
    for c, Dc in enumerate(descs):
        if c == skip_id or not (abs(times[c] - now) > gap):
            continue
        d = distances(Dq, Dc)
        k = int(np.argmin(d))
        rows.append((d[k], c, k))
    if not rows:
        return -1, 0, 1.0, 0, np.inf
    rows.sort()
    return rows[0][1], rows[0][2], rows[0][0], len(rows), (rows[1][0] if len(rows) > 1 else np.inf)
