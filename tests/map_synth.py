"""Synthetic scan-to-map problems (planes + line features) for the scan-to-map row's tests."""
import numpy as np

# the project's bar on a device scan-to-map transform against the CPU oracle's: the 27 sums are f64 on both sides, added
# in another order (tests/test_gpu_map.py, tests/test_gpu_map_rounds.py, tests/test_gpu_ref_mapnode.py)
SCAN2MAP_BAR = 2e-5


def rot(rx, ry, rz):
    """pointAssociateToMap's rotation (LM:594-607): rotate about z, then x, then y."""
    cz, sz, cx, sx, cy, sy = np.cos(rz), np.sin(rz), np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return Ry @ Rx @ Rz


def make_problem(defs, seed, n_map_surf=20000, n_map_corner=3000, n_scan_surf=900, n_scan_corner=250, noise=0.01,
                 perturb=(0.01, 0.05)):
    rng = np.random.default_rng(seed)
    # a room: floor, ceiling-less, four walls (surf); vertical and horizontal edges (corner)
    def plane(n, origin, u, v):
        a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
        return origin + a[:, None] * u + b[:, None] * v
    L, W, H = 30.0, 20.0, 6.0
    o = np.array([-L / 2, -W / 2, -1.5])
    ex, ey, ez = np.array([L, 0, 0.0]), np.array([0, W, 0.0]), np.array([0, 0, H])
    parts = [plane(n_map_surf // 5, o, ex, ey), plane(n_map_surf // 5, o, ex, ez), plane(n_map_surf // 5, o + ey, ex, ez),
             plane(n_map_surf // 5, o, ey, ez), plane(n_map_surf - 4 * (n_map_surf // 5), o + ex, ey, ez)]
    map_surf = np.concatenate(parts) + rng.normal(0, noise, (n_map_surf, 3))
    edges = []
    corners = [o, o + ex, o + ey, o + ex + ey]
    per = n_map_corner // 8
    for c0 in corners:
        edges.append(c0 + rng.uniform(0, 1, per)[:, None] * ez)
    for a, d in ((o, ex), (o + ey, ex), (o, ey), (o + ex, ey)):
        edges.append(a + rng.uniform(0, 1, per)[:, None] * d)
    map_corner = np.concatenate(edges) + rng.normal(0, noise / 2, (8 * per, 3))
    # true transform (sensor -> map) and the scan = map points seen from the sensor frame
    T_true = np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.5, 3)])
    R = rot(*T_true[:3])
    def to_sensor(pm):
        return (pm - T_true[3:]) @ R  # R^T (p - t)
    ss = to_sensor(map_surf[rng.choice(n_map_surf, n_scan_surf, replace=False)]) + rng.normal(0, noise, (n_scan_surf, 3))
    sc = to_sensor(map_corner[rng.choice(len(map_corner), n_scan_corner, replace=False)]) + rng.normal(0, noise, (n_scan_corner, 3))
    T0 = T_true + np.concatenate([rng.normal(0, perturb[0], 3), rng.normal(0, perturb[1], 3)])
    pad = lambda a: np.concatenate([a, np.zeros((len(a), 1))], 1).astype(np.float32)
    return defs.MapProblem(pad(map_corner), pad(map_surf), pad(sc), pad(ss), T0.astype(np.float32)), T_true


def make_corridor(defs, seed, n_map_surf=12000, n_map_corner=1500, n_scan_surf=900, n_scan_corner=200, noise=0.01):
    """A corridor along x: floor and two side walls, edges along x only — nothing constrains the translation along
    x, so LMOptimization's eigen-test must flag the problem as degenerate (LM:1589-1614)."""
    rng = np.random.default_rng(seed)
    L, W, H = 40.0, 4.0, 3.0
    n3 = n_map_surf // 3
    floor = np.stack([rng.uniform(-L / 2, L / 2, n3), rng.uniform(-W / 2, W / 2, n3), np.full(n3, -1.5)], 1)
    wl = np.stack([rng.uniform(-L / 2, L / 2, n3), np.full(n3, -W / 2), rng.uniform(-1.5, -1.5 + H, n3)], 1)
    n_r = n_map_surf - 2 * n3
    wr = np.stack([rng.uniform(-L / 2, L / 2, n_r), np.full(n_r, W / 2), rng.uniform(-1.5, -1.5 + H, n_r)], 1)
    map_surf = np.concatenate([floor, wl, wr]) + rng.normal(0, noise, (n_map_surf, 3))
    per = n_map_corner // 4
    edges = [np.stack([rng.uniform(-L / 2, L / 2, per), np.full(per, y), np.full(per, z)], 1)
             for y in (-W / 2, W / 2) for z in (-1.5, -1.5 + H)]
    map_corner = np.concatenate(edges) + rng.normal(0, noise / 2, (4 * per, 3))
    T_true = np.concatenate([rng.normal(0, 0.02, 3), rng.normal(0, 0.2, 3)])
    R = rot(*T_true[:3])
    to_sensor = lambda pm: (pm - T_true[3:]) @ R
    near = lambda a: a[np.abs(a[:, 0]) < L / 2 - 3]  # keep the scan away from the corridor's open ends
    ms, mc = near(map_surf), near(map_corner)
    ss = to_sensor(ms[rng.choice(len(ms), n_scan_surf, replace=False)]) + rng.normal(0, noise, (n_scan_surf, 3))
    sc = to_sensor(mc[rng.choice(len(mc), n_scan_corner, replace=False)]) + rng.normal(0, noise, (n_scan_corner, 3))
    T0 = T_true + np.concatenate([rng.normal(0, 0.005, 3), rng.normal(0, 0.03, 3)])
    pad = lambda a: np.concatenate([a, np.zeros((len(a), 1))], 1).astype(np.float32)
    return defs.MapProblem(pad(map_corner), pad(map_surf), pad(sc), pad(ss), T0.astype(np.float32)), T_true


# ---- problems of tests/test_gpu_map_rounds.py (their conditions are asserted on the CPU oracle by tests/test_map_rounds_inputs.py) ----
def pad4(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    return np.concatenate([a, np.zeros((len(a), 1))], 1).astype(np.float32)


def rounds_problems(defs):
    """name -> problem: what the round-by-round parity runs on.  The six rooms and the corridor of test_gpu_map.py; `quick`
    starts next to its answer (converges within three rounds); `slow` takes seven rounds; `far` and `far2` start far off
    in a noisy room and run all ten rounds, degenerate, on the projection carried from round 0 (`far` never converges,
    `far2` does in its last round); `floor` and `floor50` sit just above LMOptimization's floor of 50 rows (50-60
    selected in every round, `floor50` with exactly 50 in its first) beside `below49` and `few` just below it (ten
    rounds without a step)."""
    big = dict(n_map_surf=8000, n_map_corner=1200, n_scan_surf=600, n_scan_corner=150)
    thin = dict(n_map_surf=2000, n_map_corner=200)
    out = {"room%d" % k: make_problem(defs, 30 + k)[0] for k in range(6)}
    out["corridor"] = make_corridor(defs, 50)[0]
    out["quick"] = make_problem(defs, 36, perturb=(1e-5, 1e-4))[0]
    out["slow"] = make_problem(defs, 38, noise=0.06, perturb=(0.04, 0.25), **big)[0]
    out["far"] = make_problem(defs, 39, noise=0.06, perturb=(0.08, 0.5), **big)[0]
    out["far2"] = make_problem(defs, 37, noise=0.03, perturb=(0.08, 0.5), **big)[0]
    out["floor"] = make_problem(defs, 43, n_scan_surf=54, n_scan_corner=16, **thin)[0]
    out["floor50"] = make_problem(defs, 43, n_scan_surf=52, n_scan_corner=14, **thin)[0]
    out["below49"] = make_problem(defs, 46, n_scan_surf=54, n_scan_corner=16, **thin)[0]
    out["few"] = make_problem(defs, 41, n_scan_surf=30, n_scan_corner=10, **thin)[0]
    return out


# kinds of the batch pool: how a problem loads the correspondence kernel's (problem, block) grid
POOL_KINDS = ("large", "empty", "inactive", "quick", "small", "medium", "few")


def batch_pool(defs):
    """kind -> problem, very uneven: `large` several thousand queries (sets the batch's blocks per problem), `empty` an
    active map without a single query, `inactive` below the precondition of LM:1636, `quick` converges early, `small`
    and `medium` ordinary rooms of a few blocks, `few` ten rounds without a step."""
    e = np.zeros((0, 4), np.float32)
    base = make_problem(defs, 81, n_map_surf=6000, n_map_corner=900, n_scan_surf=100, n_scan_corner=30)[0]
    return {
        "large": make_problem(defs, 80, n_map_surf=9000, n_map_corner=1500, n_scan_surf=3000, n_scan_corner=700)[0],
        "empty": defs.MapProblem(base.map_corner, base.map_surf, e, e, base.transform),
        "inactive": make_problem(defs, 42, n_map_surf=90, n_map_corner=40, n_scan_surf=60, n_scan_corner=20)[0],
        "quick": make_problem(defs, 82, n_map_surf=6000, n_map_corner=900, n_scan_surf=500, n_scan_corner=150, perturb=(1e-5, 1e-4))[0],
        "small": base,
        "medium": make_problem(defs, 83, n_map_surf=8000, n_map_corner=1200, n_scan_surf=800, n_scan_corner=200)[0],
        "few": make_problem(defs, 41, n_map_surf=2000, n_map_corner=200, n_scan_surf=30, n_scan_corner=10)[0],
    }


BATCH_SIZES = (1, 7, 8, 9, 16, 19, 33)


def batch_orders():
    """two orders of the pool: order -> [kinds of batch b for b in BATCH_SIZES].  Seven kinds against groups of eight:
    the walks below put every kind at every position of a group of eight somewhere (asserted on the CPU)."""
    K = len(POOL_KINDS)
    first = [[POOL_KINDS[(i + b + 1) % K] for i in range(n)] for b, n in enumerate(BATCH_SIZES)]
    second = [[POOL_KINDS[(3 * i + 5 * b + 4) % K] for i in range(n)] for b, n in enumerate(BATCH_SIZES)]
    return {"first": first, "second": second}


def _with_transform(defs, mc, ms, tc, ts, T):
    """problem whose ASSOCIATED corner / surf query points are (up to f32 rounding) tc / ts under transform T"""
    T = np.asarray(T, dtype=np.float64)
    R = rot(*T[:3])
    inv = lambda p: (np.asarray(p, dtype=np.float64).reshape(-1, 3) - T[3:]) @ R
    return defs.MapProblem(pad4(mc), pad4(ms), pad4(inv(tc)), pad4(inv(ts)), T.astype(np.float32))


LATTICE_T = (0.03, -0.02, 0.4, 1.25, -0.75, 0.5)  # the non-trivial transform of every lattice case


def lattice_cases(defs, transform=None):
    """name -> (problem, claims): hand-built maps and queries at the edges of the 27-cell search.  The same cloud serves
    as corner and as surf map, the same points as corner and surf queries.  transform None: identity — the associated
    points are the listed targets exactly; else the queries are the targets moved back through `transform`, so that the
    associated points are the targets up to rounding.  claims: what tests/test_map_rounds_inputs.py asserts from the
    oracle's records about the case (see there)."""
    rng = np.random.default_rng(2024)
    T = np.zeros(6) if transform is None else np.asarray(transform, dtype=np.float64)
    cases = {}

    def add(name, m, q, **claims):
        cases[name] = (_with_transform(defs, m, m, q, q, T), claims)

    g = np.arange(-3, 3.5, 0.5)
    half = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    qi = np.stack(np.meshgrid(*[np.arange(-2, 3.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    # half-metre lattice, queries on integer coordinates: every distance is tied many times over
    add("integer_half_lattice", half, qi, on_integers=True, min_found=len(qi))
    # unit lattice: a query on a lattice point has itself and six neighbours at squared distance exactly 1
    unit = half[(np.abs(half - np.round(half)) < 1e-9).all(1)]
    add("integer_unit_lattice", unit, qi, on_integers=True, fifth_exactly_one=len(qi))
    # fifth neighbour at exactly 1.0f (rejected) and at the float below (accepted): four near points and one along +x
    m, q = [], []
    for k, just_below in enumerate((False, True, False, True)):
        if just_below:
            # query on x = 0: dx = 1 - 2^-24 and dy = 2^-12 are exact, dx^2 rounds to 1 - 2^-23, + dy^2 = 1 - 2^-24 exactly
            c = np.array([0.0, 4.0 * k, 0.0])
            p5 = c + [1.0 - 2.0 ** -24, 2.0 ** -12, 0.0]
        else:
            c = np.array([8.0 * k - 12.0, 0.25 * k, -0.5 * k]) + 0.25  # (multiples of 1/4: exact in f32 at these magnitudes)
            p5 = c + [1.0, 0.0, 0.0]
        m += [c + [0.125, 0, 0], c + [0, 0.125, 0], c + [0, 0, 0.125], c + [-0.125, 0.125, 0], p5]
        q.append(c)
    add("fifth_at_one", np.array(m), np.array(q), fifth_exactly_one=2, fifth_just_below_one=2)
    # the five neighbours in five different cells, corner cells of the 3 x 3 x 3 block among them
    m, q = [], []
    for k in range(4):
        o = np.array([6.0 * k - 9.0, 2.0 * k, -3.0 * k])
        q.append(o + 0.5)
        for s in ((-1, -1, -1), (1, 1, 1), (-1, 1, -1), (1, -1, 1), (1, 1, -1)):
            m.append(o + 0.5 + 0.55 * np.array(s) + rng.uniform(-0.01, 0.01, 3))
    add("corner_cells", np.array(m), np.array(q), spread_over_corner_cells=4)
    # queries one and two cells outside the box on each side of each axis, over a dense box [0, 4)^3
    dense = rng.uniform(0.02, 3.98, (4000, 3))
    q = []
    for a in range(3):
        for v in (-1.6, -0.35, 4.35, 5.6):
            p = rng.uniform(0.5, 3.5, (6, 3))
            p[:, a] = v + rng.uniform(-0.05, 0.05, 6)
            q.append(p)
    q.append(np.array([[-0.4, -0.4, -0.4], [4.4, 4.4, 4.4], [-1.5, 4.4, 2.0], [5.5, -1.5, -1.5]]))  # outside along several axes
    add("outside_box", dense, np.concatenate(q), outside_cells={-2, -1, 4, 5}, min_found=20, min_unfound=20)
    around = lambda lo, hi, n: rng.uniform(np.asarray(lo) - 1.3, np.asarray(hi) + 1.3, (n, 3))
    # boxes one cell thick along one, two and all three axes (the last: a single-cell map)
    for name, lo, hi in (("flat_z", (0, 0, 0.1), (4, 4, 0.9)), ("line_x", (0, 0.1, 0.1), (5, 0.9, 0.9)), ("single_cell", (0.1, 0.1, 0.1), (0.9, 0.9, 0.9)),
                         ("single_cell_negative", (-6.9, -2.9, -0.9), (-6.1, -2.1, -0.1))):
        mm = rng.uniform(lo, hi, (600, 3))
        add(name, mm, np.concatenate([around(lo, hi, 150), rng.uniform(lo, hi, (50, 3))]),
            thin_axes=tuple(int(np.floor(h) == np.floor(l)) for l, h in zip(lo, hi)), min_found=20, min_unfound=20)
    # boxes entirely below / above zero (cmin of either sign, far from the origin)
    add("all_negative", rng.uniform((-57.5, -8.3, -3.9), (-53.1, -4.2, -1.1), (3000, 3)),
        around((-57.5, -8.3, -3.9), (-53.1, -4.2, -1.1), 300), box_sign=-1, min_found=20, min_unfound=20)
    add("all_positive", rng.uniform((100.2, 7.1, 1.3), (104.7, 11.6, 3.8), (3000, 3)),
        around((100.2, 7.1, 1.3), (104.7, 11.6, 3.8), 300), box_sign=1, min_found=20, min_unfound=20)
    # two clusters far apart: a box of millions of cells, nearly all of them empty (the gridding kernel's scan walks
    # thousands of cells per thread)
    a, b = rng.uniform(-2, 2, (1500, 3)), rng.uniform(-2, 2, (1500, 3)) + np.array([300.0, 200.0, 60.0])
    add("sparse_box", np.concatenate([a, b]),
        np.concatenate([rng.uniform(-2.5, 2.5, (100, 3)), rng.uniform(-2.5, 2.5, (100, 3)) + [300.0, 200.0, 60.0], rng.uniform(-2, 302, (40, 3))]),
        min_cells=3_000_000, min_found=50, min_unfound=20)
    return cases


SWEEP_SIGMAS = (0.0, 0.02, 0.05, 0.1, 0.2)


def threshold_sweep(defs):
    """name -> problem: inputs that populate both sides of every accept / reject branch of the two fits (asserted on the
    CPU oracle): rooms at five noise levels on map and scan; corner neighbourhoods that are clustered (tight knots along
    an edge) and near-isotropic (balls); surf queries hovering over a plane that does not pass through the origin,
    around the weight threshold s = 0.1 (s falls with the distance to the plane over the root of the query's norm)."""
    out = {}
    for k, sg in enumerate(SWEEP_SIGMAS):
        out["sigma_%g" % sg] = make_problem(defs, 90 + k, n_map_surf=8000, n_map_corner=2400, n_scan_surf=500, n_scan_corner=300, noise=sg)[0]
    rng = np.random.default_rng(77)
    # knots: 5-point clusters (sigma 2 cm) every 25 cm along a line, anisotropy decided by the knot's own scatter vs its neighbours
    t = np.repeat(np.arange(0, 30, 0.25), 5)
    knots = np.stack([t - 15, np.full_like(t, 2.0), np.full_like(t, 1.0)], 1) + rng.normal(0, 0.02, (len(t), 3))
    balls = rng.normal(0, 1, (3000, 3))
    balls = np.array([-5.0, -6.0, 0.5]) + balls / np.linalg.norm(balls, axis=1)[:, None] * rng.uniform(0, 1, (3000, 1)) ** (1 / 3) * np.array([3.0, 1.2, 0.8])
    mc = np.concatenate([knots, balls])
    qc = np.concatenate([knots[rng.choice(len(knots), 150, replace=False)] + rng.normal(0, 0.05, (150, 3)),
                         balls[rng.choice(len(balls), 250, replace=False)] + rng.normal(0, 0.05, (250, 3))])
    # plane z = -0.5 under the origin, queries hovering 0.3 .. 0.95 above it within 0.8 m of the axis
    gx = np.arange(-3, 3.01, 0.1)
    plane = np.stack(np.meshgrid(gx, gx, indexing="ij"), -1).reshape(-1, 2)
    plane = np.concatenate([plane, np.full((len(plane), 1), -0.5)], 1) + rng.normal(0, 0.005, (len(plane), 3))
    qs = np.stack([rng.uniform(-0.8, 0.8, 2500), rng.uniform(-0.8, 0.8, 2500), rng.uniform(-0.2, 0.45, 2500)], 1)
    out["shapes"] = defs.MapProblem(pad4(mc), pad4(plane), pad4(qc), pad4(qs), np.zeros(6, np.float32))
    return out


EXACT_CLAIMS = ("on_integers", "fifth_exactly_one", "fifth_just_below_one")  # hold at the identity transform only


def knn5_f32(cloud, sel):
    """the five smallest ((dx^2 + dy^2) + dz^2, index) of one associated point, in f32 as the search computes them"""
    d = cloud[:, :3].astype(np.float32) - np.asarray(sel, dtype=np.float32)
    sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    order = np.lexsort((np.arange(len(sq)), sq))[:5]
    return order, sq[order]


def check_lattice_claims(problem, claims, surf_records, exact):
    """asserts, from the ORACLE'S records of the surf queries (its exhaustive search knows no grid), that a lattice case
    is what its generator says — a generator that drifts off its edge fails here instead of hollowing the test"""
    rec, cloud = surf_records, problem.map_surf
    sel = rec["sel"].astype(np.float64)
    found = rec["ind"][:, 0] >= 0
    assert ((rec["ind"] >= 0).all(1) == found).all() and (np.isinf(rec["sq5"]) == ~found).all()
    lo = np.floor(cloud[:, :3].min(0)).astype(int)
    dim = np.floor(cloud[:, :3].max(0)).astype(int) - lo + 1
    cell = np.floor(sel).astype(int) - lo  # the query's cell relative to the map's box
    fifth = np.array([knn5_f32(cloud, s)[1][4] for s in rec["sel"]]) if len(cloud) >= 5 else np.full(len(rec), np.inf, np.float32)
    assert ((fifth < np.float32(1.0)) == found).all()
    for key, want in claims.items():
        if key in EXACT_CLAIMS and not exact:
            continue
        if key == "on_integers":
            assert (sel == np.round(sel)).all()
        elif key == "min_found":
            assert found.sum() >= want, (key, found.sum())
        elif key == "min_unfound":
            assert (~found).sum() >= want, (key, (~found).sum())
        elif key == "fifth_exactly_one":
            assert ((fifth == np.float32(1.0)) & ~found).sum() == want, (key, fifth)
        elif key == "fifth_just_below_one":
            assert ((fifth == np.nextafter(np.float32(1.0), np.float32(0.0))) & found).sum() == want, (key, fifth)
        elif key == "spread_over_corner_cells":
            n = 0
            for r, c in zip(rec[found], np.floor(sel[found]).astype(int)):
                rel = np.floor(cloud[r["ind"], :3]).astype(int) - c
                assert (np.abs(rel) <= 1).all()
                n += len({tuple(v) for v in rel}) >= 4 and (np.abs(rel) == 1).all(1).any()
            assert n >= want, (key, n)
        elif key == "outside_cells":
            for a in range(3):
                seen = set(cell[:, a].tolist())
                assert {-2, -1, int(dim[a]), int(dim[a]) + 1} <= seen, (key, a, sorted(seen))
            assert want == {-2, -1, int(dim[0]), int(dim[0]) + 1}
            out1 = ((cell == -1) | (cell == dim)).any(1) & ((cell >= -1) & (cell <= dim)).all(1)
            assert (found & out1).sum() >= 10  # one cell outside still finds its neighbours inside
            assert not found[((cell <= -2) | (cell >= dim + 1)).any(1)].any()  # two cells outside cannot
        elif key == "thin_axes":
            assert tuple(int(v == 1) for v in dim) == tuple(want) and sum(want) >= 1, (key, dim)
            outside = ((cell < 0) | (cell >= dim)).any(1)
            assert (found & outside).sum() >= 10 and (found & ~outside).sum() >= 10
        elif key == "box_sign":
            assert (np.sign(lo) == want).all() and (np.sign(lo + dim) == want).all(), (key, lo, dim)
        elif key == "min_cells":
            assert int(np.prod(dim.astype(np.int64))) >= want, (key, dim)
        else:
            raise KeyError(key)
