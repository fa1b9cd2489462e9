"""Raw clouds built from a CHOSEN 16 x 1800 range image, for the segmentation stage (image_projection_node, IP:191-415;
csrc/segment_kernels.hip, csrc/host/frontend.cpp, oracle/frontend_oracle.cpp).

Ray-cast scenes give big blobs in which almost every cell has its right neighbour in its own segment, so what makes the
device's min-label propagation equal to the reference's BFS is never decisive there: the DIRECTED neighbour table (right,
"+255 columns, else column 0", down), the seed's own row not counting towards the 3-row test, the 5 .. 29-cell window,
labels that travel through hundreds of thread runs, the LAST point of a cell owning it.  The cases below decide them.

Every point sits at the centre of its cell — elevation -15 + 2 row degrees (0.05 of a row above the row's lower boundary),
azimuth at the column centre (0.1 deg from either edge) — and neighbouring ranges differ by a ratio that is far from
the connect limits (1.00201 along a row, 1.01954 between rows), so whose atan2f is used cannot matter:
tests/test_seg_inputs.py checks those margins, and that each case is what it claims, with `segment_model` below.
"""
import collections

import numpy as np

ROWS, COLS, CELLS = 16, 1800, 16 * 1800
RUN = 29  # cells per thread of segment_kernel's label propagation (28 800 cells over 1024 threads)
ALPHA_X, ALPHA_Y = float(np.float32(0.2 / 180.0 * np.pi)), float(np.float32(2.0 / 180.0 * np.pi))  # parameters.h:88-90
THETA = float(np.float32(1.0472))


def cell_points(rows, cols, rng):
    """(…, 3) float64: the point at the centre of cell (row, col) at range rng (column = IP:224-227 of atan2(x, y))"""
    el = np.radians(-15.0 + 2.0 * np.asarray(rows, np.float64))
    az = np.radians(0.2 * (np.asarray(cols, np.float64) - 900.0))
    rng = np.asarray(rng, np.float64)
    return np.stack([rng * np.cos(el) * np.cos(az), rng * np.cos(el) * np.sin(az), rng * np.sin(el)], -1)


def points_of(cells, rng):
    """(n, 4) float32 raw points at the centres of the flat cell indices `cells`"""
    cells = np.asarray(cells)
    p = np.zeros((len(cells), 4), np.float32)
    p[:, :3] = cell_points(cells // COLS, cells % COLS, rng)
    return p


def cloud_from_range_image(img, extra=None, extra_at=None, perm=None):
    """img: (16, 1800), one range per cell, 0 = no return -> raw float32 (n, 4) cloud in firing order: column-major from
    +179.8 deg clockwise, the 16 rings of a column together (as _wide_room_raw_scan of test_gpu_edge_cases.py).
    extra: (m, 4) further points — appended (extra_at None: they are the LATER owners of their cells) or inserted before
    the base cloud's positions extra_at (np.insert: earlier owners).  perm: a permutation of the resulting firing order."""
    img = np.asarray(img, np.float64)
    assert img.shape == (ROWS, COLS)
    cols, rows = np.meshgrid(np.arange(COLS - 1, -1, -1), np.arange(ROWS), indexing="ij")  # (1800, 16): column-major
    keep = img[rows, cols] > 0
    raw = points_of((rows * COLS + cols)[keep], img[rows, cols][keep])
    if extra is not None:
        extra = np.asarray(extra, np.float32).reshape(-1, 4)
        raw = np.concatenate([raw, extra]) if extra_at is None else np.insert(raw, np.asarray(extra_at), extra, axis=0)
    if perm is not None:
        raw = raw[np.asarray(perm)]
    return np.ascontiguousarray(raw, np.float32)


def segment_model(img):
    """A plain statement of the stage on a range image whose points sit at the cell centres, in float64: ground flags, the
    directed edge set, label(x) = the smallest raster index from which x is reachable (the reference's BFS: seeds in raster
    order, a flood never enters a labelled cell), validity, emission.  depth[x] = the least number of edges that LEAVE a
    29-cell run on a path from x's root to x: a right edge inside a run is free for the kernel (same thread, same pass),
    every other edge can cost it a sweep."""
    img = np.asarray(img, np.float64)
    has = img > 0
    rr, cc = np.meshgrid(np.arange(ROWS), np.arange(COLS), indexing="ij")
    pts = cell_points(rr, cc, img)
    gmat = np.zeros((ROWS, COLS), np.int8)
    ground_margin = np.inf
    for i in range(5):  # groundRemoval (IP:243-278): pairs (i, i + 1), i < groundScanInd, bottom-up
        both = has[i] & has[i + 1]
        d = pts[i + 1] - pts[i]
        ang = np.degrees(np.arctan2(d[:, 2], np.hypot(d[:, 0], d[:, 1])))
        gmat[i][~both] = -1  # (also over the 1 the pair below may have left there, IP:252-256)
        g = both & (np.abs(ang) <= 10)
        gmat[i][g] = 1
        gmat[i + 1][g] = 1
        if both.any():
            ground_margin = min(ground_margin, np.abs(np.abs(ang[both]) - 10).min())
    ground = gmat == 1
    elig = (has & ~ground).ravel()
    flat = np.arange(CELLS)
    r, c = flat // COLS, flat % COLS
    rng = img.ravel()
    targets = [np.where(c + 1 < COLS, flat + 1, r * COLS), np.where(c + 255 < COLS, flat + 255, r * COLS),
               np.where(r + 1 < ROWS, flat + COLS, -1)]
    edges, edge_margin = [], np.inf
    for d, t in enumerate(targets):
        ok = elig & (t >= 0)
        ok[ok] &= elig[t[ok]]
        a, b = rng[ok], rng[t[ok]]
        d1, d2 = np.maximum(a, b), np.minimum(a, b)
        alpha = ALPHA_Y if d == 2 else ALPHA_X
        ang = np.arctan2(d2 * np.sin(alpha), d1 - d2 * np.cos(alpha))
        if ang.size:
            edge_margin = min(edge_margin, np.abs(ang - THETA).min())
        e = np.zeros(CELLS, bool)
        e[np.flatnonzero(ok)[ang > THETA]] = True
        edges.append(e)
    out = [[] for _ in range(CELLS)]
    parent = list(range(CELLS))  # union-find: weakly connected components

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for d, t in enumerate(targets):
        for u in np.flatnonzero(edges[d]).tolist():
            v = int(t[u])
            out[u].append((v, 0 if (d == 0 and v == u + 1 and u // RUN == v // RUN) else 1))
            parent[find(u)] = find(v)
    label = np.full(CELLS, -1, np.int64)
    depth = np.zeros(CELLS, np.int64)
    segments = {}
    for s in np.flatnonzero(elig).tolist():
        if label[s] >= 0:
            continue
        label[s], depth[s] = s, 0
        cells, q = [s], collections.deque([s])
        while q:  # 0-1 BFS inside the flood of seed s
            u = q.popleft()
            for v, w in out[u]:
                if label[v] == -1:
                    label[v], depth[v] = s, depth[u] + w
                    cells.append(v)
                elif label[v] == s and depth[v] > depth[u] + w:
                    depth[v] = depth[u] + w
                else:
                    continue
                q.appendleft(v) if w == 0 else q.append(v)
        pushed_rows = {v // COLS for v in cells if v != s}  # the seed itself is not a pushed neighbour (IP:383-387)
        valid = len(cells) >= 30 or (len(cells) >= 5 and len(pushed_rows) >= 3)
        segments[s] = dict(cells=cells, size=len(cells), rows=len(pushed_rows), valid=valid)
    valid_cell = np.zeros(CELLS, bool)
    oracle_label = np.full(CELLS, -1, np.int64)
    for k, (s, seg) in enumerate(sorted((s, g) for s, g in segments.items() if g["valid"])):
        valid_cell[seg["cells"]] = True
        oracle_label[seg["cells"]] = k + 1
    invalid_cell = elig & ~valid_cell
    oracle_label[invalid_cell] = 999999
    g = ground.ravel()
    emitted = valid_cell | (g & ~((c % 5 != 0) & (c > 5) & (c < COLS - 5)))
    return dict(ground=ground, eligible=elig.reshape(ROWS, COLS), edges=edges, label=label.reshape(ROWS, COLS),
                depth=depth.reshape(ROWS, COLS), segments=segments, emitted=emitted.reshape(ROWS, COLS),
                oracle_label=oracle_label.reshape(ROWS, COLS), n_outlier=int((invalid_cell & (r > 5) & (c % 5 == 0)).sum()),
                n_components=len({find(x) for x in np.flatnonzero(elig).tolist()}),
                edge_margin=float(edge_margin), ground_margin=float(ground_margin))


# ---- the cases: each returns dict(raw=cloud, img=the range image its owners leave (None: nothing projects), + its claims)

BLOCKS = (4, 3, 2, 1, 3, 1, 2)  # rows 0-3, 4-6, 7-8, 9, 10-12, 13, 14-15: a 2-row and two 1-row blocks lie above ring 5


def directed_chains_image(a=10.0):
    """Range a 1.05^(col mod 3) 1.05^(block parity): neighbouring columns never connect, a cell connects to column + 255
    (255 = 3 * 85: the same class), and beyond column 1544 to column 0 — which only class 0 matches.  Rows are grouped in
    blocks of equal range (a second factor 1.05 between blocks): inside a block every cell connects downwards."""
    img = np.zeros((ROWS, COLS))
    row = 0
    for k, h in enumerate(BLOCKS):
        img[row:row + h] = a * 1.05 ** (np.arange(COLS) % 3) * 1.05 ** (k % 2)
        row += h
    return img


def directed_chains():
    """Chains c0, c0 + 255, ... of 8 cells (c0 < 15) or 7 (1800 = 7 * 255 + 15) per row, times the rows of the block: 7 / 8
    (one row: invalid), 14 / 16 (two rows: invalid), 21 / 24 (valid by the row rule), 28 (row rule) / 32 (size).  Every
    class-0 chain ends in column 0 and so leads on into column 0's own chain: weakly connected, but directed — an
    undirected labelling merges each block's class-0 cells into one huge valid segment, a wrap to col + 255 - 1800 joins
    chain c0 to chain c0 + 240."""
    img = directed_chains_image()
    sizes = {n * h: h >= 3 for h in BLOCKS for n in (7, 8)}  # size -> valid
    return dict(raw=cloud_from_range_image(img), img=img, sizes=sizes)


SHAPES = {  # name: (cells as (d_row, d_col), valid)
    "lone_seed_5": ([(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)], False),  # the seed alone in its row: 2 pushed rows
    "seed_row_shared_5": ([(0, 0), (0, 1), (1, 0), (2, 0), (2, 1)], True),  # the control: 3 pushed rows
    "line_4": ([(0, j) for j in range(4)], False),
    "column_4": ([(i, 0) for i in range(4)], False),
    "line_5": ([(0, j) for j in range(5)], False),
    "two_rows_5": ([(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)], False),
    "column_5": ([(i, 0) for i in range(5)], True),
    "line_29": ([(0, j) for j in range(29)], False),
    "two_rows_29": ([(0, j) for j in range(15)] + [(1, j) for j in range(14)], False),
    "three_rows_29": ([(i, j) for i in range(3) for j in range(10)][:29], True),
    "line_30": ([(0, j) for j in range(30)], True),
    "two_rows_30": ([(i, j) for i in range(2) for j in range(15)], True),
    "three_rows_30": ([(i, j) for i in range(3) for j in range(10)], True),
}


def seed_row():
    """Isolated segments of equal range on an empty image.  Every shape stands three times: in rings 0 .. 4 (never an
    outlier), in rings 6 .. 10 on a column divisible by 5 and in rings 11 .. 15 one column further (a single-column shape
    then holds no outlier column).  Anchors are 100 columns apart (no two cells 255 apart in a row), the top band's are
    shifted by 50 columns against the middle band's (rows 10 and 11 never share a column)."""
    img = np.zeros((ROWS, COLS))
    placed = []
    for band, (row0, col0) in enumerate(((0, 40), (6, 40), (11, 91))):
        for k, (name, (cells, valid)) in enumerate(SHAPES.items()):
            flat = sorted((row0 + i) * COLS + col0 + 100 * k + j for i, j in cells)
            img.ravel()[flat] = 10.0
            placed.append(dict(name=name, band=band, cells=flat, valid=valid))
    n_outlier = sum(1 for p in placed if not p["valid"] for c in p["cells"] if c // COLS > 5 and c % COLS % 5 == 0)
    return dict(raw=cloud_from_range_image(img), img=img, placed=placed, n_outlier=n_outlier)


SERP_UNIT, SERP_ROW, SERP_MIN_DEPTH = 1.0007, 84, 500


def serpentine_image(base=20.0):
    """One segment whose root (cell 0) reaches the rest only through a long path.  Log-ranges in units of ln 1.0007: along
    a row a triangle (up 900 columns, down 900: column 1799 meets column 0 again, so a row can be walked all the way round,
    rightwards — the only way the edges allow), every row 84 units (a factor 1.0605) BELOW the one under it (closer: in the
    rings that groundRemoval reads a farther upper ring would look like floor), and near one link column per row pair
    row r dips to row r + 1's range, one unit per column.  The walk enters row r + 1 at link(r) and
    has to go round to link(r + 1) = link(r) - 200 to get further down.  Steps along a row are 0 or 2 units (ratio <=
    1.0014: connected, 0.14 rad from the limit — the unit is 1.0007 and not 1.001 because two steps of 1.001 would lie
    within 2e-3 rad of it); cells 255 apart connect only where they happen to lie within 2 units
    (3 units: 0.02 rad on the other side); rows connect within 27 units of each other (+-27 columns around a link)."""
    col = np.arange(COLS)
    tri = np.where(col <= 900, col, COLS - col).astype(np.float64)
    units = np.zeros((ROWS, COLS))
    for r in range(ROWS):
        units[r] = tri - SERP_ROW * r
        if r < ROWS - 1:
            link = (1700 - 200 * r) % COLS
            units[r] -= np.maximum(0, SERP_ROW - np.abs(col - link))
    return base * SERP_UNIT ** units


def serpentine():
    img = serpentine_image()
    return dict(raw=cloud_from_range_image(img), img=img, min_depth=SERP_MIN_DEPTH)


def _ownership_parts():
    """A wall of range 10 in rings 6 .. 13 (14 400 cells, one segment) and, in 300 cells of it, rival points 5 % farther
    (a cell they own connects to nothing: a 1-cell segment, dropped) — a third, 5 % nearer, in every other such cell."""
    img = np.zeros((ROWS, COLS))
    img[6:14] = 10.0
    rng = np.random.default_rng(11)
    contested = np.sort(rng.choice(np.arange(6 * COLS, 14 * COLS), 300, replace=False))
    far, near = points_of(contested, 10.5), points_of(contested[::2], 9.5)
    return img, contested, far, near


def ownership(order="rivals_last", n_total=None):
    """rivals_last: the 10.5 m points are fired after the wall (they own their cells: 300 holes in the wall);
    rivals_first: the same points, fired before it (the wall's own points own every cell).  The 9.5 m points are fired
    before the wall both times and never own a cell.  n_total: pad the cloud to that many points with returns 11 m
    away in random wall cells, fired first (overwritten by everything)."""
    img, contested, far, near = _ownership_parts()
    base = cloud_from_range_image(img)
    if order == "rivals_last":
        raw = cloud_from_range_image(img, extra=np.concatenate([near, far]), extra_at=[0] * len(near) + [len(base)] * len(far))
        final = img.copy()
        final.ravel()[contested] = 10.5
    else:
        raw = cloud_from_range_image(img, extra=np.concatenate([far, near]), extra_at=[0] * (len(far) + len(near)))
        final = img
    if n_total is not None:
        pad = n_total - len(raw)
        assert pad >= 0
        cells = np.random.default_rng(12).integers(6 * COLS, 14 * COLS, pad)
        raw = np.concatenate([points_of(cells, 11.0), raw])
    return dict(raw=np.ascontiguousarray(raw, np.float32), img=final, contested=contested)


def ownership_two_points():
    """n = 2, the smallest cloud the stage accepts: two returns in neighbouring cells, nothing survives"""
    img = np.zeros((ROWS, COLS))
    img[8, 700:702] = 10.0
    return dict(raw=cloud_from_range_image(img), img=img)


FLOOR_Z, WALL_D, BOX_D = -1.8, 12.0, 6.0
GROUND_HOLES = [(2, 0), (4, 5), (1796, 3), (1798, 1), (100, 0), (101, 1), (250, 2), (253, 3), (400, 4), (402, 5), (555, 4),
                (1000, 5), (1001, 0), (1205, 2), (1500, 1), (1503, 4)]  # (column, ring without a return)


def ground_holes():
    """A floor at z = -1.8 under rings 0 .. 6 (ring 6 is never ground-tested: a segment of floor cells), a wall 12 m away in
    rings 7 .. 15.  Holes: one of rings 0 .. 5 without a return — the pair that has the hole on top gets groundMat -1, over
    the 1 the pair below left there (the cell under a hole is no longer ground), and the cell above the hole becomes
    ground from the next pair or not at all (ring 5 above a hole in ring 4: no longer
    ground) — in columns 0 .. 5 / 1795 .. 1799 (never decimated) and elsewhere (kept when col % 5 == 0).  A box 6 m away in
    rings 2 .. 5: one column of it (4 cells) left of a two-column strip where the floor shows through, 30 columns right
    of it — the strip is ground, so the single column is a segment of its own and is dropped."""
    img = np.zeros((ROWS, COLS))
    el = np.radians(-15.0 + 2.0 * np.arange(ROWS))
    img[:7] = (FLOOR_Z / np.sin(el[:7]))[:, None]
    img[7:] = (WALL_D / np.cos(el[7:]))[:, None]
    box = (BOX_D / np.cos(el[2:6]))[:, None]
    img[2:6, 700:701] = box
    img[2:6, 703:733] = box
    for col, ring in GROUND_HOLES:
        img[ring, col] = 0.0
    lone_column = [r * COLS + 700 for r in range(2, 6)]
    return dict(raw=cloud_from_range_image(img), img=img, lone_column=lone_column)


def nothing_projects():
    """Every point 0.1 of a row or more outside the image: elevation >= +17.3 deg (row >= 16.2) or <= -17.3 deg (row
    <= -1.1), one straight up.  n = 0, and every ring's start / end index is 0 - 1 + 5 / 0 - 1 - 5."""
    rng = np.random.default_rng(13)
    n = 3001
    el = np.radians(np.where(rng.random(n) < 0.5, rng.uniform(17.3, 80.0, n), rng.uniform(-80.0, -17.3, n)))
    az = np.radians(0.2 * (rng.integers(0, COLS, n) - 900.0))
    r = rng.uniform(3.0, 40.0, n)
    raw = np.zeros((n, 4), np.float32)
    raw[:, 0], raw[:, 1], raw[:, 2] = r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)
    raw[1500, :3] = (0.0, 0.0, 5.0)
    return dict(raw=raw, img=None)


def nan_returns():
    """directed_chains with non-finite returns fired into it: all-NaN points, NaN in z only, NaN in x only — at index 0, at
    the last two indices (nothing overwrites what the last one would leave in cell (7, 1350), where comparisons-only
    atan2 puts an all-NaN point) and in the middle.  `clean` is the same cloud with those points deleted: the expected
    segmentation, start / end orientation included (first, last and second-to-last REMAINING points)."""
    clean = directed_chains()["raw"]
    nan = np.float32(np.nan)
    p = points_of([7 * COLS + 1350, 3 * COLS + 20, 9 * COLS + 905], [12.0, 12.0, 12.0])  # finite templates
    rows = []
    for tmpl, which in ((p[0], "all"), (p[1], "z"), (p[2], "x")):
        q = tmpl.copy()
        if which == "all":
            q[:3] = nan
        elif which == "z":
            q[2] = nan
        else:
            q[0] = nan
        rows.append(q)
    all_nan, z_nan, x_nan = rows
    n = len(clean)
    at = [0, 0, 5000, 5000, 14000, 14000, 14001, n, n]  # positions in the clean cloud the points are inserted before
    pts = [z_nan, all_nan, z_nan, x_nan, all_nan, x_nan, z_nan, x_nan, all_nan]
    raw = np.insert(clean, at, np.array(pts, np.float32), axis=0)
    assert np.isnan(raw[0]).any() and np.isnan(raw[-1, :3]).all() and np.isnan(raw[-2]).any() and len(raw) == n + len(at)
    return dict(raw=np.ascontiguousarray(raw), clean=clean, img=directed_chains_image())


CASES = {
    "directed_chains": directed_chains,
    "seed_row": seed_row,
    "serpentine": serpentine,
    "ownership_rivals_last_32768": lambda: ownership("rivals_last", 32768),  # the last register slot of the point path
    "ownership_rivals_first": lambda: ownership("rivals_first"),             # 14 850 points: n % 4 == 2
    "ownership_rivals_last_32769": lambda: ownership("rivals_last", 32769),  # the first size of the cell-by-cell path
    "ownership_two_points": ownership_two_points,
    "ground_holes": ground_holes,
    "nothing_projects": nothing_projects,
    "nan_returns": nan_returns,
}

_BUILT = {}


def case(name):
    """the case `name`, built once per process (treat it as read-only)"""
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
        _BUILT[name]["raw"].setflags(write=False)
    return _BUILT[name]
