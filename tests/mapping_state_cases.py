"""Seeded inputs of tests/test_gpu_mapping_state.py and tests/test_gpu_sort_shapes.py (not a test), and the numpy
statements of what those tests rest on (asserted on the CPU by tests/test_mapping_state_inputs.py).

History pairs.  The mapping side keeps grow-only device scratch that no call clears; a history test runs
a call Y on a fresh context and on one that first ran a warm-up X, and compares the bits.  X is STRICTLY larger than Y
in every dimension the C API sizes an allocation by — the *_extents functions below restate that sizing — so whatever
stale element a broken kernel of Y could read lies inside an allocation X sized and wrote: wrong data, never memory
outside the allocations.  Nothing here fills scratch with patterns.

Sort cases.  Boxes whose VoxelGrid jobs need 0, 1, 2, 3 and 4 radix passes (pass_count restates lm_setup_kernel), one
of them a key of 31 bits; counts on the 512-point tile and the 64-lane wave; a voxel run over a tile edge."""
import functools
import importlib

import numpy as np

import local_map_np as lnp
from local_map_synth import room_scan, trajectory

F = np.float32
TILE, WAVE, DIGIT = 512, 64, 8
E = np.zeros((0, 4), F)
ID = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
INT_MAX = 2 ** 31 - 1
SMALL = dict(n_corner=60, n_surf=500, n_outlier=40)
BIG = dict(n_corner=150, n_surf=1250, n_outlier=100)  # ~1.5 k points a frame
FAR = np.array([[-9e5, -9e5, -9e5, 0], [9e5, 9e5, 9e5, 0]], F)  # a VoxelGrid box of more than 2^31 cells
PT = np.ones((3, 4), F)
AR_CHUNK = 16  # keyframe_archive.h kArScanChunk
LOOP_Q_PER_BLOCK = 32  # loop_icp.h kLoopQPerBlock
LOOP_SUMS = 17  # loop_icp_math.h kSums


def frame(seed, pose, **kw):
    return room_scan(seed, pose, **kw) + (pose,)


def tiles(n):
    return -(-int(n) // TILE)


def strictly_larger(x, y):
    """the dimensions in which the warm-up's extents x do NOT exceed y's"""
    assert set(x) == set(y)
    return [k for k in x if not x[k] > y[k]]


# ---- the VoxelGrid set-up, as lm_setup_kernel states it -----------------------------------------------------------------
def pass_count(cloud, leaf):
    """(ncell, bits, passes) of the VoxelGrid job over `cloud`: f32 inv = 1.0f / leaf, floorf(min * inv), floorf(max * inv),
    bits = the smallest b with 2^b >= ncell, passes = ceil(bits / 8).  An empty cloud: (0, 0, 0); a box of more than
    2^31 cells (LINS_E_CAPACITY): (ncell, None, None)."""
    p = np.asarray(cloud, F).reshape(-1, 4)
    if len(p) == 0:
        return 0, 0, 0
    inv = F(1.0) / F(leaf)
    lo = np.floor(p[:, :3].min(0) * inv).astype(np.int64)
    hi = np.floor(p[:, :3].max(0) * inv).astype(np.int64)
    div = hi - lo + 1
    ncell = int(div[0]) * int(div[1]) * int(div[2])
    if ncell > 2 ** 31:
        return ncell, None, None
    bits = 0
    while (1 << bits) < ncell:
        bits += 1
    return ncell, bits, -(-bits // DIGIT)


def voxel_keys(cloud, leaf):
    """the sort key (PCL's linear voxel index) of every point"""
    p = np.asarray(cloud, F).reshape(-1, 4)
    inv = F(1.0) / F(leaf)
    lo = np.floor(p[:, :3].min(0) * inv).astype(np.int64)
    div = np.floor(p[:, :3].max(0) * inv).astype(np.int64) - lo + 1
    ijk = np.floor(p[:, :3] * inv).astype(np.int64) - lo
    return ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]


LEAVES = (0.2, 0.4, 0.2, 0.4, 0.4, 0.4)  # corner map, surf map, cornerDS, surfDS, outlierDS, surfTotalDS
JOB_NAMES = ("map corner", "map surf", "scan corner", "scan surf", "scan outlier", "scan total")


def job_inputs(frames, scan, window=50):
    """the six VoxelGrid jobs of one local-map entry: [(input cloud, leaf)] in LOCAL_* order (the sixth job's input is the
    output of the fourth and the fifth, None where either is refused)"""
    used = frames[max(0, len(frames) - window):]
    cat = lambda xs: np.concatenate(xs) if xs else E
    corner = cat([lnp.transform(f[0], f[3]) for f in used])
    surf = cat([c for f in used for c in (lnp.transform(f[1], f[3]), lnp.transform(f[2], f[3]))])
    ds = [lnp.voxel_grid(scan[1], 0.4), lnp.voxel_grid(scan[2], 0.4)]
    total = None if any(d is None for d in ds) else np.concatenate(ds)
    return list(zip([corner, surf, scan[0], scan[1], scan[2], total], LEAVES))


def entry_passes(frames, scan, window=50):
    """per job of the entry (ncell, bits, passes)"""
    return [(0, None, None) if c is None else pass_count(c, leaf) for c, leaf in job_inputs(frames, scan, window)]


# ---- boxes of every pass count (leaf 0.2 / leaf 0.4) ------------------------------------------------------------------
BOXES = {
    "one cell": ((0.01, 0.01, 0.01), (0.15, 0.15, 0.15)),  # 1 / 1 cells: 0 / 0 passes
    "metre": ((0.0, 0.0, 0.0), (1.1, 1.1, 0.9)),  # 180 / 27: 1 / 1
    "room": ((-15.0, -10.0, -1.5), (15.0, 10.0, 4.5)),  # 472 781 / 62 016: 3 / 2
    "field": ((-150.0, -150.0, -15.0), (150.0, 150.0, 15.0)),  # 3.4e8 / 4.3e7: 4 / 4
    "plain": ((-1000.0, -1000.0, -1.9), (1000.0, 1000.0, 1.9)),  # 2 000 400 020 (31 bits) / 2.5e8: 4 / 4
}
BOX_PASSES = {"one cell": (0, 0), "metre": (1, 1), "room": (3, 2), "field": (4, 4), "plain": (4, 4)}


def box_cloud(name, n, seed):
    """n points uniform in the box, its two extreme corners among them (first and last)"""
    lo, hi = (np.array(v) for v in BOXES[name])
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(lo, hi, (n, 3))
    xyz[0], xyz[-1] = lo, hi
    return np.concatenate([xyz, rng.uniform(0, 100, (n, 1))], 1).astype(F)


@functools.lru_cache(maxsize=None)
def pass_entries():
    """[(frames of the entry's ring, scan)]: three entries (slot k = entry k) whose eighteen jobs need 0, 1, 2, 3 and 4
    passes in one launch — map clouds under the identity pose, so that the transform keeps the extents.  The 31-bit
    box is a corner map (entry 2) and a scan corner cloud (entry 1); an empty ring gives two jobs without input."""
    b = lambda name, seed, n=600: box_cloud(name, n, seed)
    return [
        ([], (b("one cell", 1, 300), b("metre", 2, 300), b("room", 3))),
        ([(b("room", 4), b("field", 5), E, ID)], (b("plain", 6), b("room", 7), b("one cell", 8, 300))),
        ([(b("plain", 9), b("metre", 10, 300), b("one cell", 11, 300), ID)], (b("field", 12), b("one cell", 13, 300), b("metre", 14, 300))),
    ]


# ---- counts on the tile and the wave, a run over a tile edge, duplicates, voxel faces ------------------------------------
EDGE_COUNTS = (512, 513, 1024, 64, 65)


def patch(n, seed):
    """n points in a 3 x 3 x 1 m patch: 1 125 voxels at leaf 0.2 — runs of one and of several points"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform((-1.5, -1.5, 0.0), (1.5, 1.5, 1.0), (n, 3))
    return np.concatenate([xyz, rng.uniform(0, 100, (n, 1))], 1).astype(F)


@functools.lru_cache(maxsize=None)
def edge_entries():
    """one entry per count of EDGE_COUNTS: every input cloud of the entry — the ring's one frame (identity pose; its
    corner and surf clouds, no outliers) and the three scan clouds — has exactly that many points"""
    return [([(patch(n, 100 + n), patch(n, 200 + n), E, ID)], (patch(n, 300 + n), patch(n, 400 + n), patch(n, 500 + n))) for n in EDGE_COUNTS]


def straddle_cloud(leaf, seed=7):
    """1024 points on 1023 voxels in a row along x, one point each but voxel 511 with two: in sorted order that run begins
    in the last lane of tile 0 (position 511) and ends in the first lane of tile 1 (position 512).  Input order shuffled."""
    rng = np.random.default_rng(seed)
    vox = np.r_[np.arange(1023), 511]
    xyz = np.stack([(vox + rng.uniform(0.2, 0.8, 1024)) * leaf, rng.uniform(0.01, 0.15, 1024), rng.uniform(0.01, 0.15, 1024)], 1)
    c = np.concatenate([xyz, rng.uniform(0, 100, (1024, 1))], 1).astype(F)
    return c[rng.permutation(1024)]


def straddle_entry():
    return [], (straddle_cloud(0.2), straddle_cloud(0.4), patch(65, 65))


DUP_POINT = np.array([0.5, -1.25, 2.0, 3.0], F)  # (600 x each coordinate is exact in f32: the centroid is the point)


def duplicate_entry(n=600):
    d = np.tile(DUP_POINT, (n, 1))
    return [(d, d, E, ID)], (d, d, d)


def face_lattice():
    """every point with coordinates k * 0.2, k = -16 .. 0: points on voxel faces at negative coordinates, where
    floorf(x * inv) decides the voxel"""
    g = (np.arange(-16, 1) * 0.2).astype(F)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([xyz, np.arange(len(xyz), dtype=F)[:, None] % F(97)], 1).astype(F)


def face_entry():
    lat = face_lattice()
    return [(lat, lat[::3], E, ID)], (lat, lat, lat[::5])


# ---- sizing of a local-map build (lins_local_map_capi.hip local_map_build_impl) ------------------------------------------
def build_extents(entries, chunk=None, window=50):
    """entries: [(frames on the map side — the ring's window or the surround list's frames in list order —, scan)].
    chunk: the archive's scan chunk of a surround build (None: a ring build, nothing is split)."""
    x = dict(staged_points=0, tiles_stage_a=0, tiles_stage_b=0, output_points=0, raw_points=0, jobs=6 * len(entries), segments=0,
             split_jobs=0, chunks=0)
    for frames, scan in entries:
        used = frames if chunk is not None else frames[max(0, len(frames) - window):]
        mc = sum(len(f[0]) for f in used)
        ms = sum(len(f[1]) + len(f[2]) for f in used)
        nc, ns, no = (len(c) for c in scan)
        x["staged_points"] += mc + ms + nc + ns + no + (ns + no)
        x["tiles_stage_a"] += sum(tiles(v) for v in (mc, ms, nc, ns, no))
        x["tiles_stage_b"] += tiles(ns + no)
        x["output_points"] += mc + ms + (nc + ns + no) + ns + no
        x["raw_points"] += nc + ns + no
        x["segments"] += sum(len(c) > 0 for f in used for c in f[:3])
        for m in (mc, ms):
            if chunk is not None and tiles(m) > chunk:
                x["split_jobs"] += 1
                x["chunks"] += -(-tiles(m) // chunk)
    x["tiles"] = x["tiles_stage_a"] + x["tiles_stage_b"]
    if chunk is None:
        del x["split_jobs"], x["chunks"]
    return x


# ---- 1. ring builds --------------------------------------------------------------------------------------------------------
RING = dict(n_slots=9, window=12, max_pts=4096)


@functools.lru_cache(maxsize=None)
def ring_pair():
    """X: five entries on slots 0 .. 4 — three with windows of 12 frames of ~1.5 k points and two of one frame (five, so
    that X's job count exceeds Y's) —, scans of ~3 k points.  Y: four entries on slots 5 .. 8, all smaller: an empty
    ring with empty scan clouds; one refused with LINS_E_CAPACITY; one with a surf scan of exactly 512 points; a plain one."""
    poses = trajectory(12, seed=31)
    xf = {s: [frame(3100 + 100 * s + i, poses[i], **BIG) for i in range(12)] for s in range(3)}
    xf[3], xf[4] = [frame(3500, poses[0], **SMALL)], [frame(3501, poses[1], **SMALL)]
    xs = [room_scan(3600 + k, poses[k], n_corner=300, n_surf=2500, n_outlier=150) for k in range(5)]
    yf = {5: [], 6: [frame(3700, poses[2], **SMALL)], 7: [frame(3710 + i, poses[i], **SMALL) for i in range(3)],
          8: [frame(3720 + i, poses[4 + i], **SMALL) for i in range(3)]}
    exact = room_scan(3800, poses[1], n_corner=60, n_surf=TILE, n_outlier=40)
    ys = [(E, E, E), (FAR, PT, PT), exact, room_scan(3801, poses[5], **SMALL)]
    return dict(X=dict(slots=[0, 1, 2, 3, 4], frames=xf, scans=xs), Y=dict(slots=[5, 6, 7, 8], frames=yf, scans=ys))


@functools.lru_cache(maxsize=None)
def ring_pass_pair():
    """the reverse mix of pass counts: every job of X (three entries, slots 0 .. 2) needs four passes, every job of Y
    (two entries, slots 3 .. 4, the same job slots of the table and the same ranges of the sort's scratch) none or one"""
    b = box_cloud
    xf = {s: [(b("plain", 600, 40 + s), b("field", 600, 50 + s), b("field", 300, 60 + s), ID)] for s in range(3)}
    xs = [(b("plain", 600, 70 + s), b("field", 600, 80 + s), b("field", 600, 90 + s)) for s in range(3)]
    yf = {3 + s: [(b("one cell", 200, 110 + s), b("metre", 200, 120 + s), b("one cell", 100, 130 + s), ID)] for s in range(2)}
    ys = [(b("metre", 200, 140 + s), b("one cell", 200, 150 + s), b("metre", 200, 160 + s)) for s in range(2)]
    return dict(X=dict(slots=[0, 1, 2], frames=xf, scans=xs), Y=dict(slots=[3, 4], frames=yf, scans=ys))


def ring_entries(side):
    return [(side["frames"][s], sc) for s, sc in zip(side["slots"], side["scans"])]


# ---- 2. surround builds and archive assemblies ---------------------------------------------------------------------------
ARCHIVE = dict(n_slots=2, max_frames=16, max_points=1 << 16)
SURROUND_CHUNK = 2
CORNER, SURF, OUTLIER, DROP_NEGATIVE = 1, 2, 4, 1


@functools.lru_cache(maxsize=None)
def archive_frames():
    """slot -> frames: twelve of ~1.5 k points on slot 0, three of 600 on slot 1; the newest of either with a few
    negative intensities (what DROP_NEGATIVE drops)"""
    poses = trajectory(12, seed=33)
    big = [frame(3300 + i, poses[i], **BIG) for i in range(12)]
    small = [frame(3400 + i, poses[2 * i], **SMALL) for i in range(3)]
    big[11][1][:9, 3] = -F(2.0)
    small[2][1][:5, 3] = -F(1.5)
    return {0: big, 1: small}


@functools.lru_cache(maxsize=None)
def surround_pair():
    """X: three entries with lists of all twelve frames of slot 0 (at chunk 2: 16 + 2 chunks an entry, both map jobs
    split).  Y: lists of three frames — slot 0's (the surf job splits into 4 chunks, the corner job does not split) and
    slot 1's (2 chunks)."""
    poses = trajectory(12, seed=33)
    order = np.random.default_rng(5).permutation(12).tolist()
    x = dict(slots=[0, 0, 0], lists=[list(range(12)), list(range(11, -1, -1)), order],
             scans=[room_scan(3900 + k, poses[k], n_corner=300, n_surf=2500, n_outlier=150) for k in range(3)])
    y = dict(slots=[0, 1], lists=[[5, 0, 3], [2, 0, 1]], scans=[room_scan(3950 + k, poses[3 + k], **SMALL) for k in range(2)])
    return dict(X=x, Y=y)


def surround_entries(side):
    fr = archive_frames()
    return [([fr[s][i] for i in lst], sc) for s, lst, sc in zip(side["slots"], side["lists"], side["scans"])]


def spec(slot, ids, clouds, leaf, flags=0):
    return dict(slot=slot, ids=list(ids), clouds=clouds, leaf=leaf, flags=flags)


@functools.lru_cache(maxsize=None)
def assembly_pair():
    """X: the history submap over twelve frames at leaf 0.4, the latest frame unfiltered with DROP_NEGATIVE, and (so that
    X's job count exceeds Y's) the twelve frames' three clouds at leaf 0.2.  Y, in the other entry order: the latest
    frame of slot 1 unfiltered, then a submap over its three frames."""
    x = [spec(0, range(12), CORNER | SURF, 0.4), spec(0, [11], CORNER | SURF, 0.0, DROP_NEGATIVE), spec(0, range(12), CORNER | SURF | OUTLIER, 0.2)]
    y = [spec(1, [2], CORNER | SURF, 0.0, DROP_NEGATIVE), spec(1, [0, 1, 2], CORNER | SURF, 0.4)]
    return dict(X=x, Y=y)


def assembly_extents(specs, chunk=AR_CHUNK):
    """lins_archive_assemble's sizing"""
    fr = archive_frames()
    x = dict(staged_points=0, sorted_points=0, tiles=0, voxelgrid_tiles=0, output_points=0, jobs=len(specs), segments=0, chunks=0)
    for sp in specs:
        cap = sum(len(fr[sp["slot"]][i][q]) for i in sp["ids"] for q in range(3) if sp["clouds"] & (1 << q))
        x["staged_points"] += cap
        x["output_points"] += cap
        x["tiles"] += tiles(cap)
        x["segments"] += len(sp["ids"])
        if sp["leaf"] > 0:
            x["sorted_points"] += cap
            x["voxelgrid_tiles"] += tiles(cap)
        if tiles(cap) > chunk:
            x["chunks"] += -(-tiles(cap) // chunk)
    return x


# ---- 3. scan-to-map --------------------------------------------------------------------------------------------------------
def _defs():
    return importlib.import_module("lins---lidar-inertial-slam_amd._ctypes_defs")


@functools.lru_cache(maxsize=None)
def map_pair():
    """X: three rooms of 23 k map points and 2.5 k queries whose maps carry forty stray points up to 30 m out (a box of
    61 x 51 x 12 cells).  Y: a room and a corridor of a third of the points in their own, smaller boxes."""
    from map_synth import make_corridor, make_problem

    defs = _defs()
    xs = []
    for k in range(3):
        p = make_problem(defs, 300 + k, n_scan_surf=2000, n_scan_corner=500)[0]
        rng = np.random.default_rng(310 + k)
        stray = lambda n: np.concatenate([rng.uniform((-30, -25, -3), (30, 25, 8), (n, 3)), np.zeros((n, 1))], 1).astype(F)
        mc, ms = np.concatenate([p.map_corner, stray(20)]), np.concatenate([p.map_surf, stray(20)])
        for m in (mc, ms):  # the box's corners for certain
            m[-2, :3], m[-1, :3] = (-30, -25, -3), (30, 25, 8)
        xs.append(defs.MapProblem(mc, ms, p.scan_corner, p.scan_surf, p.transform))
    ys = [make_problem(defs, 320, n_map_surf=6000, n_map_corner=900, n_scan_surf=400, n_scan_corner=120)[0],
          make_corridor(defs, 321, n_map_surf=6000, n_map_corner=800, n_scan_surf=500, n_scan_corner=120)[0]]
    return dict(X=xs, Y=ys)


def cells_of(cloud):
    """2 (ncell + 1) of a map cloud's 1 m box: cell starts and scratch cursors (map_upload)"""
    if len(cloud) == 0:
        return 4
    f = np.floor(np.asarray(cloud, F)[:, :3]).astype(np.int64)
    return 2 * (int(np.prod(f.max(0) - f.min(0) + 1)) + 1)


def map_extents(maps, queries):
    """maps: [(corner map, surf map)]; queries: [number of query points] per problem"""
    return dict(problems=len(maps), map_points=sum(len(c) + len(s) for c, s in maps), cells=sum(cells_of(c) + cells_of(s) for c, s in maps),
                query_points=sum(queries), largest_query=max(queries))


def problem_extents(problems):
    return map_extents([(p.map_corner, p.map_surf) for p in problems], [len(p.scan_corner) + len(p.scan_surf) for p in problems])


MAP_LOCAL = dict(n_slots=2, window=50, max_pts=4096, fills=(12, 3))


@functools.lru_cache(maxsize=None)
def map_local_case():
    """Y through LINS_MAP_LOCAL: two slots of twelve and of three frames of ~1.4 k points, scans of ~1.5 k near the rings'
    last poses; t0 = the last key pose as a transform (rx, ry, rz, x, y, z)"""
    poses = trajectory(40, seed=34)
    kw = dict(n_corner=150, n_surf=1200, n_outlier=60)
    frames = {s: [frame(3450 + 100 * s + i, poses[i], **kw) for i in range(f)] for s, f in enumerate(MAP_LOCAL["fills"])}
    truth = [poses[f - 1] + np.array([0.05, 0.03, 0.0, 0.0, 0.0, 0.01], F) for f in MAP_LOCAL["fills"]]
    scans = [room_scan(3480 + s, truth[s], n_corner=200, n_surf=1200, n_outlier=80) for s in range(2)]
    t0 = [np.array([p[3], p[4], p[5], p[0], p[1], p[2]], F) for p in poses[[f - 1 for f in MAP_LOCAL["fills"]]]]
    return dict(slots=[0, 1], frames=frames, scans=scans, t0=t0)


def map_local_extents():
    """the extents of the scan-to-map call on the built clouds, from the numpy restatement of the build"""
    c = map_local_case()
    built = [lnp.local_map(c["frames"][s], sc, MAP_LOCAL["window"])[0] for s, sc in zip(c["slots"], c["scans"])]
    return map_extents([(b[0], b[1]) for b in built], [len(b[2]) + len(b[5]) for b in built])


# ---- 4. loop-closure ICP ---------------------------------------------------------------------------------------------------
WIDE = np.array([[0, 0, 0, 0], [500, 500, 500, 1]], F)  # a target box of more than 2^26 cells: LINS_E_CAPACITY


@functools.lru_cache(maxsize=None)
def icp_pair():
    """X: three problems with sources of ~3 k points on targets of ~6 k.  Y: the first whole-loop problem of
    tests/loop_icp_cases.py (a source of 300 points; its stop margins are asserted by tests/test_loop_icp_inputs.py) and
    the same source on a target that is refused."""
    import loop_icp_cases as cases
    import loop_icp_np as licp

    xs = []
    for k in range(3):
        pose = trajectory(6, seed=35)[k].astype(np.float64)
        tgt = room_scan(3550 + k, pose, n_corner=600, n_surf=5400, n_outlier=0)
        src = room_scan(3560 + k, pose, n_corner=300 + 17 * k, n_surf=2700, n_outlier=0)
        xs.append((licp.to_map(np.concatenate(src[:2]), (pose + licp.ERR).astype(F)), licp.to_map(np.concatenate(tgt[:2]), pose)))
    s, t = cases.whole_loop_problems()[0][:2]
    return dict(X=xs, Y=[(s, t), (s, WIDE)])


def icp_extents(problems):
    ok = [(s, t) for s, t in problems if cells_of(t) <= 2 * ((1 << 26) + 1)]
    bpp = max(1, -(-max(len(s) for s, _ in ok) // LOOP_Q_PER_BLOCK))
    return dict(problems=len(problems), source_points=sum(len(s) for s, _ in problems), target_points=sum(len(t) for _, t in problems),
                gridded_points=sum(len(t) for _, t in ok), cells=sum(cells_of(t) for _, t in ok), blocks_per_problem=bpp,
                partials=len(problems) * bpp * LOOP_SUMS)


# ---- 5. key-pose selection -------------------------------------------------------------------------------------------------
def _poses6(xyz):
    p = np.zeros((len(xyz), 6), F)
    p[:, :3] = np.asarray(xyz, F).reshape(-1, 3)
    return p


@functools.lru_cache(maxsize=None)
def keypose_pair():
    """X: eight queries over 40 key poses; Y: two over 5 — poses on a 0.5 m lattice (equal distances, coincident poses).
    Per side: poses, times, select queries (slot, centre, radius, pose leaf), loop queries (slot, centre, radius, now,
    minimum gap) and the surround lists before."""
    def side(n, nq, seed):
        rng = np.random.default_rng(seed)
        poses = _poses6(np.stack([0.5 * rng.integers(-8, 9, n), 0.5 * rng.integers(-8, 9, n), 0.5 * rng.integers(-1, 2, n)], 1))
        centres = [tuple(float(v) for v in 0.5 * rng.integers(-4, 5, 3)) for _ in range(nq)]
        radii = [2.0 + 1.5 * (q % 4) for q in range(nq)]
        select = [(0, centres[q], radii[q], (1.0, 0.4, 0.02)[q % 3]) for q in range(nq)]
        loop = [(0, centres[q], radii[q], float(n + 10 * q), float(5 + q)) for q in range(nq)]
        lists = [rng.permutation(n)[: (q % 3) + 1].tolist() for q in range(nq)]
        return dict(poses=poses, times=np.arange(n, dtype=np.float64), select=select, loop=loop, lists=lists)

    return dict(X=side(40, 8, 36), Y=side(5, 2, 37))


def keypose_extents(side):
    return dict(frames=len(side["poses"]), queries=len(side["select"]), ids_per_entry=len(side["poses"]) + max(len(l) for l in side["lists"]))


# ---- 6. the front end ------------------------------------------------------------------------------------------------------
ROWS, COLS = 16, 1800


def ring_and_column(raw):
    """the 2-degree ring and the 0.2-degree column of every raw point"""
    p = np.asarray(raw, np.float64)
    ring = np.rint((np.degrees(np.arctan2(p[:, 2], np.hypot(p[:, 0], p[:, 1]))) + 15.0) / 2.0).astype(np.int64)
    col = (np.rint(np.degrees(np.arctan2(p[:, 1], p[:, 0])) / 0.2).astype(np.int64) + 900) % COLS
    return ring, col


def sparse(raw):
    """every second ring emptied and every third column dropped"""
    ring, col = ring_and_column(raw)
    return np.ascontiguousarray(raw[(ring % 2 == 0) & (col % 3 != 0)])


def fewer_columns(raw):
    """every third column dropped, every ring kept"""
    return np.ascontiguousarray(raw[ring_and_column(raw)[1] % 3 != 0])


@functools.lru_cache(maxsize=None)
def frontend_pair():
    """X: four dense synthetic raw scans.  Y: two others with every second ring emptied and every third column dropped —
    without a neighbouring ring nothing of them survives the segmentation: an empty segmented scan, an outlier cloud
    and empty feature clouds — and a third with all rings and two columns of three, which segments as a scan does."""
    host = importlib.import_module("lins---lidar-inertial-slam_amd.host")
    return dict(X=[host.synth_raw_scan(40 + i, i % 2) for i in range(4)],
                Y=[sparse(host.synth_raw_scan(50 + i, i % 2)) for i in range(2)] + [fewer_columns(host.synth_raw_scan(52, 0))])


def frontend_extents(raws):
    return dict(scans=len(raws), raw_points=sum(len(r) for r in raws), largest_scan=max(len(r) for r in raws))
