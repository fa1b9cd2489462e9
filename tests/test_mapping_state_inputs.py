"""What tests/test_gpu_mapping_state.py and tests/test_gpu_sort_shapes.py rest on, asserted from numpy alone
(tests/mapping_state_cases.py builds the inputs and restates the C API's sizing):

  every warm-up X is STRICTLY larger than its call under test Y in every dimension an allocation is sized by — what
  keeps a stale read of a broken kernel inside memory X wrote;
  the sort cases hold VoxelGrid jobs of 0, 1, 2, 3 and 4 radix passes, one of exactly 31 bits;
  the tile-edge cases have the counts they claim, and the straddling run lies where it is said to lie."""
import numpy as np

import local_map_np as lnp
import mapping_state_cases as mc


def show(name, x, y):
    print("%s:" % name)
    for k in x:
        print("    %-18s X %9d   Y %9d" % (k, x[k], y[k]))


def assert_larger(name, x, y):
    show(name, x, y)
    assert mc.strictly_larger(x, y) == [], (name, mc.strictly_larger(x, y))


def test_every_warm_up_is_strictly_larger_in_every_grow_only_dimension():
    p = mc.ring_pair()
    assert_larger("ring build", mc.build_extents(mc.ring_entries(p["X"]), window=mc.RING["window"]),
                  mc.build_extents(mc.ring_entries(p["Y"]), window=mc.RING["window"]))
    p = mc.ring_pass_pair()
    assert_larger("ring build, reverse mix of pass counts", mc.build_extents(mc.ring_entries(p["X"])), mc.build_extents(mc.ring_entries(p["Y"])))
    p = mc.surround_pair()
    x = mc.build_extents(mc.surround_entries(p["X"]), chunk=mc.SURROUND_CHUNK)
    y = mc.build_extents(mc.surround_entries(p["Y"]), chunk=mc.SURROUND_CHUNK)
    assert_larger("surround build, chunk %d" % mc.SURROUND_CHUNK, x, y)
    assert (x["split_jobs"], y["split_jobs"]) == (6, 2) and y["chunks"] == 4 + 2  # fewer split jobs, fewer chunks
    unsplit = mc.build_extents(mc.surround_entries(p["Y"]), chunk=mc.INT_MAX)
    assert unsplit["split_jobs"] == 0 and unsplit["chunks"] == 0
    assert_larger("surround build, Y without a split", x, unsplit)
    p = mc.assembly_pair()
    x, y = mc.assembly_extents(p["X"]), mc.assembly_extents(p["Y"])
    assert y["chunks"] == 0 and x["chunks"] > 0  # (at the default chunk the warm-up's scans are split, Y's are not)
    assert_larger("archive assembly", x, dict(y, chunks=-1))
    p = mc.map_pair()
    x = mc.problem_extents(p["X"])
    assert_larger("scan-to-map, explicit", x, mc.problem_extents(p["Y"]))
    assert_larger("scan-to-map, LINS_MAP_LOCAL after the explicit X", x, mc.map_local_extents())
    p = mc.icp_pair()
    assert_larger("loop ICP", mc.icp_extents(p["X"]), mc.icp_extents(p["Y"]))
    assert_larger("loop ICP, correspondences of Y's accepted problem", mc.icp_extents(p["X"]), mc.icp_extents(p["Y"][:1]))
    p = mc.keypose_pair()
    assert_larger("key-pose selection", mc.keypose_extents(p["X"]), mc.keypose_extents(p["Y"]))
    p = mc.frontend_pair()
    assert_larger("front end", mc.frontend_extents(p["X"]), mc.frontend_extents(p["Y"]))


def test_the_history_cases_are_what_they_claim():
    p = mc.ring_pair()
    assert [len(p["X"]["frames"][s]) for s in range(3)] == [12, 12, 12]
    assert all(1400 <= sum(len(c) for c in f[:3]) <= 1600 for s in range(3) for f in p["X"]["frames"][s])
    ys = p["Y"]["scans"]
    assert p["Y"]["frames"][5] == [] and all(len(c) == 0 for c in ys[0])  # an empty ring, empty scan clouds
    assert mc.pass_count(ys[1][0], 0.2)[1] is None and lnp.voxel_grid(ys[1][0], 0.2) is None  # refused: more than 2^31 cells
    assert len(ys[2][1]) == mc.TILE
    # the reverse mix: four passes in every job of X, none or one in every job of Y
    p = mc.ring_pass_pair()
    for side, allowed in (("X", {4}), ("Y", {0, 1})):
        got = [[j[2] for j in mc.entry_passes(fr, sc)] for fr, sc in mc.ring_entries(p[side])]
        print("reverse mix, passes per job of %s: %s" % (side, got))
        assert {v for e in got for v in e} <= allowed and (side == "X" or {v for e in got for v in e} == {0, 1}), (side, got)
    # the front end's Y: every second ring empty, every third column dropped
    fy = mc.frontend_pair()["Y"]
    for raw in fy[:2]:
        ring, col = mc.ring_and_column(raw)
        assert len(raw) > 1000 and not (ring % 2).any() and (col % 3 != 0).all()
    ring, col = mc.ring_and_column(fy[2])  # ... and one with every ring and two columns of three
    assert set(ring.tolist()) >= set(range(16)) and (col % 3 != 0).all()
    # scan-to-map's Y lies in smaller boxes than X's
    m = mc.map_pair()
    assert max(mc.cells_of(q.map_surf) for q in m["Y"]) < min(mc.cells_of(q.map_surf) for q in m["X"])
    assert len({(len(q.map_corner), len(q.map_surf)) for q in m["Y"]}) == 2  # (swapped, their sizes differ from the resident ones)
    i = mc.icp_pair()
    assert all(2800 <= len(s) <= 3400 for s, _ in i["X"]) and len(i["Y"][0][0]) == 300 and mc.cells_of(mc.WIDE) > 2 * (1 << 26)


def test_the_sort_cases_cover_every_pass_count():
    for name, (p02, p04) in mc.BOX_PASSES.items():
        c = mc.box_cloud(name, 600, 1)
        got = [mc.pass_count(c, leaf) for leaf in (0.2, 0.4)]
        print("box %-9s leaf 0.2: %11d cells %2d bits %d passes   leaf 0.4: %10d cells %2d bits %d passes" % ((name,) + got[0] + got[1]))
        assert (got[0][2], got[1][2]) == (p02, p04), (name, got)
    assert [mc.pass_count(mc.box_cloud(n, 600, 1), 0.2)[0] for n in ("one cell", "metre", "room", "plain")] == [1, 180, 472781, 2000400020]
    assert [mc.pass_count(mc.box_cloud(n, 600, 1), 0.4)[0] for n in ("one cell", "metre", "room")] == [1, 27, 62016]
    covered, bits31 = set(), 0
    for k, (frames, scan) in enumerate(mc.pass_entries()):
        for name, (ncell, bits, passes), (cloud, _) in zip(mc.JOB_NAMES, mc.entry_passes(frames, scan), mc.job_inputs(frames, scan)):
            print("entry %d %-12s %5d points %11d cells %2d bits %d passes" % (k, name, len(cloud), ncell, bits, passes))
            covered.add(passes)
            bits31 += bits == 31 and passes == 4
        assert all(len(c) <= 900 for c, _ in mc.job_inputs(frames, scan))  # a few hundred points a job
    print("pass counts covered:", sorted(covered))
    assert covered == {0, 1, 2, 3, 4} and bits31 >= 1
    # the identity pose keeps the extents: the map jobs see the boxes as built
    fr = mc.pass_entries()[2][0]
    assert lnp.transform(fr[0][0], mc.ID).tobytes() == fr[0][0].tobytes()
    # the 31-bit box goes through the numpy VoxelGrid; it stays inside the input contract and scan-to-map's 2^26-cell box
    plain = mc.box_cloud("plain", 600, 9)
    assert lnp.voxel_grid(plain, 0.2) is not None and np.abs(plain[:, :3]).max() <= 1e6 and mc.cells_of(plain) <= 2 * ((1 << 26) + 1)


def test_the_tile_edge_cases_have_the_stated_counts():
    assert mc.EDGE_COUNTS == (512, 513, 1024, 64, 65) == (mc.TILE, mc.TILE + 1, 2 * mc.TILE, mc.WAVE, mc.WAVE + 1)
    for n, (frames, scan) in zip(mc.EDGE_COUNTS, mc.edge_entries()):
        counts = [len(c) for c, _ in mc.job_inputs(frames, scan)[:5]]
        print("count %4d: job inputs %s, runs of more than one point at leaf 0.2: %d" % (n, counts, n - len(lnp.voxel_grid(scan[0], 0.2))))
        assert counts == [n] * 5
        assert len(lnp.voxel_grid(scan[0], 0.2)) < n  # (some runs of several points)
    for leaf in (0.2, 0.4):
        c = mc.straddle_cloud(leaf)
        key = np.sort(mc.voxel_keys(c, leaf), kind="stable")
        assert len(c) == 2 * mc.TILE
        # positions 511 and 512 hold one voxel, their neighbours others: the run begins in the last lane of tile 0 and
        # ends in the first lane of tile 1
        assert key[mc.TILE - 2] != key[mc.TILE - 1] == key[mc.TILE] != key[mc.TILE + 1]
        assert np.count_nonzero(np.diff(key) == 0) == 1 and not np.array_equal(mc.voxel_keys(c, leaf), key)
    d = mc.duplicate_entry()[1][0]
    assert len(d) == 600 and lnp.voxel_grid(d, 0.2).tobytes() == mc.DUP_POINT.tobytes()  # one voxel, the exact centroid
    lat = mc.face_lattice()
    assert len(lat) == 17 ** 3 and lat[:, :3].max() == 0 and lat[:, :3].min() == np.float32(-3.2)
    assert np.array_equal(lat[:, :3], (np.rint(lat[:, :3].astype(np.float64) / 0.2) * 0.2).astype(np.float32))  # multiples of 0.2
