"""The VoxelGrid radix sort of local_map_kernels.hip at the shapes no other test reaches (tests/mapping_state_cases.py
builds them, tests/test_mapping_state_inputs.py asserts what they are): one batch whose jobs need 0, 1, 2, 3 and 4
passes at once — every early-return branch live in one launch, a key of 31 bits, the result in either key buffer —,
input counts on the 512-point tile and the 64-lane wave, a voxel run over a tile edge, 600 copies of one point, and
points on voxel faces at negative coordinates.  lins_local_map_build against the CPU restatement (host.local_map), bit
for bit on the six clouds and the size records, and the scan clouds against the numpy VoxelGrid (local_map_np)."""
import numpy as np
import pytest

import local_map_np as lnp
import mapping_state_cases as mc

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture
def ctx(pkg, ieskf):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    yield c
    c.close()


def build(ctx, entries, slots=None, max_pts=8192):
    """a fresh ring per entry (slot k = entry k unless said), one build -> [(sizes, six clouds)]"""
    slots = list(range(len(entries))) if slots is None else slots
    ctx.local_map_init(len(entries), 50, max_pts)
    for s, (frames, _) in zip(slots, entries):
        for f in frames:
            ctx.local_map_push(s, *f)
    sizes = ctx.local_map_build(slots, [sc for _, sc in entries])
    return [(sizes[k], [ctx.local_map_download(k, c) for c in range(6)]) for k in range(len(entries))]


def assert_entry(host, what, got, frames, scan):
    """one entry against host.local_map (six clouds and the size record) and the numpy VoxelGrid (the scan clouds)"""
    sizes, clouds = got
    want, ws = host.local_map(frames, scan, 50)
    assert sizes == ws, (what, sizes, ws)
    nbytes = 0
    for c in range(6):
        assert clouds[c].shape == want[c].shape and np.array_equal(bits(clouds[c]), bits(want[c])), (what, c)
        nbytes += clouds[c].nbytes
    for c, (cloud, leaf) in zip((2, 3, 4), ((scan[0], 0.2), (scan[1], 0.4), (scan[2], 0.4))):
        assert np.array_equal(bits(clouds[c]), bits(lnp.voxel_grid(cloud, leaf))), (what, c)
    print("%s: 6 clouds, %d bytes, sizes %s = host.local_map; 3 scan clouds = numpy VoxelGrid" % (what, nbytes, sizes["n"]))
    return nbytes


def same(a, b):
    return a[0] == b[0] and all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a[1], b[1]))


def test_a_batch_whose_jobs_need_every_pass_count(ctx, host):
    entries = mc.pass_entries()
    passes = [[j[2] for j in mc.entry_passes(fr, sc)] for fr, sc in entries]
    assert {p for e in passes for p in e} == {0, 1, 2, 3, 4}
    got = build(ctx, entries)
    for k, (frames, scan) in enumerate(entries):
        assert_entry(host, "batch entry %d (passes %s)" % (k, passes[k]), got[k], frames, scan)
    assert [g[0]["status"] for g in got] == [0, 0, 0]
    assert got[1][0]["n"][2] > 500 and got[2][0]["n"][0] > 500  # the 31-bit jobs: (nearly) every point its own voxel


def test_the_same_jobs_one_entry_per_call(ctx, host):
    entries = mc.pass_entries()
    batch = build(ctx, entries)
    for k, (frames, scan) in enumerate(entries):
        alone = build(ctx, [entries[k]])[0]
        assert same(alone, batch[k]), k
        assert_entry(host, "entry %d alone" % k, alone, frames, scan)
    print("3 entries alone = the batch's: 18 clouds and 3 size records, bit for bit")


def test_counts_on_the_tile_and_the_wave_and_a_run_over_a_tile_edge(ctx, host):
    entries = mc.edge_entries() + [mc.straddle_entry()]
    got = build(ctx, entries)
    for k, (frames, scan) in enumerate(entries):
        what = "count %d" % mc.EDGE_COUNTS[k] if k < len(mc.EDGE_COUNTS) else "straddling run"
        assert_entry(host, what, got[k], frames, scan)
    straddle = got[-1]
    assert straddle[0]["n"][2] == straddle[0]["n"][3] == 1023  # 1024 points, one run of two
    for k in range(len(entries)):  # ... and each alone
        assert same(build(ctx, [entries[k]])[0], got[k]), k


def test_duplicated_points_give_one_voxel_and_the_exact_centroid(ctx, host):
    frames, scan = mc.duplicate_entry()
    got = build(ctx, [(frames, scan)])[0]
    assert_entry(host, "600 copies of one point", got, frames, scan)
    assert got[0]["n"] == [1] * 6
    for c in range(6):
        assert got[1][c].tobytes() == mc.DUP_POINT.tobytes(), c


def test_points_on_voxel_faces_at_negative_coordinates(ctx, host):
    frames, scan = mc.face_entry()
    got = build(ctx, [(frames, scan)])[0]
    assert_entry(host, "lattice of multiples of 0.2 in -3.2 .. 0", got, frames, scan)
    assert got[0]["n"][2] > 4000 and got[0]["box_min"][0] == [-4, -4, -4]
