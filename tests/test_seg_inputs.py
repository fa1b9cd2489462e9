"""The segmentation cases of tests/seg_cases.py are what they claim, and the three CPU statements of the stage agree on
them: the product's host restatement (csrc/host/frontend.cpp — what tests/test_gpu_segmentation.py holds the device kernel
against, bit for bit), the independent libm checker (oracle/frontend_oracle.cpp) and the reference's own compiled node
(oracle/_ref).  The claims are checked with seg_cases.segment_model: a plain float64 statement of the directed edge set
on the range image, the labels it implies and how far each cell lies from its root.

Conditions on the inputs, so that the comparisons are about logic and not about whose atan2f is used: no edge angle
within 1e-3 rad of segmentTheta, no ground angle within 0.1 deg of 10 deg, no point within 0.02 deg of a column edge or
0.02 of a row from a row boundary."""
import os

import numpy as np
import pytest

import seg_cases as sc
from test_frontend_oracle import assert_same_segmentation

IMAGE_CASES = [n for n in sc.CASES if sc.case(n)["img"] is not None]
_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = sc.segment_model(sc.case(name)["img"])
    return _MODELS[name]


@pytest.fixture(scope="module")
def ref():
    from oracle import ref as r

    if not r.available():
        if os.environ.get("LINS_REQUIRE_REF") == "1":
            pytest.fail("LINS_REQUIRE_REF=1 and oracle/_ref/liblins_ref.so is neither built nor buildable here")
        pytest.skip("oracle/_ref/liblins_ref.so not built and the reference's sources are not present")
    r.lib()
    return r


def as_dict(s):
    """a host.Segmented (the host restatement's, the device's or the reference node's) as oracle.fe_segment's dict"""
    return dict(n=s.n, cloud=s.cloud, range=s.range, col=s.col, ground=s.ground, start_ring=np.array(s.c.start_ring[:]),
                end_ring=np.array(s.c.end_ring[:]), n_outlier=s.c.n_outlier,
                orientation=np.array([s.c.start_ori, s.c.end_ori, s.c.ori_diff], np.float32))


def finite(raw):
    return raw[np.isfinite(raw[:, :3]).all(1)]


def emitted_cells(o):
    """the (row, col) image of what a segmentation emitted: fullCloud's intensity is row + col / 10000 (IP:234)"""
    n = o["n"]
    m = np.zeros((sc.ROWS, sc.COLS), bool)
    m[np.floor(o["cloud"][:n, 3]).astype(int), o["col"][:n].astype(int)] = True
    assert m.sum() == n
    return m


# ---- the inputs meet the conditions -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sc.CASES))
def test_points_sit_mid_cell_and_leave_the_claimed_range_image(name):
    c = sc.case(name)
    p = finite(c["raw"]).astype(np.float64)
    rowf = (np.degrees(np.arctan2(p[:, 2], np.hypot(p[:, 0], p[:, 1]))) + 15.1) / 2.0
    off_boundary = np.abs(rowf[:, None] - np.arange(-1, 17)[None]).min(1)
    assert off_boundary.min() >= 0.02  # of a row (the boundaries that decide anything: -1 .. 16)
    inside = (rowf > -1) & (rowf < 16)
    colf = -np.degrees(np.arctan2(p[:, 0], p[:, 1]) - np.pi / 2) / 0.2 + 900  # IP:224-225 before the rounding
    on_axis = np.hypot(p[:, 0], p[:, 1]) == 0
    assert (np.abs(colf - np.round(colf))[~on_axis] <= 0.4).all()  # 0.02 deg = 0.1 of a column from the edge at +-0.5
    if c["img"] is None:
        assert not inside.any()
        return
    col = np.round(colf).astype(int) % sc.COLS
    img = np.zeros(sc.CELLS)
    cell = np.floor(np.maximum(rowf, 0)).astype(int) * sc.COLS + col
    img[cell[inside]] = np.linalg.norm(p[inside], axis=1)  # (numpy keeps the LAST assignment to a repeated index)
    want = c["img"].ravel()
    assert np.array_equal(img > 0, want > 0)
    assert np.abs(img - want).max() <= 1e-6 * want.max()


@pytest.mark.parametrize("name", IMAGE_CASES)
def test_no_angle_lies_near_its_threshold(name):
    m = model(name)
    assert m["edge_margin"] >= 1e-3  # rad from segmentTheta, over every pair of eligible neighbours
    assert m["ground_margin"] >= 0.1  # deg from 10 deg, over every pair groundRemoval reads


# ---- each case is what it claims -----------------------------------------------------------------------------------------

def test_directed_chains_is_weakly_connected_but_directed():
    c, m = sc.case("directed_chains"), model("directed_chains")
    segs = m["segments"].values()
    assert m["n_components"] * 10 < len(segs) * 7 and len(segs) > 1500  # every class-0 chain hangs on column 0's
    assert max(g["size"] for g in segs) == 32  # (an undirected labelling would make segments of thousands of cells)
    assert {g["size"] for g in segs} == set(c["sizes"])
    for g in segs:
        assert g["valid"] == c["sizes"][g["size"]]
    assert {g["size"]: g["rows"] for g in segs} == {7: 1, 8: 1, 14: 2, 16: 2, 21: 3, 24: 3, 28: 4, 32: 4}
    assert m["n_outlier"] == 6 * 360  # rings 7, 8, 9, 13, 14, 15: every cell invalid, every fifth column counted
    # column 0's chain is reached by every class-0 chain of its row and reaches none of them
    row0 = m["label"][0]
    assert (row0[np.arange(0, 1800, 255)] == 0).all() and row0[3] == 3 and row0[1788] == 3 and m["edges"][1][1788]


def test_seed_row_shapes_are_separate_segments_with_the_stated_validity():
    c, m = sc.case("seed_row"), model("seed_row")
    assert len(m["segments"]) == len(c["placed"]) == 39
    for p in c["placed"]:
        g = m["segments"][p["cells"][0]]
        assert sorted(g["cells"]) == p["cells"] and g["valid"] == p["valid"], p["name"]
    by_name = {p["name"]: m["segments"][p["cells"][0]] for p in c["placed"]}
    assert (by_name["lone_seed_5"]["size"], by_name["lone_seed_5"]["rows"]) == (5, 2)
    assert (by_name["seed_row_shared_5"]["size"], by_name["seed_row_shared_5"]["rows"]) == (5, 3)
    assert {n: by_name[n]["size"] for n in ("line_4", "line_5", "line_29", "line_30")} == dict(line_4=4, line_5=5, line_29=29, line_30=30)
    assert m["n_outlier"] == c["n_outlier"] > 0
    per_band = [sum(1 for p in c["placed"] if p["band"] == b and not p["valid"] for x in p["cells"] if x // sc.COLS > 5 and x % 5 == 0)
                for b in range(3)]
    assert per_band[0] == 0 and per_band[1] > per_band[2] > 0  # (the single-column shapes count in the aligned band only)


def test_serpentine_is_one_segment_many_hundred_thread_runs_deep():
    c, m = sc.case("serpentine"), model("serpentine")
    assert len(m["segments"]) == 1 and m["segments"][0]["size"] == sc.CELLS and m["segments"][0]["valid"]
    deepest = int(m["depth"].max())
    assert deepest >= c["min_depth"] == 500
    assert deepest == 812  # what this construction gives; the kernel's cap is 4096 sweeps (bound: 2288, see its comment)
    assert np.unravel_index(m["depth"].argmax(), m["depth"].shape)[0] == 15


def test_ownership_orders_leave_different_images_and_segmentations(oracle):
    last, first = sc.case("ownership_rivals_last_32768"), sc.case("ownership_rivals_first")
    assert len(last["raw"]) == 32768 and len(sc.case("ownership_rivals_last_32769")["raw"]) == 32769
    assert len(first["raw"]) % 4 != 0 and len(sc.case("ownership_two_points")["raw"]) == 2
    a, b = emitted_cells(oracle.fe_segment(last["raw"])), emitted_cells(oracle.fe_segment(first["raw"]))
    assert b.sum() == 14400 and b[6:14].all()
    assert not a.ravel()[last["contested"]].any() and (a != b).sum() >= 300


def test_ground_holes_marks_what_it_says():
    c, m = sc.case("ground_holes"), model("ground_holes")
    g = m["ground"]
    assert g[:6, 50].all() and not g[6:, :].any()
    for col, ring in sc.GROUND_HOLES:
        want = np.ones(6, bool)
        want[ring] = False
        if ring >= 1:
            want[ring - 1] = False  # groundMat -1 for the pair with the hole on top, over what the pair below left
        if ring == 4:
            want[5] = False  # ring 5 has no pair of its own
        assert np.array_equal(g[:6, col], want), (col, ring)
    assert g[:6, 701:703].all() and not g[2:6, 700].any() and not g[2:6, 703:733].any()
    lone = m["segments"][c["lone_column"][0]]
    assert sorted(lone["cells"]) == c["lone_column"] and not lone["valid"]
    assert m["segments"][2 * sc.COLS + 703]["size"] == 120 and not m["emitted"][2:6, 700].any() and m["emitted"][2:6, 703:733].all()
    kept = m["emitted"][0]
    assert kept[:6].sum() == 5 and kept[1795:].sum() == 4 and kept[6:1795].sum() == (np.arange(6, 1795) % 5 == 0).sum() - 2  # (less the holes)


# ---- the three CPU statements agree ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sc.CASES))
def test_host_restatement_and_checker_agree_and_match_the_model(host, oracle, name):
    c = sc.case(name)
    o = oracle.fe_segment(c["raw"])
    assert_same_segmentation(o, host.frontend_segment(c["raw"]))
    if c["img"] is None:
        assert o["n"] == 0 and (o["start_ring"] == 4).all() and (o["end_ring"] == -6).all() and (o["label"] == -1).all()
        return
    m = model(name)
    assert np.array_equal(o["label"], m["oracle_label"])
    assert np.array_equal(emitted_cells(o), m["emitted"]) and o["n_outlier"] == m["n_outlier"]


@pytest.mark.parametrize("name", list(sc.CASES))
def test_host_restatement_agrees_with_the_references_node(host, ref, name):
    raw = sc.case(name)["raw"]
    assert_same_segmentation(as_dict(ref.segment(raw)), host.frontend_segment(raw))


def test_non_finite_returns_behave_as_if_they_were_not_in_the_cloud(host, oracle):
    """removeNaNFromPointCloud (IP:176): the expected result is the segmentation of the cloud with those points deleted,
    the orientations (first, last and second-to-last REMAINING point) included — for the host restatement bit for bit"""
    c = sc.case("nan_returns")
    raw, clean = c["raw"], c["clean"]
    assert len(raw) == len(clean) + 9 and np.array_equal(finite(raw), clean)
    got, want = host.frontend_segment(raw), host.frontend_segment(clean)
    assert_same_segmentation(oracle.fe_segment(clean), got)
    assert np.isfinite(got.cloud[: got.n]).all() and np.isfinite(got.range[: got.n]).all()
    assert (got.c.start_ori, got.c.end_ori, got.c.ori_diff) == (want.c.start_ori, want.c.end_ori, want.c.ori_diff)
    assert as_dict(got)["orientation"].tobytes() == as_dict(want)["orientation"].tobytes()
    # a single coordinate is enough, whichever it is — and infinities are dropped by the host restatement like NaN
    for k, bad in ((0, np.nan), (1, np.nan), (2, np.nan), (0, np.inf), (2, -np.inf)):
        r = np.insert(clean, [0, 7000, len(clean)], np.zeros((3, 4), np.float32), axis=0)
        r[[0, 7001, -1], :3] = sc.points_of([7 * sc.COLS + 1350], [9.0])[0, :3]
        r[[0, 7001, -1], k] = bad
        assert_same_segmentation(as_dict(want), host.frontend_segment(r))


def test_fewer_than_two_finite_points_is_an_input_error(host, pkg):
    raw = sc.case("ownership_two_points")["raw"]
    for n_nan in (1, 2):
        r = np.concatenate([raw, raw])
        r[:2 + n_nan, n_nan] = np.nan  # 1 or 0 finite points left of 4
        with pytest.raises(RuntimeError, match="-4"):  # LINS_E_INPUT
            host.frontend_segment(r)
    assert host.frontend_segment(np.concatenate([raw, raw * np.float32(np.nan)])).n == 0  # two finite points: accepted
