"""lins_frontend_segment_outliers (csrc/host/frontend.cpp): image_projection_node's /outlier_cloud (IP:300-303) on the
host — its count against lins_frontend_segment and the reference's node, its points against the independent libm checker
(oracle/frontend_oracle.cpp fo_segment) and against what tests/seg_cases.py's model implies on built range images."""
import ctypes as C
import os

import numpy as np
import pytest

import outlier_cases as oc
import seg_cases as sc

SEEDS = range(4)
IMG_CASES = [n for n in sc.CASES if n != "nothing_projects"]


@pytest.fixture(scope="module")
def stock(host):
    return [host.synth_raw_scan(i, 1) for i in SEEDS]


def checker_outliers(oracle, raw):
    """fo_segment with its outlier_xyzi output (oracle.fe_segment passes None there)"""
    raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1, 4)
    L = oracle.lib()
    N = oracle.CLOUD_MAX
    cloud, rng, col, ground = np.zeros((N, 4), np.float32), np.zeros(N, np.float32), np.zeros(N, np.uint32), np.zeros(N, np.uint8)
    sr, er, ori, label = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(3, np.float32), np.zeros(N, np.int32)
    outl, nout = np.zeros((N, 4), np.float32), C.c_int32(0)
    L.fo_segment.restype = C.c_int
    L.fo_segment.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
    m = L.fo_segment(raw.ctypes.data, len(raw), cloud.ctypes.data, rng.ctypes.data, col.ctypes.data, ground.ctypes.data,
                     sr.ctypes.data, er.ctypes.data, ori.ctypes.data, C.byref(nout), outl.ctypes.data, label.ctypes.data)
    assert m >= 0, m
    return outl[: nout.value].copy()


def test_constant_and_swap(defs):
    assert defs.OUTLIER_MAX == oc.OUTLIER_MAX == 3600
    c = np.arange(8, dtype=np.float32).reshape(2, 4)
    assert oc.yzx(c).tolist() == [[1, 2, 0, 3], [5, 6, 4, 7]]


def test_count_is_what_the_segmentation_reports(host, stock):
    for raw in stock + [sc.case(n)["raw"] for n in sc.CASES]:
        o = host.frontend_segment_outliers(raw)
        assert len(o) == host.frontend_segment(raw).c.n_outlier
    assert sum(len(host.frontend_segment_outliers(r)) for r in stock) > 100


def test_count_is_the_reference_nodes_outlier_cloud_size(host, stock):
    from oracle import ref

    if not ref.available():
        if os.environ.get("LINS_REQUIRE_REF") == "1":
            pytest.fail("LINS_REQUIRE_REF=1 and oracle/_ref/liblins_ref.so is not there")
        pytest.skip("oracle/_ref/liblins_ref.so is not there and the reference's sources are not here to build it")
    ref.lib()
    for raw in stock + [sc.case(n)["raw"] for n in sc.CASES]:
        assert len(host.frontend_segment_outliers(raw)) == ref.segment(raw).c.n_outlier


def test_points_equal_the_independent_checker_bit_for_bit(host, oracle, stock):
    for raw in stock:
        got, want = host.frontend_segment_outliers(raw), checker_outliers(oracle, raw)
        assert len(got) == len(want) > 0
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", IMG_CASES)
def test_outlier_cells_are_what_the_model_implies(host, name):
    c = sc.case(name)
    want = oc.model_outlier_cloud(c["img"])
    got = host.frontend_segment_outliers(c["raw"])
    assert len(got) == len(want)
    assert got.tobytes() == want.tobytes()


def test_the_three_images_are_what_they_claim(host):
    a, b, c = (oc.image_case(n) for n in ("no_outlier", "full", "extreme"))
    assert len(a["cloud"]) == 0 and sum(s["valid"] for s in a["model"]["segments"].values()) == 1
    assert len(b["cloud"]) == oc.OUTLIER_MAX and all(s["size"] == 1 for s in b["model"]["segments"].values())
    assert min(b["model"]["edge_margin"], c["model"]["edge_margin"]) > 0.01
    cells = oc.model_outlier_cells(c["img"], c["model"])
    assert [(int(x) // sc.COLS, int(x) % sc.COLS) for x in cells] == oc.EXTREME_CELLS
    assert not any(s["valid"] for s in c["model"]["segments"].values())
    for case in (a, b, c):
        got = host.frontend_segment_outliers(case["raw"])
        assert got.tobytes() == case["cloud"].tobytes()
        assert len(got) == host.frontend_segment(case["raw"]).c.n_outlier == case["model"]["n_outlier"]


def test_input_contract(host):
    two = sc.case("ownership_two_points")["raw"]
    L = host.lib()
    host.frontend_segment_outliers(two)
    P = C.POINTER(host.Point)
    buf = np.zeros((oc.OUTLIER_MAX, 4), np.float32)
    assert L.lins_frontend_segment_outliers(two.ctypes.data_as(P), 1, buf.ctypes.data_as(P)) == -1
    assert L.lins_frontend_segment_outliers(two.ctypes.data_as(P), 2, None) == -1
    bad = np.concatenate([two, two])
    bad[:3, 2] = np.nan  # one finite point left
    assert L.lins_frontend_segment_outliers(bad.ctypes.data_as(P), len(bad), buf.ctypes.data_as(P)) == -4
    c = sc.case("nan_returns")
    assert host.frontend_segment_outliers(c["raw"]).tobytes() == host.frontend_segment_outliers(c["clean"]).tobytes()
