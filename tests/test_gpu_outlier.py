"""lins_segment_batch_outliers (csrc/segment_kernels.hip): the outlier cloud from the segmentation kernel equals the host
call (lins_frontend_segment_outliers) bit for bit — order and count included — on both projection paths, and
lins_segment_batch, which runs the same kernel without the emission, still returns what it returned."""
import numpy as np
import pytest

import outlier_cases as oc
import seg_cases as sc
from test_gpu_segmentation import bits, context

pytestmark = pytest.mark.gpu


def repeated_packets(host):
    """more raw points than the 32 768 the point path takes (a driver that repeats packets, as
    tests/test_gpu_edge_cases.py builds it): the cell-by-cell path on a ray-cast scene with many outliers"""
    base = host.synth_raw_scan(3, 1)
    extra = base[np.random.default_rng(11).permutation(len(base))[:14000]].copy()
    extra[:, :3] *= np.float32(1.01)
    return np.ascontiguousarray(np.concatenate([base, extra]))


@pytest.fixture(scope="module")
def inputs(host):
    """name -> raw cloud, in the calls (at most 4 scans each) the device runs them in"""
    stock = {"stock_%d" % i: host.synth_raw_scan(i, i % 2) for i in range(3)}  # three different counts: per-scan offsets
    assert len({len(r) for r in stock.values()}) == 3
    images = {n: oc.image_case(n)["raw"] for n in ("no_outlier", "full", "extreme")}
    big = {"nan_returns": sc.case("nan_returns")["raw"], "cells_32769": sc.case("ownership_rivals_last_32769")["raw"],
           "repeated_packets": repeated_packets(host)}
    assert len(big["cells_32769"]) > 32768 and len(big["repeated_packets"]) > 32768
    return [stock, images, big]


@pytest.fixture(scope="module")
def want(host, inputs):
    return {n: (host.frontend_segment(r), host.frontend_segment_outliers(r)) for call in inputs for n, r in call.items()}


@pytest.fixture(scope="module")
def got(pkg, ieskf, inputs):
    """(with the emission, without it) per name; one context, the calls one after the other — a slot's outlier cloud
    is overwritten by the next call's"""
    out = {}
    with context(pkg, ieskf) as c:
        for call in inputs:
            names = list(call)
            segs, outl = c.segment_batch_outliers([call[n] for n in names])
            plain = c.segment_batch([call[n] for n in names])
            for n, s, o, p in zip(names, segs, outl, plain):
                out[n] = (s, o, p)
    return out


NAMES = ["stock_0", "stock_1", "stock_2", "no_outlier", "full", "extreme", "nan_returns", "cells_32769", "repeated_packets"]


@pytest.mark.parametrize("name", NAMES)
def test_outlier_cloud_equals_the_host_call_bit_for_bit(got, want, name):
    (seg, outl, _), (wseg, woutl) = got[name], want[name]
    assert seg.c.n_outlier == len(outl) == len(woutl) == wseg.c.n_outlier
    assert outl.tobytes() == woutl.tobytes()
    assert bits(seg) == bits(wseg)
    if name == "full":
        assert len(outl) == oc.OUTLIER_MAX
    if name == "no_outlier":
        assert len(outl) == 0
    if name in ("stock_0", "repeated_packets", "cells_32769", "nan_returns"):
        assert len(outl) > 0


@pytest.mark.parametrize("name", NAMES)
def test_segment_batch_still_returns_what_it_returned(got, want, name):
    seg, _, plain = got[name]
    assert bits(plain) == bits(seg) == bits(want[name][0])


def test_images_equal_the_model(got):
    for n in ("no_outlier", "full", "extreme"):
        assert got[n][1].tobytes() == oc.image_case(n)["cloud"].tobytes()


def test_arguments(pkg, ieskf, host):
    import ctypes as C

    two = sc.case("ownership_two_points")["raw"]
    with context(pkg, ieskf) as c:
        L = ieskf.lib()
        P = C.POINTER(host.Point)
        segs, _ = c.segment_batch_outliers([two])  # (sets the argtypes)
        raws = (P * 1)(two.ctypes.data_as(P))
        cnt = (C.c_int32 * 1)(len(two))
        out = (host.SegmentedScanC * 1)(segs[0].c)
        assert L.lins_segment_batch_outliers(c._h, 1, raws, cnt, out, None) == -1
        assert L.lins_segment_batch_outliers(c._h, 1, raws, cnt, out, (P * 1)()) == -1
        assert L.lins_segment_batch_outliers(c._h, 0, None, None, None, None) == 0
