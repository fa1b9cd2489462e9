"""segment_kernel (csrc/segment_kernels.hip) on range images built to decide what ray-cast scenes never decide
(tests/seg_cases.py; tests/test_seg_inputs.py shows that the cases are what they claim and that the CPU statements agree
on them): the directed edges and the many-to-one wrap to column 0, the seed's own row, the 5 .. 29-cell window, a label
that crosses 812 thread runs one after the other, the last point of a cell owning it on both projection paths, ground
columns with holes, a cloud of which nothing projects, and NaN returns.  Bit for bit against the host restatement; against
the independent checker and the reference's node with the orientation allowance of test_frontend_oracle.py."""
import os

import numpy as np
import pytest

import seg_cases as sc
from test_frontend_oracle import assert_same_segmentation
from test_seg_inputs import as_dict

pytestmark = pytest.mark.gpu

NAMES = list(sc.CASES)


@pytest.fixture(scope="module")
def ref():
    from oracle import ref as r

    if not r.available():
        if os.environ.get("LINS_REQUIRE_REF") == "1":  # (the default on a GPU box, tests/conftest.py)
            pytest.fail("LINS_REQUIRE_REF=1 and oracle/_ref/liblins_ref.so did not travel with the snapshot")
        pytest.skip("oracle/_ref/liblins_ref.so did not travel and the reference's sources are not here to build it")
    r.lib()
    return r


def bits(s):
    """everything a segmentation hands on, as bytes"""
    n = s.n
    return (n, s.cloud[:n].tobytes(), s.range[:n].tobytes(), s.col[:n].tobytes(), s.ground[:n].tobytes(),
            tuple(s.c.start_ring), tuple(s.c.end_ring), as_dict(s)["orientation"].tobytes(), s.c.n_outlier)


def context(pkg, ieskf):
    return ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)


@pytest.fixture(scope="module")
def want(host):
    return {name: host.frontend_segment(sc.case(name)["raw"]) for name in NAMES}


@pytest.fixture(scope="module")
def batch(pkg, ieskf):
    """all cases in one call: the 32 769-point scan (cell-by-cell path) sits between scans of the point path"""
    with context(pkg, ieskf) as c:
        return dict(zip(NAMES, c.segment_batch([sc.case(name)["raw"] for name in NAMES])))


@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_host_restatement_bit_for_bit(batch, want, name):
    g, w = batch[name], want[name]
    assert g.n == w.n and g.c.n_outlier == w.c.n_outlier
    assert list(g.c.start_ring) == list(w.c.start_ring) and list(g.c.end_ring) == list(w.c.end_ring)
    assert (g.c.start_ori, g.c.end_ori, g.c.ori_diff) == (w.c.start_ori, w.c.end_ori, w.c.ori_diff)
    n = w.n
    assert np.array_equal(g.cloud[:n], w.cloud[:n]) and np.array_equal(g.range[:n], w.range[:n])
    assert np.array_equal(g.col[:n], w.col[:n]) and np.array_equal(g.ground[:n], w.ground[:n])
    assert bits(g) == bits(w)
    if name == "nothing_projects":
        assert n == 0 and set(g.c.start_ring) == {4} and set(g.c.end_ring) == {-6}


@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_independent_checker_and_the_references_node(batch, oracle, ref, name):
    raw = sc.case(name)["raw"]
    assert_same_segmentation(oracle.fe_segment(raw), batch[name])
    assert_same_segmentation(as_dict(ref.segment(raw)), batch[name])


def test_non_finite_returns_are_dropped_on_the_device(pkg, ieskf, batch, want, host):
    """the NaN case gives the bits of the same cloud without those points; infinities stay LINS_E_INPUT; fewer than two
    finite points are LINS_E_INPUT too, and the context stays usable"""
    c = sc.case("nan_returns")
    assert bits(batch["nan_returns"]) == bits(host.frontend_segment(c["clean"])) == bits(want["nan_returns"])
    two = sc.case("ownership_two_points")["raw"]
    inf = c["clean"].copy()
    inf[1234, 1] = np.inf
    one_left = np.concatenate([two, two])
    one_left[:3, 2] = np.nan
    with context(pkg, ieskf) as ctx:
        for bad in (inf, one_left):
            with pytest.raises(RuntimeError, match="-4"):
                ctx.segment_batch([two, bad])
        got = ctx.segment_batch([np.concatenate([two * np.float32(np.nan), two]), c["raw"]])
        assert bits(got[0]) == bits(want["ownership_two_points"]) and bits(got[1]) == bits(want["nan_returns"])


def test_results_do_not_depend_on_the_batch_the_slot_or_the_context(pkg, ieskf, batch, want):
    """The same bits per case from: all cases in one call; that call in reversed order; each case alone in a fresh
    context; a case run in the slot that just held `serpentine` (seg_rows is zeroed at segment roots only and cellidx is
    per slot: a stale word must never be read)."""
    raws = {name: sc.case(name)["raw"] for name in NAMES}
    with context(pkg, ieskf) as c:
        backwards = dict(zip(NAMES[::-1], c.segment_batch([raws[name] for name in NAMES[::-1]])))
    alone = {}
    for name in NAMES:
        with context(pkg, ieskf) as c:
            alone[name] = c.segment_batch([raws[name]])[0]
    after = {}
    with context(pkg, ieskf) as c:
        for name in NAMES:
            assert bits(c.segment_batch([raws["serpentine"]])[0]) == bits(want["serpentine"])
            after[name] = c.segment_batch([raws[name]])[0]
    for name in NAMES:
        w = bits(want[name])
        assert bits(batch[name]) == w, name
        assert bits(backwards[name]) == w, name
        assert bits(alone[name]) == w, name
        assert bits(after[name]) == w, name


def test_feature_stage_on_the_device_output(pkg, ieskf, host, batch, want):
    names = ["directed_chains", "ground_holes", "nothing_projects"]
    with context(pkg, ieskf) as c:
        feats = c.extract_features_batch([batch[name] for name in names])
    for name, f in zip(names, feats):
        ref = host.frontend_extract_segmented(want[name])
        for k in ("corner_sharp", "corner_less_sharp", "surf_flat", "surf_less_flat"):
            assert np.array_equal(f[k], ref[k]), (name, k)
        assert (f["n_segmented"], f["n_outlier"]) == (want[name].n, want[name].c.n_outlier)
