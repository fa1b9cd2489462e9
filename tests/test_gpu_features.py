"""frontend_kernel (csrc/frontend_kernels.hip) on segmented scans built to decide one rule each (tests/fe_cases.py;
tests/test_fe_inputs.py shows that the cases are what they claim and that the CPU statements agree on them): all four
feature clouds bit for bit against the host restatement — shapes, order and tags — in any batch order, alone, and on a
context that first ran stock scans; against the independent checker with the bars of test_frontend_oracle.py.

The resident path (raw cloud -> segmentation -> feature stage on the device) is not repeated here: the cases choose the
range array, the columns and the coordinates independently of each other, which no raw cloud segments to; that path is
covered by test_gpu_segmentation.py::test_feature_stage_on_the_device_output."""
import numpy as np
import pytest

import fe_cases as fc
from test_fe_inputs import CLOUDS, segmented
from test_frontend_oracle import assert_same_features

pytestmark = pytest.mark.gpu

NAMES = list(fc.CASES)


def bits(f):
    return tuple((f[k].shape, f[k].tobytes()) for k in CLOUDS) + (f["n_segmented"], f["n_outlier"])


def context(pkg, ieskf):
    return ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)


@pytest.fixture(scope="module")
def segs(host):
    return {name: segmented(host, fc.case(name)) for name in NAMES}


@pytest.fixture(scope="module")
def want(host, segs):
    return {name: host.frontend_extract_segmented(segs[name]) for name in NAMES}


@pytest.fixture(scope="module")
def batch(pkg, ieskf, segs):
    with context(pkg, ieskf) as c:
        return dict(zip(NAMES, c.extract_features_batch([segs[name] for name in NAMES])))


@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_host_restatement_bit_for_bit(batch, want, name):
    g, w = batch[name], want[name]
    for k in CLOUDS:
        assert g[k].shape == w[k].shape, k
        assert np.array_equal(g[k][:, :3].view(np.int32), w[k][:, :3].view(np.int32)), k  # points, order
        assert np.array_equal(g[k][:, 3].view(np.int32), w[k][:, 3].view(np.int32)), k  # tags
    assert bits(g) == bits(w)


@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_independent_checker(batch, oracle, name):
    # (the checker breaks ties by index as the product does: the tie cases are compared in full as well)
    assert_same_features(oracle.fe_features(fc.case(name)), batch[name])


def test_results_do_not_depend_on_the_batch_the_order_or_the_context(pkg, ieskf, host, segs, want, batch):
    """the same bits per case from: one batch; that batch reversed; shuffled; each case alone in a fresh context; a
    context that first ran stock scans (a full-size scan leaves every LDS and arena word of the stage used)"""
    shuffled = [NAMES[i] for i in np.random.default_rng(11).permutation(len(NAMES))]
    runs = {}
    with context(pkg, ieskf) as c:
        runs["reversed"] = dict(zip(NAMES[::-1], c.extract_features_batch([segs[n] for n in NAMES[::-1]])))
        runs["shuffled"] = dict(zip(shuffled, c.extract_features_batch([segs[n] for n in shuffled])))
    runs["alone"] = {}
    for name in NAMES:
        with context(pkg, ieskf) as c:
            runs["alone"][name] = c.extract_features_batch([segs[name]])[0]
    stock = [host.frontend_segment(host.synth_raw_scan(30 + i, i % 2)) for i in range(3)]
    with context(pkg, ieskf) as c:
        got = c.extract_features_batch(stock)
        for s, f in zip(stock, got):
            assert bits(f) == bits(host.frontend_extract_segmented(s))
        runs["after_stock"] = dict(zip(NAMES, c.extract_features_batch([segs[n] for n in NAMES])))
    for name in NAMES:
        w = bits(want[name])
        assert bits(batch[name]) == w, name
        for how, r in runs.items():
            assert bits(r[name]) == w, (how, name)
