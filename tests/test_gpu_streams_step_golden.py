"""The device-resident streams step (csrc/lins_capi_streams.hip) against tests/golden/streams_step_parent_bits.npz: the
bits the library gave before the step was split into phases and took the batch path's update launcher
(tests/golden/make_streams_step_golden.py, recorded on an MI355X).  The scenarios of tests/streams_step_cases.py cover
every mode of the step — prior given (each kernel family, the any-size kernel among them; raw clouds), prior from the
device filter with a gated scan, the state machine, the divergence fall-back — and everything a call returns or leaves
resident has to be the same, bit for bit."""
import os

import numpy as np
import pytest

import streams_step_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streams_step_parent_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(cases.SCENARIOS))
def test_streams_step_leaves_the_parents_bits(pkg, host, ieskf, golden, name):
    got = cases.SCENARIOS[name](pkg, host, ieskf)
    want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
    assert want and sorted(got) == sorted(want)
    for key in sorted(got):
        g, w = got[key], want[key]
        assert g.dtype == w.dtype and g.shape == w.shape, key
        diff = np.argwhere(g != w)
        assert len(diff) == 0, (name, key, f"{len(diff)} of {g.size} values differ, first at {tuple(diff[0])}")
