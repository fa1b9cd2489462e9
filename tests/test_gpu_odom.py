"""The odometry records on the device (include/lins_streams_slam.h lins_streams_odometry; csrc/odom_kernels.hip): the case
set of tests/odom_cases.py loaded as global states with lins_streams_filter_set, in batches of 65 streams (a second wave
with one lane), against the host restatement and the numpy.longdouble route; a record's bits do not depend on its lane
or on the batch size."""
import importlib

import numpy as np
import pytest

import filter_common as fc
import odom_cases as oc
import odom_np as on

pytestmark = pytest.mark.gpu
PKG = "lins---lidar-inertial-slam_amd"
BATCH = 65


@pytest.fixture(scope="module")
def sl():
    return importlib.import_module(PKG + ".streams_slam")


def context(pkg, ieskf, n):
    return ieskf.IeskfContext(pkg.default_params(num_iter=8), max_batch=n, max_targets=16384)


@pytest.fixture(scope="module")
def device_records(pkg, ieskf, host, sl):
    """the device's record of every case: batches of 65 global states (the last one filled up with the identity)"""
    states = list(oc.STATES)
    while len(states) % BATCH:
        states.append(oc.STATES[0])
    filt = fc.new_filter(host)[0]
    out = []
    with context(pkg, ieskf, BATCH) as c:
        c.streams_init(BATCH)
        before = sl.odometry(c)  # no stream has been given a filter
        for lo in range(0, len(states), BATCH):
            for k in range(BATCH):
                c.streams_filter_set(k, filt, states[lo + k])
            out += sl.odometry(c)
    return before, out[:len(oc.CASES)]


@pytest.fixture(scope="module")
def host_records(sl):
    return [sl.host_odom_from_global(g) for g in oc.STATES]


def test_streams_without_a_global_state_are_not_valid(device_records):
    before, _ = device_records
    assert len(before) == BATCH
    for r in before:
        assert r["valid"] == 0 and not r["position"].any() and not r["orientation"].any() and not r["transform_sum"].any()


def test_pose_and_translation_are_the_hosts_bits(device_records, host_records):
    _, dev = device_records
    for (name, _), d, h in zip(oc.CASES, dev, host_records):
        assert d["valid"] == h["valid"] == 1, name
        assert np.array_equal(oc.bits64(d["position"]), oc.bits64(h["position"])), name
        assert np.array_equal(oc.bits64(d["orientation"]), oc.bits64(h["orientation"])), name
        assert np.array_equal(oc.bits32(d["transform_sum"][3:]), oc.bits32(h["transform_sum"][3:])), name


def test_angles_are_the_hosts_or_an_adjacent_float(device_records, host_records):
    """the two sides differ by ocml's and glibc's last place in f64 only, which survives the rounding to f32 next to a
    rounding boundary: every angle equal or adjacent, at most 1 % not identical"""
    _, dev = device_records
    d = np.stack([r["transform_sum"][:3] for r in dev])
    h = np.stack([r["transform_sum"][:3] for r in host_records])
    differ = int((oc.bits32(d) != oc.bits32(h)).sum())
    print("transform_sum angles: %d of %d differ from the host's bits" % (differ, d.size))
    assert oc.adjacent_or_equal32(d, h).all()
    assert differ <= 0.01 * d.size


def test_angles_against_the_longdouble_composition(device_records):
    _, dev = device_records
    worst = max(on.sum_rotation_error(r["transform_sum"], r["orientation"]) for r in dev)
    print("device transform_sum against the longdouble composition: %.3e (E_host %.3e)" % (worst, oc.E_HOST_SUM))
    assert worst <= 4 * oc.E_HOST_SUM


def test_a_records_bits_do_not_depend_on_lane_or_batch_size(pkg, ieskf, host, sl, device_records):
    """n = 1 against lane 64 of 65"""
    _, dev = device_records
    with context(pkg, ieskf, 1) as c:
        c.streams_init(1)
        c.streams_filter_set(0, fc.new_filter(host)[0], oc.STATES[BATCH - 1])
        one = sl.odometry(c)[0]
    lane64 = dev[BATCH - 1]
    assert one["valid"] == lane64["valid"] == 1
    for f in ("position", "orientation"):
        assert np.array_equal(oc.bits64(one[f]), oc.bits64(lane64[f])), f
    assert np.array_equal(oc.bits32(one["transform_sum"]), oc.bits32(lane64["transform_sum"]))


def test_a_non_finite_global_state_is_not_valid(pkg, ieskf, host, sl):
    """lins_streams_filter_set does not look at the 19 numbers: the kernel does"""
    with context(pkg, ieskf, 2) as c:
        c.streams_init(2)
        bad = oc.STATES[20].copy()
        bad[7] = np.nan
        c.streams_filter_set(0, fc.new_filter(host)[0], bad)
        c.streams_filter_set(1, fc.new_filter(host)[0], oc.STATES[20])
        r = sl.odometry(c)
        assert r[0]["valid"] == 0 and not r[0]["transform_sum"].any() and r[1]["valid"] == 1
