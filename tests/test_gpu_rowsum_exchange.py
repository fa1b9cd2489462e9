"""wave_reduce_rows (ieskf_rowsum.h) with its two top levels as in-place lane swaps of the pair (lower half, upper
half): the routing of every lane into every sum, partially filled waves, the number classes an addition can meet, and
NaN.  Everything goes through the debug ops of lins_debug_math, one wave per item, 64 rows of 7 in, 28 sums out: op 9
is wave_reduce_rows, op 10 the same tree on __shfl_xor — and against a NumPy float64 emulation of the fixed tree that is
written out here and shares nothing with the device code."""
import ctypes as C

import numpy as np
import pytest

A = [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5, 0, 1, 2, 3, 4, 5, 6]
B = [0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 2, 3, 4, 5, 3, 4, 5, 4, 5, 5, 6, 6, 6, 6, 6, 6, 6]
LANES = np.arange(64)


@pytest.fixture(scope="module")
def ctx(pkg, ieskf):
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    yield c
    c.close()


def dev(ieskf, ctx, op, rows):
    x = np.ascontiguousarray(rows, dtype=np.float64).reshape(len(rows), 448)
    out = np.zeros((len(x), 28))
    L = ieskf.lib()
    L.lins_debug_math.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.lins_debug_math.restype = C.c_int
    assert L.lins_debug_math(ctx._h, op, len(x), x.ctypes.data, 448, out.ctypes.data, 28) == 0
    return out


def sum_index(lane):
    """Which of the 28 sums a lane ends up with (-1: none), from the tree: bit 5 of the lane took the upper 14 of 28,
    bit 4 the upper 7 of 14, bits 3, 2, 1 the upper half of 8 (7 and a zero), 4, 2; bit 0 holds a copy."""
    local = ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1)
    return ((lane >> 5) & 1) * 14 + ((lane >> 4) & 1) * 7 + local if local < 7 and not lane & 1 else -1


def tree(rows):
    """The fixed tree in float64, lane by lane: (n, 64, 7) rows -> (n, 28) sums.  At a halving level xor m a lane without
    bit m keeps the lower `cnt` of the sums it carries and adds its partner's copies of them, a lane with the bit does
    the same with the upper `cnt`; a last xor-1 add.  (NumPy's add is the IEEE add; no multiply-add is formed.)"""
    with np.errstate(all="ignore"):
        v = np.stack([rows[:, :, a] * rows[:, :, b] for a, b in zip(A, B)], axis=2)  # (n, 64, 28)
        for m, cnt in ((32, 14), (16, 7), (8, 4), (4, 2), (2, 1)):
            if m == 8:
                v = np.concatenate([v, np.zeros_like(v[:, :, :1])], axis=2)  # the 7 sums of a lane and a zero: 8
            up = ((LANES & m) != 0)[None, :, None]
            other = v[:, LANES ^ m, :]
            v = np.where(up, v[:, :, cnt:2 * cnt], v[:, :, :cnt]) + np.where(up, other[:, :, cnt:2 * cnt], other[:, :, :cnt])
        v = v[:, :, 0] + v[:, LANES ^ 1, 0]
    out = np.zeros((len(rows), 28))
    for lane in range(64):
        if sum_index(lane) >= 0:
            out[:, sum_index(lane)] = v[:, lane]
    return out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def check_bits(ieskf, ctx, rows):
    got, shfl, want = dev(ieskf, ctx, 9, rows), dev(ieskf, ctx, 10, rows), tree(rows)
    assert not np.isnan(want).any()  # (NaN has its own test: these inputs are built to produce none)
    assert np.array_equal(bits(got), bits(shfl))
    assert np.array_equal(bits(got), bits(want))
    return got


def primes(n):
    p = [2]
    k = 3
    while len(p) < n:
        if all(k % q for q in p if q * q <= k):
            p.append(k)
        k += 2
    return np.array(p, dtype=np.float64)


def test_the_emulation_covers_each_sum_exactly_once():
    assert sorted(sum_index(l) for l in range(64) if sum_index(l) >= 0) == list(range(28))
    rng = np.random.default_rng(1)
    rows = np.rint(rng.normal(size=(3, 64, 7)) * 8.0)  # small integers: every order of summation is exact
    want = np.stack([(rows[:, :, a] * rows[:, :, b]).sum(axis=1) for a, b in zip(A, B)], axis=1)
    assert np.array_equal(tree(rows), want)


@pytest.mark.gpu
def test_routing_every_lane_reaches_every_sum_once(ieskf, ctx):
    """Item l has a non-zero row in lane l only, 7 distinct primes (448 different ones over the items): each of the
    28 sums is then that lane's product and nothing else — a wrong half or row in a swap loses it or doubles it."""
    p = primes(448).reshape(64, 7)
    rows = np.zeros((64, 64, 7))
    rows[LANES, LANES] = p
    want = np.stack([p[:, a] * p[:, b] for a, b in zip(A, B)], axis=1)
    got = check_bits(ieskf, ctx, rows)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("name,used", [("upper 32", LANES >= 32), ("lower 32", LANES < 32), ("rows of 16 with bit 4", (LANES & 16) != 0),
                                       ("rows of 16 without bit 4", (LANES & 16) == 0), ("first 37", LANES < 37), ("first 5", LANES < 5)])
def test_partially_filled_waves(ieskf, ctx, name, used):
    """The last wave of a real scan: rows that are zero outside one half of the wave / every other row of 16 lanes / past
    a count that is no multiple of 16."""
    rng = np.random.default_rng(len(name))
    rows = rng.normal(size=(8, 64, 7)) * 10.0 ** rng.integers(-3, 4, size=(8, 64, 1)) * used[None, :, None]
    got = check_bits(ieskf, ctx, rows)
    want = np.stack([(rows[:, :, a] * rows[:, :, b]).sum(axis=1) for a, b in zip(A, B)], axis=1)
    scale = np.stack([np.abs(rows[:, :, a] * rows[:, :, b]).sum(axis=1) for a, b in zip(A, B)], axis=1)
    assert (np.abs(got - want) <= 1e-13 * scale).all()


@pytest.mark.gpu
def test_magnitudes_denormals_signed_zeros_and_overflow(ieskf, ctx):
    """200 random items scaled 1e-3 ... 1e3 per row; products that are denormal; products that are -0.0 in one half of
    the wave and +0.0 in the other (and -0.0 in both: the sum keeps the sign); products that overflow to +-inf.  The
    overflowing items give every component ONE sign over the whole wave, so that no sum meets +inf and -inf: inf - inf
    creates a NaN whose sign is the host's or the device's choice, which is not what this test is about."""
    rng = np.random.default_rng(5)
    rnd = rng.normal(size=(200, 64, 7)) * 10.0 ** rng.integers(-3, 4, size=(200, 64, 1))
    den = rng.normal(size=(16, 64, 7)) * 10.0 ** rng.integers(-162, -153, size=(16, 64, 1))  # products 1e-324 ... 1e-306
    with np.errstate(all="ignore"):
        p = den[:, :, 0] * den[:, :, 1]
    assert ((p != 0) & (np.abs(p) < 2.2250738585072014e-308)).any()
    zer = np.abs(rng.normal(size=(8, 64, 7)))
    lower, upper = LANES < 32, LANES >= 32
    zer[0, :, 0], zer[1, :, 0] = np.where(lower, -0.0, 0.0), np.where(lower, 0.0, -0.0)
    zer[2, :, 0], zer[3, :, 0] = np.where(LANES & 16, -0.0, 0.0), np.where(LANES & 16, 0.0, -0.0)
    zer[4, :, 0] = -0.0                                        # -0 in every lane: sums 1..5 and 21 are -0.0
    zer[5, :, :] = np.where(lower, -0.0, 0.0)[:, None] * np.array([1, -1, 1, -1, 1, -1, 1.0])  # nothing but zeros of both signs
    zer[6, :, 6], zer[7, :, 3] = np.where(upper, -0.0, 0.0), -0.0
    zer[7, :, :3] = 0.0
    ovf = np.abs(rng.normal(size=(12, 64, 7))) * 10.0 ** rng.choice([-3.0, 0.0, 150.0, 160.0, 200.0], size=(12, 64, 1))
    ovf *= rng.choice([-1.0, 1.0], size=(12, 1, 7))            # a component's sign: the same in all 64 lanes
    ovf[0] *= (LANES >= 32)[:, None]                           # infinities from one half only
    ovf[1] *= ((LANES & 16) == 0)[:, None]
    rows = np.concatenate([rnd, den, zer, ovf])
    got = check_bits(ieskf, ctx, rows)
    assert np.isinf(got[-12:]).any() and (got[-12:] == -np.inf).any()
    z = got[200 + 16 + 4]
    assert np.signbit(z[1:6]).all() and np.signbit(z[21]) and not np.signbit(z[0])  # (-0) + (-0) = -0, (-0)(-0) = +0


@pytest.mark.gpu
@pytest.mark.parametrize("lane", [5, 41])
def test_nan_in_one_lane(ieskf, ctx, lane):
    """One NaN component in one lane (lower half / upper half): the sums that contain it are NaN in both trees, in the
    emulation too, and all others are the same bits.  Whether the payload survives alike is printed (pytest -s), not asserted:
    profiles/rowsum_swap_exchange.md has the outcome."""
    rng = np.random.default_rng(lane)
    rows = rng.normal(size=(7, 64, 7))
    nan = np.array([0x7FF8000000001234], dtype=np.uint64).view(np.float64)[0]
    for k in range(7):
        rows[k, lane, k] = nan
    got, shfl, want = dev(ieskf, ctx, 9, rows), dev(ieskf, ctx, 10, rows), tree(rows)
    expect = np.array([[a == k or b == k for a, b in zip(A, B)] for k in range(7)])
    assert np.array_equal(np.isnan(got), expect)
    assert np.array_equal(np.isnan(got), np.isnan(shfl)) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(bits(got)[~expect], bits(shfl)[~expect]) and np.array_equal(bits(got)[~expect], bits(want)[~expect])
    # for the record: one NaN in the wave (every add has at most one NaN operand), then two NaNs with different
    # payloads in partner lanes of the xor-32 and of the xor-16 level (the adds whose operand order changed)
    two = rng.normal(size=(2, 64, 7))
    other = np.array([0x7FF8000000005678], dtype=np.uint64).view(np.float64)[0]
    two[0, lane, :], two[0, lane ^ 32, :] = nan, other
    two[1, lane, :], two[1, lane ^ 16, :] = nan, other
    g2, s2 = dev(ieskf, ctx, 9, two), dev(ieskf, ctx, 10, two)
    print("[nan lane %d] one NaN: payload bits equal to the shuffle tree: %s (%s)" % (
        lane, np.array_equal(bits(got), bits(shfl)), sorted(set("%016x" % b for b in bits(got)[expect]))))
    for name, g, s in (("xor 32", g2[0], s2[0]), ("xor 16", g2[1], s2[1])):
        print("[nan lane %d] two NaNs in partner lanes of %s: sums whose payload differs from the shuffle tree: %s; op 9 %s, op 10 %s" % (
            lane, name, np.nonzero(bits(g) != bits(s))[0].tolist(), sorted(set("%016x" % b for b in bits(g))),
            sorted(set("%016x" % b for b in bits(s)))))
    assert np.isnan(g2).all() and np.isnan(s2).all()
