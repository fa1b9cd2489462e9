"""The case set of transformAssociateToMap shared by tests/test_map_pose_host.py and tests/test_gpu_map_pose.py (not a
test), the comparison against tests/map_pose_np.py's two forms, and the key rule's threshold cases."""
import ctypes as C
import ctypes.util

import numpy as np

import map_pose_np as mp

F = np.float32
SEED = 20260
RX_MAX, T_MAX = 1.2, 200.0

# E_host: the largest difference of lins_host_map_associate to the f64 composition (map_pose_np.associate_f64) over
# CASES — rotation: largest absolute entry of R(tobe) - R_b; translation: largest absolute component, in metres.
# Measured on the CPU (x86-64, glibc 2.39's libm, g++ -O3 -ffp-contract=off) with tests/test_map_pose_host.py, which
# prints the two figures before it asserts.  The tests' bars are 4 x these: margin for another libm build, and for
# ocml's last-place differences on the device (same f32 text, trigonometry aside; measured on an MI355X: 1.159e-06 and
# 2.353e-04 m, profiles/map_pose_gpu_tests.txt).
E_HOST_ROT = 9.332e-07
E_HOST_TRANS = 1.759e-04


def _pose(rng, rot=True, trans=True):
    r = rng.uniform(-1.0, 1.0, 3) * [RX_MAX, np.pi, np.pi] if rot else np.zeros(3)
    t = rng.uniform(-T_MAX, T_MAX, 3) if trans else np.zeros(3)
    return np.concatenate([r, t]).astype(F)


def build_cases():
    """[(name, bef, aft, sum)], all (6,) f32; |rx| <= 1.2 rad, |ry|, |rz| <= pi, |t| <= 200 m"""
    rng = np.random.default_rng(SEED)
    z = np.zeros(6, F)
    cases = [("identity", z, z, z)]
    for i in range(6):  # pure translations
        cases.append(("translation%d" % i, _pose(rng, rot=False), _pose(rng, rot=False), _pose(rng, rot=False)))
    for who in range(3):  # single-axis rotations: one angle of one of the three poses
        for axis in range(3):
            for ang in (0.7, -1.1):
                v = [z.copy(), z.copy(), z.copy()]
                v[who][axis] = ang
                cases.append(("axis%d_%d_%+.1f" % (who, axis, ang), *v))
    for i in range(200):
        cases.append(("seeded%d" % i, _pose(rng), _pose(rng), _pose(rng)))
    for i in range(8):  # bef == sum: the odometry has not moved since the last mapped scan, tobe = aft to rounding
        b = _pose(rng)
        cases.append(("bef_is_sum%d" % i, b, _pose(rng), b.copy()))
    for i in range(8):  # the first scan: transformBefMapped = transformAftMapped = 0 (LM:305-409)
        cases.append(("first_scan%d" % i, z, z, _pose(rng)))
    return [(n, np.asarray(b, F), np.asarray(a, F), np.asarray(s, F)) for n, b, a, s in cases]


CASES = build_cases()

_LIBM = None


def libm():
    global _LIBM
    if _LIBM is None:
        L = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for name, nargs in (("sinf", 1), ("cosf", 1), ("asinf", 1), ("atan2f", 2)):
            f = getattr(L, name)
            f.argtypes, f.restype = [C.c_float] * nargs, C.c_float
        _LIBM = L
    return _LIBM


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def numpy_trig_is_libm(trig):
    """every call the evaluation `trig` recorded gave the bits libm gives on the same arguments"""
    L = libm()
    for name, args, got in trig.calls:
        want = F(getattr(L, name)(*[float(a) for a in args]))
        if not same_bits([got], [want]):
            return False
    return True


def diff_to_composition(tobe, bef, aft, total):
    """(rotation, translation) difference of a pose vector to form (b)"""
    Rb, tb = mp.associate_f64(bef, aft, total)
    R, t = mp.rigid(tobe)
    return float(np.abs(R - Rb).max()), float(np.abs(t - tb).max())


def f32_neighbours(x, k):
    """the 2 k + 1 floats around float32 x, ascending"""
    x = F(x)
    lo = x
    for _ in range(k):
        lo = np.nextafter(lo, F(-np.inf))
    out = [lo]
    for _ in range(2 * k):
        out.append(np.nextafter(out[-1], F(np.inf)))
    return out


def key_rule_threshold_cases():
    """[(prev (3,), aft (6,))]: offsets of 0.3 m from prev along one axis and along the diagonal, found by walking the
    f32 neighbours of one component of the offset until the f32 distance of LM:1660-1665 sits at the first float that is
    not < 0.3 and at the floats one ulp either side of it.  (prev = 0, so that the differences are the offsets
    themselves and a step of one component moves the distance by no more than its own ulp.)"""
    out = []
    prev = np.zeros(3, F)
    for direction in (np.array([1, 0, 0], F), np.array([1, 1, 1], F)):
        start = F(0.3) / F(np.sqrt(F(direction @ direction)))
        cands = []
        for off in f32_neighbours(start, 12):
            aft = np.zeros(6, F)
            aft[3:6] = direction * start
            aft[3] = off
            d = prev - aft[3:6]
            cands.append((F(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])), aft))
        dists = sorted(set(float(c[0]) for c in cands))
        at = min(i for i, d in enumerate(dists) if not d < 0.3)  # the threshold: the first distance that saves
        assert 0 < at < len(dists) - 1, "the walk did not straddle 0.3"
        three = dists[at - 1:at + 2]
        assert all(float(np.nextafter(F(a), F(np.inf))) == b for a, b in zip(three, three[1:])), "not consecutive floats"
        for want in three:
            out.append((prev.copy(), next(a for d, a in cands if float(d) == want)))
    return out
