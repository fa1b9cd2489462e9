"""The case set of the seam between the filter and the mapping node, shared by tests/test_odom_host.py and
tests/test_gpu_odom.py (not a test): global states (19 doubles: rn_ 0-2, qbn_ 6-9 as w, x, y, z) whose records are
finite — quaternion norms >= 0.5, finite positions — so that every case takes part in every comparison."""
import numpy as np

import odom_np as on

SEED = 20261
PITCH_MAX, T_MAX = 1.2, 200.0

# E_host: the largest difference of the host restatement to the independent numpy.longdouble route (odom_np (c)) over
# CASES, as the largest absolute entry of a rotation-matrix difference.
#   E_HOST_SUM   R(angles of lins_host_odom_from_global's transform_sum) against R(the quaternion the mapping node
#                reads); dominated by the f32 rounding of the three angles.
#   E_HOST_QUAT  R(lins_host_pose_quat of a pose) against R(setRPY's angles of that pose), over the transform_sum rows of
#                CASES taken as poses; f64 rounding of the half-angle products.
# Measured on the CPU (x86-64, glibc 2.39's libm, g++ -O3 -ffp-contract=off) with tests/test_odom_host.py, which prints
# the two figures before it asserts.  The tests' bars are 4 x these: margin for another libm build, and for ocml's
# last-place differences on the device (same f64 text, trigonometry aside).
E_HOST_SUM = 1.544e-07
E_HOST_QUAT = 3.201e-16


def state(q_wxyz, pos=(0.0, 0.0, 0.0)):
    g = np.zeros(19)
    g[0:3], g[6:10] = pos, q_wxyz
    return g


def axis_quat(axis, deg):
    h = np.deg2rad(deg) / 2.0
    q = np.zeros(4)
    q[0], q[1 + axis] = np.cos(h), np.sin(h)
    return q


def tf_pitch(q_wxyz):
    """tf's pitch of the quaternion the mapping node forms from this qbn_ (outside the gimbal branch)"""
    w, x, y, z = q_wxyz
    return -np.arcsin(np.clip(on.tf_matrix([y, z, x, w])["m20"], -1.0, 1.0))


def gimbal_states():
    """qbn_ = a 90 degree rotation about the axis that is tf's pitch axis, built from components next to sqrt(1/2) for
    which tf's m20 = xz - wy rounds to exactly +1 and to exactly -1 (searched among the f64 neighbours of sqrt(1/2))"""
    r = float(np.sqrt(0.5))
    near = [r]
    for _ in range(3):
        near = [np.nextafter(near[0], 0.0)] + near + [np.nextafter(near[-1], 1.0)]
    out = {}
    for a in near:
        for b in near:
            for sign in (1.0, -1.0):
                # the mapping node's (x', y', z', w') = (q.z, -q.x, -q.y, q.w) of (x, y, z, w) = (qbn.y, qbn.z, qbn.x, qbn.w):
                # y' = -qbn.y, so a rotation about the body's y axis is a rotation about tf's pitch axis
                q = np.array([a, 0.0, sign * b, 0.0])
                m20 = on.tf_matrix([q[2], q[3], q[1], q[0]])["m20"]
                if abs(m20) == 1.0 and m20 not in out:
                    out[m20] = q
    assert set(out) == {1.0, -1.0}, "no components next to sqrt(1/2) round m20 to +-1"
    return [("gimbal_m20_%+d" % int(m), state(out[m], (1.5, -2.5, 3.5))) for m in (1.0, -1.0)]


def build_cases():
    """[(name, global state (19,))]"""
    rng = np.random.default_rng(SEED)
    cases = [("identity", state([1.0, 0.0, 0.0, 0.0]))]
    for axis in range(3):
        for deg in (30.0, -30.0, 90.0, -90.0, 179.0):
            cases.append(("axis%d_%+.0f" % (axis, deg), state(axis_quat(axis, deg), rng.uniform(-T_MAX, T_MAX, 3))))
    seeded = []
    while len(seeded) < 200:
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        if abs(tf_pitch(q)) <= PITCH_MAX:
            seeded.append(q)
            cases.append(("seeded%d" % (len(seeded) - 1), state(q, rng.uniform(-T_MAX, T_MAX, 3))))
    for i in range(20):  # tf's 2 / d: the same rotations away from unit norm
        for scale in (0.5, 2.0):
            cases.append(("seeded%d_norm%.1f" % (i, scale), state(seeded[i] * scale, rng.uniform(-T_MAX, T_MAX, 3))))
    cases += gimbal_states()
    return cases


CASES = build_cases()
STATES = np.stack([g for _, g in CASES])


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def adjacent_or_equal32(a, b):
    """elementwise: float32 a and b are the same float or neighbours (finite values; +0 and -0 count as the same)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a == b) | (np.nextafter(a, np.float32(np.inf)) == b) | (np.nextafter(a, np.float32(-np.inf)) == b)
