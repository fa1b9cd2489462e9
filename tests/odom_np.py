"""The seam between the filter and the mapping node restated in Python (not a test; csrc/odom_math.h is the contract):
  (a) the literal f64 statement of odom_transform_sum and pose_quat, operation for operation, with the C library's f64
      asin / atan2 / sin / cos — Python floats are IEEE doubles and CPython does not contract, so the bits must agree;
  (b) the two f64 quaternion products of SE:1153-1154 written out, which odom_yzx's exact permutation departs from;
  (c) an independent route in numpy.longdouble: rotation matrices composed from the published angles / quaternions."""
import ctypes as C
import ctypes.util

import numpy as np

LD = np.longdouble
HALF_PI = 3.14159265358979323846 / 2.0
_LIBM = None


def libm():
    """the C library's f64 asin / atan2 / sin / cos (map_pose_cases.libm's f64 sibling)"""
    global _LIBM
    if _LIBM is None:
        L = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for name, nargs in (("sin", 1), ("cos", 1), ("asin", 1), ("atan2", 2)):
            f = getattr(L, name)
            f.argtypes, f.restype = [C.c_double] * nargs, C.c_double
        _LIBM = L
    return _LIBM


# ---- (a) the literal statement ------------------------------------------------------------------------------------
def yzx(gs):
    """odom_yzx: (pos (3,), q (x, y, z, w)) of a global state (19,)"""
    g = [float(v) for v in gs]
    return [g[1], g[2], g[0]], [g[8], g[9], g[7], g[6]]


def tf_matrix(q_xyzw):
    """tf::Matrix3x3::setRotation of tf::Quaternion(q.z, -q.x, -q.y, q.w): the seven entries getRPY reads"""
    x, y, z, w = float(q_xyzw[2]), -float(q_xyzw[0]), -float(q_xyzw[1]), float(q_xyzw[3])
    d = x * x + y * y + z * z + w * w
    s = 2.0 / d
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    return dict(m00=1.0 - (yy + zz), m01=xy - wz, m02=xz + wy, m10=xy + wz, m20=xz - wy, m21=yz + wx, m22=1.0 - (xx + yy))


def takes_gimbal_branch(q_xyzw):
    return abs(tf_matrix(q_xyzw)["m20"]) >= 1.0


def transform_sum(pos, q_xyzw):
    """odom_transform_sum -> (6,) f32"""
    L = libm()
    m = tf_matrix(q_xyzw)
    if abs(m["m20"]) >= 1.0:
        yaw = 0.0
        if m["m20"] < 0.0:
            pitch, roll = HALF_PI, L.atan2(m["m01"], m["m02"])
        else:
            pitch, roll = -HALF_PI, L.atan2(-m["m01"], -m["m02"])
    else:
        pitch = -L.asin(m["m20"])
        roll = L.atan2(m["m21"] / L.cos(pitch), m["m22"] / L.cos(pitch))
        yaw = L.atan2(m["m10"] / L.cos(pitch), m["m00"] / L.cos(pitch))
    return np.array([-pitch, -yaw, roll, pos[0], pos[1], pos[2]], np.float64).astype(np.float32)


def pose_quat(t6):
    """pose_quat -> (x, y, z, w) f64"""
    L = libm()
    t = np.asarray(t6, np.float32)
    roll, pitch, yaw = float(t[2]), -float(t[0]), -float(t[1])
    hy, hp, hr = yaw * 0.5, pitch * 0.5, roll * 0.5
    cy, sy, cp, sp, cr, sr = L.cos(hy), L.sin(hy), L.cos(hp), L.sin(hp), L.cos(hr), L.sin(hr)
    x = sr * cp * cy - cr * sp * sy
    y = cr * sp * cy + sr * cp * sy
    z = cr * cp * sy - sr * sp * cy
    w = cr * cp * cy + sr * sp * sy
    return np.array([-y, -z, x, w], np.float64)


# ---- (b) Eigen's two products --------------------------------------------------------------------------------------
def qmul(a, b):
    """Eigen's quaternion product, (w, x, y, z), f64 in its order of operations"""
    aw, ax, ay, az = (float(v) for v in a)
    bw, bx, by, bz = (float(v) for v in b)
    return [aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx]


# Q_xyz_to_yzx = Quaterniond(R_xyz_to_yzx) for R = [[0, 1, 0], [0, 0, 1], [1, 0, 0]] (SE:217-220): trace 0, so Eigen's
# conversion takes its largest-diagonal branch with i = 0 and gives exactly (w, x, y, z) = (-0.5, 0.5, 0.5, 0.5); the
# inverse of a quaternion of squared norm exactly 1 is its conjugate.
Q_XYZ_TO_YZX = [-0.5, 0.5, 0.5, 0.5]
Q_XYZ_TO_YZX_INV = [-0.5, -0.5, -0.5, -0.5]


def yzx_products(gs):
    """qbn_ of globalStateYZX_ by the two products of SE:1153-1154 -> (x, y, z, w) f64"""
    w, x, y, z = qmul(qmul(Q_XYZ_TO_YZX, [float(v) for v in gs[6:10]]), Q_XYZ_TO_YZX_INV)
    return np.array([x, y, z, w], np.float64)


# ---- (c) the independent route, numpy.longdouble -------------------------------------------------------------------
def rot_rpy_ld(roll, pitch, yaw):
    """Rz(yaw) Ry(pitch) Rx(roll): the matrix tf's setRPY / getRPY speak of"""
    r, p, y = LD(roll), LD(pitch), LD(yaw)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]], LD)
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]], LD)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]], LD)
    return Rz @ Ry @ Rx


def rot_quat_ld(x, y, z, w):
    """the rotation matrix of a quaternion of any non-zero norm"""
    x, y, z, w = LD(x), LD(y), LD(z), LD(w)
    n = x * x + y * y + z * z + w * w
    s = LD(2) / n
    return np.array([[1 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)],
                     [s * (x * y + w * z), 1 - s * (x * x + z * z), s * (y * z - w * x)],
                     [s * (x * z - w * y), s * (y * z + w * x), 1 - s * (x * x + y * y)]], LD)


def sum_rotation_error(total, q_xyzw):
    """largest absolute entry of R(angles of a transformSum) - R(tf::Quaternion(q.z, -q.x, -q.y, q.w))"""
    t = np.asarray(total, np.float32)
    Ra = rot_rpy_ld(t[2], -LD(t[0]), -LD(t[1]))
    Rq = rot_quat_ld(q_xyzw[2], -LD(q_xyzw[0]), -LD(q_xyzw[1]), q_xyzw[3])
    return float(np.abs(Ra - Rq).max())


def quat_rotation_error(q_xyzw, t6):
    """largest absolute entry of R(the tf quaternion behind a published orientation) - R(setRPY's angles of pose t6)"""
    t = np.asarray(t6, np.float32)
    Rq = rot_quat_ld(q_xyzw[2], -LD(q_xyzw[0]), -LD(q_xyzw[1]), q_xyzw[3])
    Ra = rot_rpy_ld(t[2], -LD(t[0]), -LD(t[1]))
    return float(np.abs(Rq - Ra).max())
