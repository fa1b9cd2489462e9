"""numpy statement of the mapping node's pose arithmetic (not a test), written from the reference's text
(lidar_mapping_node.cpp: transformAssociateToMap LM:411-536, transformUpdate's tail LM:567-576, the key-frame rule
LM:1655-1671), NOT from csrc/map_pose_math.h — the pin of lins_host_map_* and of the two pose kernels, in the manner of
tests/archive_np.py and tests/loop_icp_np.py.  Two forms of transformAssociateToMap:

(a) associate_f32: the f32 formula, every operation a numpy float32 scalar operation in the written order.  Each
    trigonometric call goes through `Trig`, which records (function, arguments, numpy's result): a test can then tell
    whether numpy's float32 sin / cos / arcsin / arctan2 agreed with libm's on exactly the arguments this evaluation met,
    which is the condition under which (a) with numpy's own trigonometry and the C restatement must agree bit for bit.
    numpy's float32 loops are SIMD approximations that differ from glibc's sinf / cosf in the last place on 11 - 17 % of
    arguments (asin 29 %, atan2 39 %), and an evaluation makes 42 such calls: nearly every case meets one.  `Trig(libm)`
    therefore takes a table of the C library's float functions and returns ITS value for each call (recording whether
    numpy's agreed): the arithmetic — every product, sum, division and their order — stays numpy's float32, the four
    functions are the ones the restatement's contract names, and no case has to be left out of the comparison.
(b) associate_f64: the rigid composition the formula expands.  R(rx, ry, rz) = Ry(ry) Rx(rx) Rz(rz), read off
    pointAssociateToMap (LM:594-607: yaw about z first, roll about x, pitch about y, then the translation
    (t[3], t[4], t[5])); T_tobe = T_aft T_bef^-1 T_sum, evaluated in f64 on the f32 inputs.  Returned as (R, t), never
    as angles: a comparison of matrices stays well conditioned where the angles do not.

Pose vectors are (rx, ry, rz, tx, ty, tz).  |rx| of the result near pi / 2 is outside the contract (the formula divides
by cos(rx))."""
import numpy as np

F = np.float32


class Trig:
    """float32 sin / cos / asin / atan2 of numpy, each call recorded"""

    def __init__(self, libm=None):
        """libm: None, or an object whose sinf / cosf / asinf / atan2f take and return C floats — then each call returns
        that function's value and `disagreed` counts the calls on which numpy's differed"""
        self.calls, self.libm, self.disagreed = [], libm, 0

    def _do(self, name, fn, *args):
        args = tuple(F(a) for a in args)
        r = F(fn(*args))
        self.calls.append((name, args, r))
        if self.libm is not None:
            c = F(getattr(self.libm, name)(*[float(a) for a in args]))
            self.disagreed += int(c.tobytes() != r.tobytes())
            return c
        return r

    def sin(self, x):
        return self._do("sinf", np.sin, x)

    def cos(self, x):
        return self._do("cosf", np.cos, x)

    def asin(self, x):
        return self._do("asinf", np.arcsin, x)

    def atan2(self, y, x):
        return self._do("atan2f", np.arctan2, y, x)


def associate_f32(bef, aft, total, trig=None):
    """(a): transformTobeMapped (6,) float32"""
    m = trig or Trig()
    b, a, s = (np.asarray(v, F).reshape(6) for v in (bef, aft, total))
    sin, cos = m.sin, m.cos
    with np.errstate(all="ignore"):
        x1 = cos(s[1]) * (b[3] - s[3]) - sin(s[1]) * (b[5] - s[5])
        y1 = b[4] - s[4]
        z1 = sin(s[1]) * (b[3] - s[3]) + cos(s[1]) * (b[5] - s[5])
        x2 = x1
        y2 = cos(s[0]) * y1 + sin(s[0]) * z1
        z2 = -sin(s[0]) * y1 + cos(s[0]) * z1
        inc3 = cos(s[2]) * x2 + sin(s[2]) * y2
        inc4 = -sin(s[2]) * x2 + cos(s[2]) * y2
        inc5 = z2

        sbcx, cbcx, sbcy, cbcy, sbcz, cbcz = sin(s[0]), cos(s[0]), sin(s[1]), cos(s[1]), sin(s[2]), cos(s[2])
        sblx, cblx, sbly, cbly, sblz, cblz = sin(b[0]), cos(b[0]), sin(b[1]), cos(b[1]), sin(b[2]), cos(b[2])
        salx, calx, saly, caly, salz, calz = sin(a[0]), cos(a[0]), sin(a[1]), cos(a[1]), sin(a[2]), cos(a[2])

        srx = (-sbcx * (salx * sblx + calx * cblx * salz * sblz + calx * calz * cblx * cblz)
               - cbcx * sbcy * (calx * calz * (cbly * sblz - cblz * sblx * sbly)
                                - calx * salz * (cbly * cblz + sblx * sbly * sblz) + cblx * salx * sbly)
               - cbcx * cbcy * (calx * salz * (cblz * sbly - cbly * sblx * sblz)
                                - calx * calz * (sbly * sblz + cbly * cblz * sblx) + cblx * cbly * salx))
        t0 = -m.asin(srx)

        srycrx = (sbcx * (cblx * cblz * (caly * salz - calz * salx * saly)
                          - cblx * sblz * (caly * calz + salx * saly * salz) + calx * saly * sblx)
                  - cbcx * cbcy * ((caly * calz + salx * saly * salz) * (cblz * sbly - cbly * sblx * sblz)
                                   + (caly * salz - calz * salx * saly) * (sbly * sblz + cbly * cblz * sblx)
                                   - calx * cblx * cbly * saly)
                  + cbcx * sbcy * ((caly * calz + salx * saly * salz) * (cbly * cblz + sblx * sbly * sblz)
                                   + (caly * salz - calz * salx * saly) * (cbly * sblz - cblz * sblx * sbly)
                                   + calx * cblx * saly * sbly))
        crycrx = (sbcx * (cblx * sblz * (calz * saly - caly * salx * salz)
                          - cblx * cblz * (saly * salz + caly * calz * salx) + calx * caly * sblx)
                  + cbcx * cbcy * ((saly * salz + caly * calz * salx) * (sbly * sblz + cbly * cblz * sblx)
                                   + (calz * saly - caly * salx * salz) * (cblz * sbly - cbly * sblx * sblz)
                                   + calx * caly * cblx * cbly)
                  - cbcx * sbcy * ((saly * salz + caly * calz * salx) * (cbly * sblz - cblz * sblx * sbly)
                                   + (calz * saly - caly * salx * salz) * (cbly * cblz + sblx * sbly * sblz)
                                   - calx * caly * cblx * sbly))
        t1 = m.atan2(srycrx / cos(t0), crycrx / cos(t0))

        srzcrx = ((cbcz * sbcy - cbcy * sbcx * sbcz) * (calx * salz * (cblz * sbly - cbly * sblx * sblz)
                                                       - calx * calz * (sbly * sblz + cbly * cblz * sblx) + cblx * cbly * salx)
                  - (cbcy * cbcz + sbcx * sbcy * sbcz) * (calx * calz * (cbly * sblz - cblz * sblx * sbly)
                                                         - calx * salz * (cbly * cblz + sblx * sbly * sblz) + cblx * salx * sbly)
                  + cbcx * sbcz * (salx * sblx + calx * cblx * salz * sblz + calx * calz * cblx * cblz))
        crzcrx = ((cbcy * sbcz - cbcz * sbcx * sbcy) * (calx * calz * (cbly * sblz - cblz * sblx * sbly)
                                                       - calx * salz * (cbly * cblz + sblx * sbly * sblz) + cblx * salx * sbly)
                  - (sbcy * sbcz + cbcy * cbcz * sbcx) * (calx * salz * (cblz * sbly - cbly * sblx * sblz)
                                                         - calx * calz * (sbly * sblz + cbly * cblz * sblx) + cblx * cbly * salx)
                  + cbcx * cbcz * (salx * sblx + calx * cblx * salz * sblz + calx * calz * cblx * cblz))
        t2 = m.atan2(srzcrx / cos(t0), crzcrx / cos(t0))

        x1 = cos(t2) * inc3 - sin(t2) * inc4
        y1 = sin(t2) * inc3 + cos(t2) * inc4
        z1 = inc5
        x2 = x1
        y2 = cos(t0) * y1 - sin(t0) * z1
        z2 = sin(t0) * y1 + cos(t0) * z1
        t3 = a[3] - (cos(t1) * x2 + sin(t1) * z2)
        t4 = a[4] - y2
        t5 = a[5] - (-sin(t1) * x2 + cos(t1) * z2)
    out = np.array([t0, t1, t2, t3, t4, t5])
    assert out.dtype == F  # (every operation above stayed in float32)
    return out


def rotation(rx, ry, rz):
    """R = Ry(ry) Rx(rx) Rz(rz) in f64 (pointAssociateToMap, LM:594-607)"""
    rx, ry, rz = float(rx), float(ry), float(rz)
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    return Ry @ Rx @ Rz


def rigid(t6):
    """(R, t) of a pose vector, f64 on the f32 values"""
    t6 = np.asarray(t6, F).astype(np.float64)
    return rotation(*t6[:3]), t6[3:6].copy()


def associate_f64(bef, aft, total):
    """(b): (R, t) of T_aft T_bef^-1 T_sum"""
    (Rb, tb), (Ra, ta), (Rs, ts) = rigid(bef), rigid(aft), rigid(total)
    Rab = Ra @ Rb.T
    return Rab @ Rs, Rab @ (ts - tb) + ta


def transform_update(tobe, has_imu, imu_roll, imu_pitch, total, bef, aft):
    """LM:567-576 -> (tobe, bef, aft): the blend is a double expression (0.998 and 0.002 are double literals) rounded
    once on assignment to the float element"""
    t = np.array(tobe, F).reshape(6).copy()
    if has_imu:
        t[0] = F(0.998 * float(t[0]) + 0.002 * float(F(imu_pitch)))
        t[2] = F(0.998 * float(t[2]) + 0.002 * float(F(imu_roll)))
    return t, np.array(total, F).reshape(6).copy(), t.copy()


def key_rule(prev, aft, have_frames):
    """LM:1655-1671 -> (save, prev): f32 differences, products and sums in the written order, the float sqrt, compared
    with the double 0.3; prev moves only when the frame is saved"""
    p, a = np.array(prev, F).reshape(3).copy(), np.asarray(aft, F).reshape(6)
    dx, dy, dz = p[0] - a[3], p[1] - a[4], p[2] - a[5]
    d = np.sqrt(dx * dx + dy * dy + dz * dz)
    assert d.dtype == F
    save = not (float(d) < 0.3)
    if not save and have_frames:
        return 0, p
    return 1, a[3:6].copy()
