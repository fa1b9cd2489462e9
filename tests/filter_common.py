"""Shared by tests/test_filter_finish.py (CPU) and tests/test_gpu_filter.py: the product's lins_filter built from the
reference's records, IMU rows, and comparisons of filters."""
import ctypes as C

import numpy as np

DT = 0.1 / 40


def new_filter(host, vn=(0, 0, 0), ba=(0, 0, 0), bw=(0, 0, 0), pos_std=None, att_std=None):
    L = host.lib()
    fp = host.FilterParams()
    L.lins_filter_default_params(C.byref(fp))
    if pos_std is not None:
        fp.init_pos_std[:] = pos_std
    if att_std is not None:
        fp.init_att_std[:] = att_std
    f = host.Filter()
    dp = C.POINTER(C.c_double)
    v = [np.ascontiguousarray(x, dtype=np.float64) for x in (vn, ba, bw)]
    L.lins_filter_init(C.byref(f), C.byref(fp), v[0].ctypes.data_as(dp), v[1].ctypes.data_as(dp), v[2].ctypes.data_as(dp))
    return f, fp


def filter_from_record(host, rec):
    """the reference's StatePredictor after a scan (record of oracle/ref_seq.py) as a lins_filter"""
    f, _ = new_filter(host)
    f.state[:] = rec.filter_state[:]
    f.cov[:] = rec.filter_cov[:]
    f.acc_last[:] = rec.imu_last[0:3]
    f.gyr_last[:] = rec.imu_last[3:6]
    f.has_imu = 1
    return f


def copy_filter(host, f):
    g = host.Filter()
    C.memmove(C.byref(g), C.byref(f), C.sizeof(g))
    return g


def imu_rows(acc, gyr, dt=DT):
    """(m, 3) acc, (m, 3) gyr -> (m, 7) rows (dt, acc, gyr)"""
    acc, gyr = np.asarray(acc, np.float64), np.asarray(gyr, np.float64)
    return np.ascontiguousarray(np.hstack([np.full((len(acc), 1), dt), acc, gyr]))


def host_predict(host, f, rows):
    dp = C.POINTER(C.c_double)
    for r in np.asarray(rows, np.float64).reshape(-1, 7):
        a, g = np.ascontiguousarray(r[1:4]), np.ascontiguousarray(r[4:7])
        host.lib().lins_filter_predict(C.byref(f), float(r[0]), a.ctypes.data_as(dp), g.ctypes.data_as(dp))


def filter_arrays(f):
    """every number a lins_filter holds that a step may change"""
    return (np.array(f.state[:]), np.array(f.cov[:]), np.array(f.acc_last[:]), np.array(f.gyr_last[:]),
            np.array([f.time, float(f.has_imu)]))


def filters_bitwise_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(filter_arrays(a), filter_arrays(b)))
