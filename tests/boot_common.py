"""Shared by tests/test_boot_host.py (CPU) and tests/test_gpu_boot.py: the stock synthetic sequences as the two-scan
bootstrap (SE:331-425) sees them, the reference's records of them, and the sparse sweep no feature survives."""
import numpy as np

import filter_common as fc
import seq_common

SEQS = (11, 12, 13)
N_SCANS = 6  # scans of each sequence the shared runs cover


def scan_time(k):
    return 0.1 * (k + 1)


def sparse(raw, step=8):
    """every `step`-th point of a raw sweep: the front-end extracts no feature from it (both gates of SE:332-333 fail)"""
    return np.ascontiguousarray(np.asarray(raw, np.float32).reshape(-1, 4)[::step])


def load(host, seq, n=N_SCANS):
    """raw clouds, (acc, gyr) samples and IMU rows (dt, acc, gyr) of the first n sweeps of a synthetic sequence"""
    raws = [host.synth_seq_raw_scan(seq, k) for k in range(n)]
    imus = [host.synth_seq_imu(seq, k) for k in range(n)]
    return dict(raws=raws, imus=imus, rows=[fc.imu_rows(a, g) for a, g in imus])


def imu_last(s, k):
    """the imu_last_ handed to processPCL with scan k: the newest sample (EC:164-169)"""
    acc, gyr = s["imus"][k]
    return np.concatenate([acc[-1], gyr[-1]])


def records(ref, ref_seq, prm, s, raws=None, n=None):
    """the reference's records over the sequence (raws: replacement clouds, e.g. a sparse sweep)"""
    raws = s["raws"] if raws is None else raws
    n = len(raws) if n is None else n
    inputs = [(scan_time(k), s["imus"][k][0], s["imus"][k][1], ref.segment(raws[k])) for k in range(n)]
    return seq_common.run(ref_seq, prm, inputs)


def host_bootstrap(host, s, icp_pose=None):
    """processFirstScan on scan 0, the pre-integration over scan 1's rows, and (icp_pose = (t, q) given)
    processSecondScan, on the CPU restatement.  Returns dict(first=(Filter, lin), pre, start=(pl, ql), second=(Filter,
    globalState_, lin) or None)."""
    f0, lin0, pre = host.boot_first(imu_last(s, 0), scan_time(0))
    host.preintegrate(pre, s["rows"][1])
    out = dict(first=(f0, lin0), pre=pre, start=host.boot_start(pre), second=None)
    if icp_pose is not None:
        out["second"] = host.boot_second(pre, icp_pose[0], icp_pose[1], imu_last(s, 1), scan_time(1))
    return out
