"""Recipe of tests/golden/streams_step_parent_bits.npz: what the five scenarios of tests/streams_step_cases.py leave, call
by call and stream by stream, as the library gave them on an MI355X BEFORE the streams step was split into phases with
the batch path's update launcher (the parent of that commit, 3326149).  Nothing but this project's own library writes
into the file.
To re-derive it: build that commit, then  LINS_IESKF_LIB=<its liblins_ieskf.so> python tests/golden/make_streams_step_golden.py
Run from a later commit it records that commit's bits, which tests/test_gpu_streams_step_golden.py requires to be the same.
usage: python tests/golden/make_streams_step_golden.py [out.npz]"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
PKG = "lins---lidar-inertial-slam_amd"
pkg = importlib.import_module(PKG)
host = importlib.import_module(PKG + ".host")
ieskf = importlib.import_module(PKG + ".ieskf")

import streams_step_cases as cases  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "streams_step_parent_bits.npz")
rec = {}
for name, fn in cases.SCENARIOS.items():
    for key, a in fn(pkg, host, ieskf).items():
        rec[name + "/" + key] = a
np.savez_compressed(out, **rec)
print("recorded", out, len(rec), "arrays,", os.path.getsize(out), "bytes")
