"""Recipe of tests/golden/tail_parent_bits.npz: the results of 8 synthetic scans (START = 31000 of tests/test_gpu_tail.py),
ten fixed iterations, in the batch shape ("mr"), as the library gave them on an MI355X BEFORE the serial tail was reduced
to the rotation chain (the parent of that commit, 2935c20).  Nothing but this project's own library writes into the file.
To re-derive it: build that commit, then  LINS_IESKF_LIB=<its liblins_ieskf.so> python tests/golden/make_tail_golden.py
Run from a later commit it records that commit's bits, which tests/test_gpu_tail.py requires to be the same.
usage: python tests/golden/make_tail_golden.py [out.npz]"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
PKG = "lins---lidar-inertial-slam_amd"
pkg = importlib.import_module(PKG)
host = importlib.import_module(PKG + ".host")
ieskf = importlib.import_module(PKG + ".ieskf")

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "tail_parent_bits.npz")
prm = pkg.default_params(num_iter=10, fixed_iters=1)
batch = host.synth_batch(8, start=31000)
with ieskf.IeskfContext(prm, max_batch=8, max_targets=16384, search="mr") as c:
    res = c.update_batch(batch)
    assert c.last_search() == "mr"
np.savez(out, state=np.array([r.state for r in res]), cov=np.array([np.asarray(r.cov).reshape(324) for r in res]),
         residual_norm=np.array([r.residual_norm for r in res]), update_norm=np.array([r.update_norm for r in res]),
         counts=np.array([[r.iters, r.converged, r.diverged, r.m_surf, r.m_corner] for r in res], dtype=np.int32))
print("recorded", out)
