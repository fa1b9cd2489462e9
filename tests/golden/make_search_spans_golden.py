"""Recipe of tests/golden/search_spans_parent_bits.npz: the results of two families of synthetic scans in the batch shape
("mr") as the library gave them on an MI355X BEFORE the searches of the lean core requested the bounds of several windows
in one trip (the parent of that commit, 4df907a).  Nothing but this project's own library writes into the file.
  room   host.synth_batch(8, start=37000): clouds beyond the resident positions, the far rings are read from global memory
  open   host.synth_batch(8, start=37100, scene=1): every position resident
(seeds no other golden file uses.)  Each family with ten fixed iterations (all 8) and with num_iter=30 under the stop rule
(the first four).  Stored per run: state, cov, residual_norm, update_norm, the five counts and reserved[1], reserved[2] — the
numbers of selections the nearest-neighbour / second-third-point certificates decided without a search: a search that
scanned another window, or the same windows in another order with another bound, moves them.
To re-derive it: build that commit, then  LINS_IESKF_LIB=<its liblins_ieskf.so> python tests/golden/make_search_spans_golden.py
Run from a later commit it records that commit's bits, which tests/test_gpu_search_spans.py requires to be the same.
usage: python tests/golden/make_search_spans_golden.py [out.npz]"""
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

ROOM_START, OPEN_START = 37000, 37100


def families():
    return {"room": host.synth_batch(8, start=ROOM_START), "open": host.synth_batch(8, start=OPEN_START, scene=1)}


def runs():
    """name -> (params, pairs): the four recorded runs"""
    fixed = pkg.default_params(num_iter=10, fixed_iters=1)
    stop = pkg.default_params(num_iter=30)
    out = {}
    for fam, pairs in families().items():
        out[fam + "_fixed"] = (fixed, pairs)
        out[fam + "_stop"] = (stop, pairs[:4])
    return out


def pack(res):
    return {"state": np.array([r.state for r in res]), "cov": np.array([np.asarray(r.cov).reshape(324) for r in res]),
            "residual_norm": np.array([r.residual_norm for r in res]), "update_norm": np.array([r.update_norm for r in res]),
            "counts": np.array([[r.iters, r.converged, r.diverged, r.m_surf, r.m_corner] for r in res], dtype=np.int32),
            "decided": np.array([[r.reserved[1], r.reserved[2]] for r in res], dtype=np.int32)}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "search_spans_parent_bits.npz")
    arrays = {}
    for name, (prm, pairs) in runs().items():
        with ieskf.IeskfContext(prm, max_batch=len(pairs), max_targets=16384, search="mr") as c:
            res = c.update_batch(pairs)
            assert c.last_search() == "mr"
        for k, v in pack(res).items():
            arrays[name + "." + k] = v
        print(name, "iters", [r.iters for r in res], "decided", [tuple(r.reserved[1:3]) for r in res])
    np.savez(out, **arrays)
    print("recorded", out)
