"""The key-pose selection on the device, the part that can be held on the CPU (include/lins_map.h lins_keyposes_*;
csrc/keypose_select_math.h): the linear-time list rule the kernel is the parallel form of against surround_update's text
and against tests/surround_np.py — crafted cases, seeded random cases with lists that hold an id twice, a there-and-back
walk — and the packed key's order, as a stand-alone program under AddressSanitizer and UBSan
(tests/native/keyposes_check.cpp); the ctypes mirrors of the three structs against the C compiler."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import surround_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lins---lidar-inertial-slam_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("keyposes") / "keyposes_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", "keyposes_check.cpp"), "-o", out])
    return out


def run_lists(exe, cases):
    """cases: (list, ds) pairs -> the lists kp_surround_list gives; the program itself fails where surround_update differs"""
    text = "".join(" ".join(map(str, lst)) + " | " + " ".join(map(str, ds)) + "\n" for lst, ds in cases)
    run = subprocess.run([exe, "lists"], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()
    got = [[int(v) for v in line.split()] for line in run.stdout.decode().split("\n")[:-1]]
    assert len(got) == len(cases)
    return got


def test_linear_list_rule_on_crafted_cases(exe):
    got = run_lists(exe, [(lst, ds) for lst, ds, _ in surround_np.CRAFTED])
    assert got == [want for _, _, want in surround_np.CRAFTED]


def test_linear_list_rule_on_random_cases(exe):
    rng = np.random.default_rng(23)
    cases = []
    for k in range(200):
        pool = int(rng.integers(1, 30))
        if k % 2:  # a list that may hold an id twice (the node's never does; the rule is defined for it all the same)
            lst = rng.integers(0, pool, int(rng.integers(0, 25))).tolist()
        else:
            lst = rng.permutation(pool)[: rng.integers(0, pool + 1)].tolist()
        cases.append((lst, rng.integers(0, pool, int(rng.integers(0, 25))).tolist()))
    got = run_lists(exe, cases)
    want = [surround_np.surround_update(lst, ds) for lst, ds in cases]
    assert got == want
    assert sum(len(set(lst)) < len(lst) for lst, _ in cases) > 20 and sum(len(set(ds)) < len(ds) for _, ds in cases) > 20
    assert sum(len(set(w)) < len(w) for w in want) > 5  # a repeated survivor stays repeated
    assert sum(len(w) > len(lst) for w, (lst, _) in zip(want, cases)) > 20 and sum(len(w) < len(lst) for w, (lst, _) in zip(want, cases)) > 20


def test_linear_list_rule_on_a_there_and_back_walk(exe, host):
    """40 poses 0.5 m apart along x, walked out and back (radius 5, pose leaf 1), as tests/test_surround_host.py walks them"""
    poses = np.zeros((40, 6), np.float32)
    poses[:, 0] = 0.5 * np.arange(40)
    cases, lst = [], []
    for at in list(range(40)) + list(range(38, -1, -1)):
        ds = host.select_radius(poses, poses[at, :3], 5.0, 1.0).tolist()
        cases.append((lst, ds))
        lst = surround_np.surround_update(lst, ds)
    got = run_lists(exe, cases)
    assert got == [surround_np.surround_update(l, ds) for l, ds in cases]
    assert got[-1] != sorted(got[-1]) and any(len(g) < len(l) for g, (l, _) in zip(got, cases))


def test_packed_key_orders_as_distance_then_id(exe):
    run = subprocess.run([exe, "keys"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()
    assert run.stdout.decode().startswith("ok ")


def test_keyposes_mirrors_match_the_c_structs(defs):
    src = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_map.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(lins_keyposes_query), offsetof(lins_keyposes_query, centre), offsetof(lins_keyposes_query, radius),
         offsetof(lins_keyposes_query, pose_leaf));
  printf("%zu %zu %zu\n", sizeof(lins_keyposes_loop_query), offsetof(lins_keyposes_loop_query, now), offsetof(lins_keyposes_loop_query, min_gap_s));
  printf("%zu %zu %zu %zu\n", sizeof(lins_keyposes_result), offsetof(lins_keyposes_result, hits), offsetof(lins_keyposes_result, status),
         offsetof(lins_keyposes_result, host));
  printf("%d %d\n", LINS_KEYPOSES_HOST, LINS_KEYPOSES_DEVICE);
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        out = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", out])
        got = [int(x) for x in subprocess.check_output([out]).split()]
    Q, L, R = defs.KeyposesQueryC, defs.KeyposesLoopQueryC, defs.KeyposesResultC
    assert got == [C.sizeof(Q), Q.centre.offset, Q.radius.offset, Q.pose_leaf.offset, C.sizeof(L), L.now.offset, L.min_gap_s.offset,
                   C.sizeof(R), R.hits.offset, R.status.offset, R.host.offset, defs.KEYPOSES_HOST, defs.KEYPOSES_DEVICE]


def test_the_library_exports_the_calls(ieskf):
    names = [n for n in ieskf.EXPORTS if n.startswith(("lins_keyposes_", "lins_last_keyposes"))]
    assert len(names) == 6
    for name in names:
        assert hasattr(ieskf.lib(), name), name
