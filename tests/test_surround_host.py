"""The mapping node's surrounding-key-frame mode on the CPU (include/lins_host.h lins_host_surround_update /
_surround_map; LM:1247-1315): the list rule against tests/surround_np.py — an independent statement of LM:1261-1308 in
Python lists — on crafted and random cases and along a there-and-back walk, the map restatement against the two
restatements it composes, and the rule's own text (csrc/host/keyframe_select.h) as a stand-alone program under
AddressSanitizer and UBSan."""
import os
import subprocess

import numpy as np
import pytest

import surround_np
from local_map_synth import room_scan, trajectory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lins---lidar-inertial-slam_amd", "csrc")
SUBMAP_CORNER, SUBMAP_SURF, SUBMAP_OUTLIER = 1, 2, 4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_the_checker_on_the_crafted_cases():
    for lst, ds, want in surround_np.CRAFTED:
        assert surround_np.surround_update(lst, ds) == want, (lst, ds)


@pytest.mark.parametrize("case", range(len(surround_np.CRAFTED)))
def test_list_rule_on_crafted_cases(host, case):
    lst, ds, want = surround_np.CRAFTED[case]
    assert host.surround_update(lst, ds) == want == surround_np.surround_update(lst, ds)


def test_list_rule_on_random_cases(host):
    rng = np.random.default_rng(11)
    grew = shrank = repeats = 0
    for _ in range(200):
        pool = int(rng.integers(1, 30))
        lst = rng.permutation(pool)[: rng.integers(0, pool + 1)].tolist()  # (the list never holds an id twice)
        ds = rng.integers(0, pool, int(rng.integers(0, 25))).tolist()
        got = host.surround_update(lst, ds)
        assert got == surround_np.surround_update(lst, ds), (lst, ds)
        grew += len(got) > len(lst)
        shrank += len(got) < len(lst)
        repeats += len(set(ds)) < len(ds)
    assert grew > 20 and shrank > 20 and repeats > 20


def test_capacity_refusal_leaves_the_list_as_it_was(host):
    assert host.surround_update([1, 2], [2, 3, 4], cap=3) == [2, 3, 4]  # (one erased first: three fit)
    with pytest.raises(MemoryError):  # (the binding asserts the array still holds [5, 6])
        host.surround_update([5, 6], [6, 5, 7], cap=2)
    with pytest.raises(MemoryError):
        host.surround_update([], [1], cap=0)


def test_there_and_back_walk(host):
    """40 poses 0.5 m apart along x; the robot walks out over them and back.  radius 5, pose leaf 1"""
    poses = np.zeros((40, 6), np.float32)
    poses[:, 0] = 0.5 * np.arange(40)
    walk = list(range(40)) + list(range(38, -1, -1))
    got, want = [], []
    erased = reentered_behind_newer = False
    for at in walk:
        centre = poses[at, :3]
        ds = host.select_radius(poses, centre, 5.0, 1.0).tolist()
        before = list(want)
        got, want = host.surround_update(got, ds), surround_np.surround_update(want, ds)
        assert got == want, (at, ds)
        erased = erased or any(v not in want for v in before)
        new = [v for v in want if v not in before]
        if new and before:
            kept = [v for v in want if v in before]
            reentered_behind_newer = reentered_behind_newer or (min(new) < max(kept) and want.index(min(new)) > want.index(max(kept)))
    assert erased and reentered_behind_newer
    assert got != sorted(got)  # (an implementation that sorts or rebuilds the list has failed above)


def frames_for_the_map():
    poses = trajectory(6, seed=9)
    kw = dict(n_corner=60, n_surf=500, n_outlier=30)
    fr = [room_scan(300 + i, poses[i], **kw) + (poses[i],) for i in range(6)]
    fr[2] = (fr[2][0], fr[2][1], fr[2][2][:0], fr[2][3])  # a frame without outliers
    fr[4] = (fr[4][0][:1], fr[4][1][:0], fr[4][2][:0], fr[4][3])  # a one-point frame
    return fr, room_scan(399, poses[1], **kw)


@pytest.mark.parametrize("lst", [[], [3], [5, 0, 3], [2, 4], [4], [0, 1, 2, 3, 4, 5]])
def test_surround_map_is_its_two_compositions(host, lst):
    fr, scan = frames_for_the_map()
    got, sizes = host.surround_map(fr, lst, scan)
    corner, ci = host.submap(fr, lst, SUBMAP_CORNER, 0.2)
    surf, si = host.submap(fr, lst, SUBMAP_SURF | SUBMAP_OUTLIER, 0.4)
    scans, ss = host.local_map([], scan)
    assert np.array_equal(bits(got[0]), bits(corner)) and np.array_equal(bits(got[1]), bits(surf))
    for c in range(2, 6):
        assert np.array_equal(bits(got[c]), bits(scans[c])), c
    assert sizes["n"] == [ci["n"], si["n"]] + ss["n"][2:] and sizes["frames"] == len(lst) and sizes["status"] == 0
    assert sizes["box_min"] == [ci["box_min"], si["box_min"]] and sizes["box_dim"] == [ci["box_dim"], si["box_dim"]]
    if lst == [4]:
        assert sizes["n"][:2] == [1, 0]
    if lst == []:
        assert sizes["n"][:2] == [0, 0] and sizes == dict(ss, frames=0)


def test_surround_map_refuses_an_id_that_is_no_frame(host):
    fr, scan = frames_for_the_map()
    for lst in ([6], [-1], [0, 9]):
        with pytest.raises(RuntimeError, match="-1"):
            host.surround_map(fr, lst, scan)


def test_list_rule_text_under_sanitizers(tmp_path):
    exe = str(tmp_path / "surround_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "surround_check.cpp"), "-o", exe])
    text = "".join(" ".join(map(str, lst)) + " | " + " ".join(map(str, ds)) + "\n" for lst, ds, _ in surround_np.CRAFTED)
    run = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()
    got = [[int(v) for v in line.split()] for line in run.stdout.decode().split("\n")[:-1]]
    assert got == [want for _, _, want in surround_np.CRAFTED]
