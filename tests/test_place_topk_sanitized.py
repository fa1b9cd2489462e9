"""lins_host_place_topk and lins_host_loop_choose as a stand-alone program under AddressSanitizer and UBSan
(tests/native/place_topk_check.cpp): every buffer a heap block of exactly its size, the k results of an entry whose ranks
fall short of k included.  Nothing is preloaded and nothing of it runs on a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lins---lidar-inertial-slam_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("place_topk") / "place_topk_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover", os.path.join(ROOT, "tests", "native", "place_topk_check.cpp"),
                           os.path.join(CSRC, "host", "place.cpp"), os.path.join(CSRC, "host", "loop_icp.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("name", ["topk", "choose"])
def test_case(exe, name):
    run = subprocess.run([exe, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    assert run.stdout.decode() == "ok %s\n" % name
    assert run.stderr == b""  # (a sanitizer report that did not end the program)
