"""The place-recognition restatement (csrc/host/place.cpp) as a stand-alone program under AddressSanitizer and UBSan
(tests/native/place_check.cpp): the contract's edge cases and a small search, every buffer a heap block of exactly its
size."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lins---lidar-inertial-slam_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("place") / "place_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover", os.path.join(ROOT, "tests", "native", "place_check.cpp"),
                           os.path.join(CSRC, "host", "place.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("name", ["edges", "search"])
def test_case(exe, name):
    run = subprocess.run([exe, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    assert run.stdout.decode() == "ok %s\n" % name
    assert run.stderr == b""  # (a sanitizer report that did not end the program)
