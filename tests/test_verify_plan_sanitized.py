"""The layout of the steps' assemble-and-align stage (csrc/host/verify_plan.h) as a stand-alone program under
AddressSanitizer and UBSan (tests/native/verify_plan_check.cpp): the four layouts the steps had each written out by hand,
the window ids at their clips, the status rules, and seeded tables, against a restatement; every array a heap block of
exactly its size.  Nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lins---lidar-inertial-slam_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("verify_plan") / "verify_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "verify_plan_check.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("name", ["shapes", "status", "random"])
def test_case(exe, name):
    run = subprocess.run([exe, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    assert run.stdout.decode() == "ok %s\n" % name
    assert run.stderr == b""  # (a sanitizer report that did not end the program)
