"""The scalar text of the pairwise-consistent team factors (csrc/host/team_pcm.h) as a stand-alone program under
AddressSanitizer and UBSan (tests/native/team_pcm_check.cpp): each bar and one nextafter beyond it — rotation, translation,
the drift term —, the cliques of 64 and 33, the duplicate graphs at the budget's edge, and seeded tables of every size
0 .. 64 against a restatement; every table a heap block of exactly its size, the stack a block of exactly 64 levels.
Nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lins---lidar-inertial-slam_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("team_pcm") / "team_pcm_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "team_pcm_check.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("name", ["edges", "cliques", "random"])
def test_case(exe, name):
    run = subprocess.run([exe, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    assert run.stdout.decode() == "ok %s\n" % name
    assert run.stderr == b""  # (a sanitizer report that did not end the program)
