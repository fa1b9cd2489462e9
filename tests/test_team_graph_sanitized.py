"""The team graph's text (csrc/pose_graph_team.h) and its CPU restatement as a stand-alone program under AddressSanitizer
and UBSan (tests/native/team_graph_check.cpp): the member table and the supports' bookkeeping against the signs written
out row by row, and small groups solved with every array a heap block of exactly its size.  Nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lins---lidar-inertial-slam_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("team_graph") / "team_graph_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "team_graph_check.cpp"), os.path.join(CSRC, "host", "team_graph.cpp"),
                           os.path.join(CSRC, "host", "pose_graph.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("name", ["tables", "solve"])
def test_case(exe, name):
    run = subprocess.run([exe, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    assert run.stdout.decode() == "ok %s\n" % name
    assert run.stderr == b""  # (a sanitizer report that did not end the program)
