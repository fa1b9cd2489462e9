"""The consensus rule's scalar text (csrc/host/rendezvous_consensus.h) as a stand-alone program under AddressSanitizer and
UBSan (tests/native/consensus_check.cpp): the contract's corners and seeded tables of every size 0 .. 128 against a
restatement, every table a heap block of exactly its size.  Nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lins---lidar-inertial-slam_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("consensus") / "consensus_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "consensus_check.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("name", ["edges", "random"])
def test_case(exe, name):
    run = subprocess.run([exe, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stdout.decode() + run.stderr.decode()
    assert run.stdout.decode() == "ok %s\n" % name
    assert run.stderr == b""  # (a sanitizer report that did not end the program)
