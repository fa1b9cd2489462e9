"""The owning buffer of the C API files (csrc/lins_buf.h), the part that can be held on the CPU: growth, failure, moves and
group growth against a malloc-backed policy that counts and logs its calls and can fail the k-th allocation, as a
stand-alone program under AddressSanitizer and UBSan (tests/native/buf_check.cpp).  The header's upper part is compiled
without ROCm headers; the two HIP policies below it only forward to the runtime."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lins---lidar-inertial-slam_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("buf") / "buf_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-self-move", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover", "-I", CSRC, os.path.join(ROOT, "tests", "native", "buf_check.cpp"), "-o", out])
    return out


def run_case(exe, name):
    run = subprocess.run([exe, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()
    assert run.stdout.decode() == "ok %s\n" % name
    assert run.stderr == b""  # (a sanitizer report that did not end the program)


def test_single_buffer_growth(exe):
    """from empty grow(0) gives capacity 1; a need within capacity touches nothing; a larger one frees, then allocates"""
    run_case(exe, "grow")


def test_failed_allocation_leaves_the_buffer_empty(exe):
    """null and capacity 0 with the error returned, the next growth succeeds, counters balance at exit"""
    run_case(exe, "fail")


def test_moves_leave_the_source_empty(exe):
    """move construction and assignment; a default-constructed struct of three buffers assigned over a filled one frees three blocks"""
    run_case(exe, "move")


def test_group_growth_is_all_or_none(exe):
    """all grow when the first is short, none when it suffices; a failing second allocation leaves all three empty"""
    run_case(exe, "group")


def test_an_unknown_case_is_refused(exe):
    assert subprocess.run([exe, "nothing"], stdout=subprocess.DEVNULL).returncode == 2
