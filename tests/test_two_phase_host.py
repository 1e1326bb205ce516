"""The rule of the step between the phases (linear-programming_amd/csrc/two_phase_host.h: feasibility test, entering
column of a drive-out, the drive-out loop), without a GPU: tests/two_phase_check.cpp built with the host compiler alone
under AddressSanitizer and UBSan -- the header needs no HIP -- and run as a program.  The one copy serves the double,
the single-float and the exact hand-overs, so the program runs every check with a double, a float and an integer type."""
import os
import shutil
import subprocess

import pytest

from tests.helpers import ROOT

GROUPS = (["feasible-%s" % t for t in ("double", "float")] +
          ["entering-column-%s" % t for t in ("double", "float", "int", "ieee-double", "ieee-float")] +
          ["drive-out-%s" % t for t in ("double", "float", "int")])


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("two_phase") / "two_phase_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "two_phase_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert not p.stderr, p.stderr[-2000:]
    return p.returncode, p.stdout.splitlines()


def test_every_check_holds(output):
    rc, lines = output
    assert [l for l in lines if l.startswith("FAIL")] == [] and rc == 0
    assert lines[-1] == "0 failed"


@pytest.mark.parametrize("group", GROUPS)
def test_group_ran(output, group):
    assert "ran " + group in output[1]


def test_the_header_is_host_only():
    """No HIP header, nothing but the status codes and the standard library: a plain host compiler takes it."""
    src = open(os.path.join(ROOT, "linear-programming_amd", "csrc", "two_phase_host.h")).read()
    includes = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert sorted(includes) == ['"../../include/mi355x_simplex.h"', "<algorithm>", "<cstdint>", "<vector>"]
