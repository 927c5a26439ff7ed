"""raven::CreateUnitigs of include/raven_hip/unitigs.hpp (tests/cpp/unitig_facade_test.cpp, g++ against the doubles of
tests/cpp/unitig_doubles.hpp) beside the routine restated on the host in the same program, on the same seeded graphs:
epsilon = 42 and then epsilon = 0 on what the first call left.  Nodes, edges, the iteration order of every `transitive`
set and the sequence names must be identical after each call."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("unitig_facade") / "unitig_facade_test")
    lib = os.path.join(ROOT, "raven_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "unitig_facade_test.cpp"), "-L", lib, "-lraven_hip",
                           "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_facade_equals_the_host_routine(program, seed):
    r = subprocess.run([program, str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "OK" and lines[0].startswith("epsilon 42: ") and lines[1].startswith("epsilon 0: ")
    assert int(lines[0].split()[2]) >= 2 and int(lines[1].split()[2]) >= 4
