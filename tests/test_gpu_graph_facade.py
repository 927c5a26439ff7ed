"""The assembly-graph facade (include/raven_hip/assembly_graph.hpp) through tests/cpp/assembly_graph_test.cpp: the
program builds a graph with ConstructAssemblyGraph, reduces it with RemoveTransitiveEdges and MarkLongEdges on the
device, and compares every step with its own pointer-graph restatement (ids, pairs, lengths, every node's `transitive`
iteration order, the return value); it exits non-zero on a difference."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_assembly_graph_facade_matches_its_restatement(tmp_path):
    exe = str(tmp_path / "assembly_graph_test")
    lib = os.path.join(ROOT, "raven_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "tests", "cpp"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "assembly_graph_test.cpp"), "-L", lib, "-lraven_hip",
                           "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, "5", "600"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[0].startswith("construct ") and lines[0].endswith(" differences 0")
    assert lines[1].startswith("transitive removed ") and lines[1].endswith(" differences 0")
    assert lines[2].startswith("long marked ") and lines[2].endswith(" differences 0")
    assert lines[3] == "order_check_throws 1"
