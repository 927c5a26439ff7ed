"""The limits of the rows-on-lanes window kernel on the CPU: raven_amd/csrc/poa4_limits.h compiled for the host
(tests/host/poa4_limits_host.cpp) against their restatement in tests/poa_cases.py (P4_RING, P4_RING_OVF, P4_MAX_D,
P4_EDGES, P4_EDGES_MAX, BANDS[0]), which the crafted window cases are placed by.  The header is the one statement the
kernel goes by (raven_amd/csrc/poa4.hip includes it), so this ties the Python restatement to the kernel."""
import os
import subprocess

from tests import poa_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = ["g++", "-std=c++17", "-I", os.path.join(ROOT, "raven_amd", "csrc")]
SOURCE = os.path.join(ROOT, "tests", "host", "poa4_limits_host.cpp")
NAMES = ("kRing", "kMaxD", "kEdges", "kEdgesMax", "kBand", "G", "GS", "kU")


def header_limits(d):
    exe = os.path.join(str(d), "poa4_limits_host")
    subprocess.check_call(BUILD + ["-O2", "-o", exe, SOURCE])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-3000:])
    pairs = [line.split() for line in run.stdout.splitlines()]
    assert tuple(name for name, _ in pairs) == NAMES, run.stdout
    return {name: int(value) for name, value in pairs}


def test_poa4_limits_match_the_restatement(tmp_path):
    lim = header_limits(tmp_path)
    assert pc.P4_RING == lim["kRing"]
    assert pc.P4_MAX_D == lim["kMaxD"]
    assert pc.P4_EDGES == lim["kEdges"]
    assert pc.P4_EDGES_MAX == lim["kEdgesMax"]
    assert pc.BANDS[0] == lim["kBand"]
    assert pc.P4_RING_OVF == lim["kRing"] - 2
