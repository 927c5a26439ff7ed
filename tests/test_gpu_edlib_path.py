"""The edlib drop-in's PATH and LOC tasks (include/edlib.h, edlib_dropin.hip): racon's edlibAlign(NW, TASK_PATH) call from
8 threads, mixed with distance requests in the combining queue (tests/cpp/edlib_path_test.cpp checks every result against
a DP traceback of its own)."""
import os
import subprocess

import numpy as np
import pytest

from raven_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_edlib_path_task_matches_dp_traceback(tmp_path):
    exe = str(tmp_path / "edlib_path_test")
    lib = os.path.join(ROOT, "raven_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "edlib_path_test.cpp"), "-L", lib, "-lraven_hip",
                           "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    g = synth.make_genome(3000, seed=15)
    rng = np.random.default_rng(16)
    seqs = []
    for i in range(49):
        a = int(rng.integers(0, 800))
        piece = synth.mutate(rng, g[a:a + int(rng.integers(200, 1500))], 0.04, 0.03, 0.03)
        if i % 9 == 4:
            piece = piece[:int(rng.integers(0, 4))]  # empty / tiny sequences
        seqs.append(bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[piece]))
    path = tmp_path / "seqs.txt"
    path.write_bytes(b"\n".join(seqs) + b"\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "hw_mode_status 1"
    assert lines[1] == "known check 0 distance 5 cigar 3=2I4=1X2=2D 3M2I7M2D"
    assert lines[2] == "pairs 48 bad 0 first_bad 0"
    assert lines[3] == "k_below -1 1 0"
    assert lines[4] == "k_equal 0"
    assert lines[5] == "loc 0 1 1 0 1"
    assert lines[6] == "loc_no_alignment 1"
