"""Pile::FindRepetitiveRegions as the device runs it (raven_amd/csrc/repeats.h, compiled for the host by
tests/host/repeats_pile.cpp) against the restatement of RavenLib/src/pile.cc:230-317 and construct.cc:493-559
(tests/host/repeats_reference.cpp, with the oracle's FindSlopes / MergeRegions), on piles with planted repeat plateaus,
k-mer cell runs around the group size, valid regions at the edges and empty kmers_; and the C++ facade of the stage
compiled against its test double."""
import os
import subprocess

import numpy as np

from tests import repeats_util as ru

ROOT = ru.ROOT


def test_find_repetitive_regions_matches_the_restatement(tmp_path):
    ref, pile = ru.build_reference(tmp_path), ru.build_pile_program(tmp_path)
    rng = np.random.default_rng(2027)
    cov, kmers, begin, end, median = ru.random_piles(rng, 3000)
    inp = ru.StageInput(np.zeros(0, ru.hip.OVERLAP_DTYPE), cov, kmers, begin, end, median, np.zeros(len(cov), np.uint8))
    want, _ = ru.run_program(ref, inp, tmp_path, "ref")
    got, _ = ru.run_program(pile, inp, tmp_path, "pile")
    ru.assert_same(got, want)
    per_pile = np.diff(want["region_offsets"].astype(np.int64))
    # not vacuous: many repetitive piles, several regions per pile, piles beyond the host program's first try of 8
    assert want["is_repetitive"].sum() > 1000
    assert (per_pile > 1).sum() > 100 and per_pile.max() > 8
    assert (want["regions"][:, 0] & 1).sum() == 0  # no UpdateRepetitiveRegions without overlaps


def test_degenerate_piles(tmp_path):
    ref, pile = ru.build_reference(tmp_path), ru.build_pile_program(tmp_path)
    cov = [np.zeros(0, np.uint16), np.full(100, 30, np.uint16), np.zeros(200, np.uint16),
           np.arange(300, dtype=np.uint16), np.full(90, 65535, np.uint16), np.full(500, 20, np.uint16)]
    cov[5][200:300] = 60  # one clean plateau at 3x the median
    kmers = [np.zeros(0, np.uint8), np.ones(101, np.uint8), np.zeros(201, np.uint8), np.zeros(0, np.uint8),
             np.ones(91, np.uint8), np.zeros(0, np.uint8)]
    begin = [0, 0, 0, 16 * 10, 0, 0]
    end = [16 * len(c) for c in cov]
    inp = ru.StageInput(np.zeros(0, ru.hip.OVERLAP_DTYPE), cov, kmers, begin, end, [20] * 6, [0, 0, 0, 0, 1, 0])
    want, _ = ru.run_program(ref, inp, tmp_path, "ref")
    got, _ = ru.run_program(pile, inp, tmp_path, "pile")
    ru.assert_same(got, want)
    assert want["is_repetitive"][5] == 1 and want["is_repetitive"][1] == 1 and want["is_repetitive"][4] == 0


def test_repeats_facade_compiles_against_its_double(tmp_path):
    lib = os.path.join(ROOT, "raven_amd", "lib")
    exe = str(tmp_path / "repeats_stage_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "tests", "cpp"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "repeats_stage_test.cpp"), "-L", lib, "-lraven_hip",
                           "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
