"""Pile::FindChimericRegions as the kernel runs it (raven_amd/csrc/slopes.h through rvn_test_find_chimeric_regions, host
side of the same __host__ __device__ code: windowed scans instead of deques) against the oracle's restatement of
RavenLib/src/pile.cc:176-187, :373-400, :403-600 with the reference's own deques / std::sort / vectors, on synthetic
coverage profiles: plateaus with pits (chimeric junctions), spikes (repeats), ramps, noise, zeroed ends."""
import numpy as np

from oracle import oracle
from raven_amd import hip
from tests.pile_cases import profile as _profile  # (shared with the crafted piles of the device tests)


def test_find_chimeric_regions_matches_the_restatement_of_pile_cc():
    rng = np.random.default_rng(2026)
    n_regions = 0
    n_with = 0
    for trial in range(3000):
        cells = int(rng.integers(130, 1500))
        d = _profile(rng, cells)
        got = hip.test_find_chimeric_regions(d)
        want = oracle.find_chimeric_regions(d)
        assert got.shape == want.shape and np.array_equal(got, want), (trial, got, want)
        n_regions += got.shape[0]
        n_with += got.shape[0] > 0
    assert n_with > 500 and n_regions > 700  # the generator does produce pits the rule accepts


def test_flat_and_degenerate_profiles():
    for d in (np.full(100, 30, np.uint16), np.zeros(200, np.uint16), np.arange(300, dtype=np.uint16),
              np.arange(300, dtype=np.uint16)[::-1].copy(), np.full(90, 65535, np.uint16)):
        assert np.array_equal(hip.test_find_chimeric_regions(d), oracle.find_chimeric_regions(d))
    d = np.full(400, 40, np.uint16)
    d[200:203] = 3  # one clean pit
    got = hip.test_find_chimeric_regions(d)
    assert got.shape[0] == 1 and got[0, 0] <= 200 and got[0, 1] >= 202
    assert np.array_equal(got, oracle.find_chimeric_regions(d))
