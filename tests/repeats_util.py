"""Shared pieces of the ResolveRepeatInducedOverlaps tests: the restatement (tests/host/repeats_reference.cpp, g++ with
the oracle's FindSlopes / MergeRegions / GetOverlapType), the host build of repeats.h (tests/host/repeats_pile.cpp),
their binary input / output format, and generators of piles with planted repeats."""
import os
import subprocess

import numpy as np

from raven_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_reference(tmp_path):
    exe = str(tmp_path / "repeats_reference")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "oracle"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "repeats_reference.cpp"),
                           os.path.join(ROOT, "oracle", "poa_oracle.cpp")])
    return exe


def build_pile_program(tmp_path):
    exe = str(tmp_path / "repeats_pile")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I",
                           os.path.join(ROOT, "raven_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "repeats_pile.cpp")])
    return exe


def _offsets(parts):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return off


class StageInput:
    """The arguments of rvn_resolve_repeat_induced_overlaps."""

    def __init__(self, overlaps, coverage, kmers, begin, end, median, invalid):
        self.overlaps = np.ascontiguousarray(overlaps, dtype=hip.OVERLAP_DTYPE)
        self.coverage_offsets = _offsets(coverage)
        self.coverage = np.concatenate([np.asarray(c, np.uint16) for c in coverage] + [np.zeros(0, np.uint16)])
        self.kmers_offsets = _offsets(kmers)
        self.kmers = np.concatenate([np.asarray(k, np.uint8) for k in kmers] + [np.zeros(0, np.uint8)])
        self.begin = np.asarray(begin, np.uint32)
        self.end = np.asarray(end, np.uint32)
        self.median = np.asarray(median, np.uint16)
        self.invalid = np.asarray(invalid, np.uint8)
        self.n = self.begin.shape[0]

    def write(self, path):
        with open(path, "wb") as f:
            f.write(np.uint32(self.n).tobytes())
            f.write(np.uint64(self.overlaps.shape[0]).tobytes())
            for a in (self.overlaps, self.coverage_offsets, self.coverage, self.kmers_offsets, self.kmers, self.begin,
                      self.end, self.median, self.invalid):
                f.write(np.ascontiguousarray(a).tobytes())

    def device(self, engine):
        return engine.resolve_repeat_induced_overlaps(self.overlaps, self.coverage, self.coverage_offsets, self.kmers,
                                                      self.kmers_offsets, self.begin, self.end, self.median, self.invalid)


def run_program(exe, inp, tmp_path, tag="x"):
    """Runs the restatement (or the host build of repeats.h) on `inp`; returns the dict the device call returns and
    the program's stderr."""
    src, dst = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".out"))
    inp.write(src)
    p = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    b = open(dst, "rb").read()
    n = inp.n
    it, comps = np.frombuffer(b, np.uint32, 2, 0)
    removed, m = np.frombuffer(b, np.uint64, 2, 8)
    pos = 24
    ovl = np.frombuffer(b, hip.OVERLAP_DTYPE, int(m), pos).copy()
    pos += 32 * int(m)
    roff = np.frombuffer(b, np.uint32, n + 1, pos).copy()
    pos += 4 * (n + 1)
    total = int(roff[-1])
    reg = np.frombuffer(b, np.uint32, 2 * total, pos).reshape(-1, 2).copy()
    pos += 8 * total
    isrep = np.frombuffer(b, np.uint8, n, pos).copy()
    assert pos + n == len(b)
    return dict(overlaps=ovl, regions=reg, region_offsets=roff, is_repetitive=isrep, iterations=int(it),
                components=int(comps), removed=int(removed)), p.stderr


def assert_same(got, want):
    for k in ("iterations", "components", "removed"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["overlaps"].shape == want["overlaps"].shape and np.array_equal(got["overlaps"], want["overlaps"])
    assert np.array_equal(got["region_offsets"], want["region_offsets"])
    assert got["regions"].shape == want["regions"].shape and np.array_equal(got["regions"], want["regions"])
    assert np.array_equal(got["is_repetitive"], want["is_repetitive"])


def repeat_profile(rng, cells, median):
    """Coverage of one pile: noise around the median, planted plateaus 1.5 - 3x the median (repeats), pits, ramps at
    the ends, an occasional staircase of nested plateaus (many slope pairs: regions beyond the first try's room)."""
    d = np.full(cells, median, dtype=np.int64) + rng.integers(-2, 3, size=cells)
    for _ in range(int(rng.integers(0, 4))):
        wdt = int(rng.integers(20, max(21, cells // 3)))
        c = int(rng.integers(0, max(1, cells - wdt)))
        d[c:c + wdt] = (d[c:c + wdt] * rng.uniform(1.5, 3.0)).astype(np.int64)
    for _ in range(int(rng.integers(0, 2))):
        c, wdt = int(rng.integers(0, cells)), int(rng.integers(1, 30))
        d[c:c + wdt] = (d[c:c + wdt] * 0.3).astype(np.int64)
    if rng.random() < 0.1 and cells > 1400:  # nested plateaus: every rise pairs with every fall
        steps = int(rng.integers(5, 9))
        step = 60
        start = int(rng.integers(cells // 8, cells // 4))
        lvl = median
        for s in range(steps):
            lvl = lvl * 2
            a, b = start + s * step, cells - start - s * step
            if a < b:
                d[a:b] = lvl
    if rng.random() < 0.5:
        r = int(rng.integers(5, 40))
        d[:r] = (d[:r] * np.linspace(0.1, 1, r)).astype(np.int64)
        d[-r:] = (d[-r:] * np.linspace(1, 0.1, r)).astype(np.int64)
    return np.clip(d, 0, 65535).astype(np.uint16)


def kmer_cells(rng, cells):
    """Pile::kmers_: empty, or (cells + 1) 0/1 cells with runs of set cells just below / above the group size 12 and
    gaps just below / above w = 29."""
    if rng.random() < 0.3:
        return np.zeros(0, np.uint8)
    k = np.zeros(cells + 1, np.uint8)
    pos = int(rng.integers(0, 40))
    while pos < cells:
        count = int(rng.integers(10, 16))
        for _ in range(count):
            if pos >= cells + 1:
                break
            k[pos] = 1
            pos += int(rng.choice([1, 1, 2, 5, 28, 29, 30]))
        pos += int(rng.integers(25, 200))
    return k


def random_piles(rng, n, min_cells=60, max_cells=2000):
    """n piles with planted repeats: coverage, k-mer cells, begin / end in bases (valid regions at or near the edges),
    medians, no invalid pile."""
    cov, kmers, begin, end, median = [], [], [], [], []
    for _ in range(n):
        cells = int(rng.integers(min_cells, max_cells))
        med = int(rng.integers(5, 60))
        d = repeat_profile(rng, cells, med)
        b = int(rng.choice([0, 0, int(rng.integers(0, cells // 10 + 1))]))
        e = int(rng.choice([cells, cells, cells - int(rng.integers(0, cells // 10 + 1))]))
        d[:b] = 0
        d[e:] = 0
        cov.append(d)
        kmers.append(kmer_cells(rng, cells))
        begin.append(b << 4)
        end.append(e << 4)
        median.append(med)
    return cov, kmers, begin, end, median
