"""Shared pieces of the ResolveContainedReads / ResolveChimericSequences tests: the restatement
(tests/host/resolve_reference.cpp, g++ with the oracle's OverlapUpdate / GetOverlapType / identity score), the host build
of chimeric.h (tests/host/resolve_pile.cpp), their binary input / output format, generators of piles with planted dips and
of overlap lists against them, and the count of ClearChimericRegions' outcomes."""
import os
import subprocess

import numpy as np

from raven_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_reference(tmp_path):
    exe = str(tmp_path / "resolve_reference")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "oracle"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "resolve_reference.cpp"),
                           os.path.join(ROOT, "oracle", "poa_oracle.cpp")])
    return exe


def build_pile_program(tmp_path):
    exe = str(tmp_path / "resolve_pile")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I",
                           os.path.join(ROOT, "raven_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "resolve_pile.cpp")])
    return exe


def _offsets(parts, dtype):
    off = np.zeros(len(parts) + 1, dtype=dtype)
    if len(parts):
        off[1:] = np.cumsum([len(p) for p in parts])
    return off


def _concat(parts, dtype):
    return np.concatenate([np.asarray(p, dtype) for p in parts] + [np.zeros(0, dtype)])


class StageInput:
    """The arguments of rvn_resolve_contained_and_chimeric: per-pile lists of overlaps, coverage arrays and region lists
    ((k, 2) cells), begin / end in cells, median, invalid."""

    def __init__(self, lists, coverage, regions, begin, end, median, invalid, reads=None):
        self.overlaps = _concat(lists, hip.OVERLAP_DTYPE)
        self.offsets = _offsets(lists, np.uint32)
        self.coverage = _concat(coverage, np.uint16)
        self.coverage_offsets = _offsets(coverage, np.uint64)
        self.regions = _concat([np.asarray(r, np.uint32).reshape(-1) for r in regions], np.uint32).reshape(-1, 2)
        self.region_offsets = _offsets(regions, np.uint32)
        self.begin = np.asarray(begin, np.uint32)
        self.end = np.asarray(end, np.uint32)
        self.median = np.asarray(median, np.uint16)
        self.invalid = np.asarray(invalid, np.uint8)
        self.n = self.begin.shape[0]
        self.reads = reads  # seqio.ReadSet: needed when identity != 0

    @classmethod
    def from_csr(cls, overlaps, offsets, coverage, coverage_offsets, regions, begin, end, median, invalid, reads=None):
        n = len(begin)
        return cls([overlaps[int(offsets[i]):int(offsets[i + 1])] for i in range(n)],
                   [coverage[int(coverage_offsets[i]):int(coverage_offsets[i + 1])] for i in range(n)],
                   regions, begin, end, median, invalid, reads)

    def write(self, path, phases, identity):
        with open(path, "wb") as f:
            f.write(np.uint32(self.n).tobytes())
            f.write(np.uint32(phases).tobytes())
            f.write(np.float64(identity).tobytes())
            for a in (self.offsets, self.overlaps, self.coverage_offsets, self.coverage, self.region_offsets, self.regions,
                      self.begin, self.end, self.median, self.invalid):
                f.write(np.ascontiguousarray(a).tobytes())
            if identity != 0:
                rs = self.reads
                nw = int(rs.word_offsets[-1])
                words = np.zeros(nw + 1, np.uint64)
                words[:nw] = np.asarray(rs.packed, np.uint64)[:nw]
                f.write(np.ascontiguousarray(rs.word_offsets, np.uint64).tobytes())
                f.write(np.ascontiguousarray(rs.lengths, np.uint32).tobytes())
                f.write(words.tobytes())

    def device(self, engine, phases=3, identity=0.0, reads=None):
        return engine.resolve_contained_and_chimeric(self.overlaps, self.offsets, self.coverage, self.coverage_offsets,
                                                     self.regions, self.region_offsets, self.begin, self.end, self.median,
                                                     self.invalid, reads=reads, identity=identity, phases=phases)


def run_program(exe, inp, tmp_path, tag="x", phases=3, identity=0.0, mode="stage"):
    """Runs the restatement (mode "stage" / "piles") or the host build of chimeric.h (mode None) on `inp`; returns the
    dict the device calls return."""
    src, dst = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".out"))
    inp.write(src, phases, identity)
    p = subprocess.run([exe] + ([mode] if mode else []) + [src, dst], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    b = open(dst, "rb").read()
    n = inp.n
    pos = 0

    def take(dtype, count):
        nonlocal pos
        a = np.frombuffer(b, dtype, count, pos).copy()
        pos += a.nbytes
        return a

    begin, end = take(np.uint32, n), take(np.uint32, n)
    invalid, contained, chimeric = take(np.uint8, n), take(np.uint8, n), take(np.uint8, n)
    roff = take(np.uint32, n + 1)
    reg = take(np.uint32, 2 * int(roff[-1])).reshape(-1, 2)
    median = int(take(np.uint16, 1)[0])
    m = int(take(np.uint64, 1)[0])
    ovl = take(hip.OVERLAP_DTYPE, m)
    off = take(np.uint32, n + 1)
    cov = take(np.uint16, inp.coverage.shape[0])
    s64 = take(np.uint64, 4)
    s32 = take(np.uint32, 4)
    assert pos == len(b)
    return dict(begin=begin, end=end, invalid=invalid, contained=contained, chimeric=chimeric, regions=reg,
                region_offsets=roff, median=median, overlaps=ovl, offsets=off, coverage=cov,
                stats=dict(dropped_by_update=(int(s64[0]), int(s64[1])), dropped_by_filter=int(s64[2]),
                           dropped_by_containment=int(s64[3]), contained=(int(s32[0]), int(s32[1])), cut=int(s32[2]),
                           invalidated=int(s32[3])))


PILE_FIELDS = ("begin", "end", "invalid", "contained", "chimeric", "region_offsets", "regions")


def assert_same(got, want, coverage=True, lists=True, stats=True, median=True):
    """Field by field, byte by byte."""
    for k in PILE_FIELDS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    if median:
        assert got["median"] == want["median"], (got["median"], want["median"])
    if lists:
        assert np.array_equal(got["offsets"], want["offsets"])
        assert got["overlaps"].shape == want["overlaps"].shape and np.array_equal(got["overlaps"], want["overlaps"])
    if coverage:
        assert got["coverage"].shape == want["coverage"].shape and np.array_equal(got["coverage"], want["coverage"])
    if stats:
        assert got["stats"] == want["stats"], (got["stats"], want["stats"])


def chimeric_piles(rng, n, region_free=0.0):
    """n piles for ClearChimericRegions: 100 to 1500 cells, the valid region up to an eighth of the pile short of either
    end, Poisson coverage with a mean of 20 to 60 and zero outside the region, one to four disjoint regions of up to 40
    cells anywhere in the pile (none in a share `region_free` of the piles), a dip to a random depth below the mean
    planted in 60 % of them, a median of 10 to 70."""
    cov, regions, begin, end, median = [], [], [], [], []
    for _ in range(n):
        cells = int(rng.integers(100, 1501))
        b = int(rng.integers(0, cells // 8 + 1))
        e = cells - int(rng.integers(0, cells // 8 + 1))
        mean = float(rng.uniform(20, 60))
        d = rng.poisson(mean, cells).astype(np.int64)
        regs = []
        if rng.random() >= region_free:
            cuts = np.sort(rng.choice(np.arange(cells), size=2 * int(rng.integers(1, 5)), replace=False))
            for k in range(0, cuts.shape[0], 2):
                first = int(cuts[k])
                second = min(int(cuts[k + 1]), first + int(rng.integers(0, 40)))
                regs.append((first, second))
                if rng.random() < 0.6:
                    depth = rng.uniform(0, mean)
                    at = int(rng.integers(first, second + 1))
                    w = int(rng.integers(1, 6))
                    d[max(first, at - w):min(second, at + w) + 1] = rng.poisson(depth, min(second, at + w) + 1 - max(first, at - w))
        d[:b] = 0
        d[e:] = 0
        cov.append(np.clip(d, 0, 65535).astype(np.uint16))
        regions.append(np.array(regs, np.uint32).reshape(-1, 2))
        begin.append(b)
        end.append(e)
        median.append(int(rng.integers(10, 71)))
    return cov, regions, begin, end, median


def overlap_lists(rng, begin, end, lengths, per_pile=6):
    """Per-pile lists against the piles' valid regions (cells): a mix of overlaps that span a whole valid region (containment
    candidates), dovetails at either end and internal matches, both strands; coordinates in bases."""
    n = len(begin)
    lists = []
    for i in range(n):
        rows = []
        for _ in range(int(rng.integers(0, 2 * per_pile))):
            j = int(rng.integers(0, n))
            if j == i:
                continue
            lb, le = int(begin[i]) << 4, int(end[i]) << 4
            rb, re = int(begin[j]) << 4, int(end[j]) << 4
            strand = int(rng.integers(0, 2))
            kind = rng.random()
            if kind < 0.35:      # all of pile i's region inside pile j's
                span = le - lb
                if re - rb < span:
                    lb, le, span = lb, lb + (re - rb), re - rb
                s = rb + int(rng.integers(0, re - rb - span + 1))
                o = (lb, le, s, s + span)
            elif kind < 0.7:     # tail of i on head of j (or the mirror image)
                span = int(rng.integers(100, max(101, min(le - lb, re - rb))))
                span = min(span, le - lb, re - rb)
                o = (le - span, le, rb, rb + span) if rng.random() < 0.5 else (lb, lb + span, re - span, re)
            else:                # somewhere inside both
                span = int(rng.integers(50, max(51, min(le - lb, re - rb) // 2 + 51)))
                span = min(span, le - lb, re - rb)
                a = lb + int(rng.integers(0, le - lb - span + 1))
                c = rb + int(rng.integers(0, re - rb - span + 1))
                o = (a, a + span, c, c + span)
            rows.append((i, o[0], o[1], j, o[2], o[3], int(rng.integers(0, 1000)), strand))
        lists.append(np.array(rows, dtype=hip.OVERLAP_DTYPE) if rows else np.zeros(0, hip.OVERLAP_DTYPE))
    return lists


OUTCOMES = ("skipped", "resolved", "unresolved", "cut_head", "cut_tail", "cut_both", "unchanged", "invalid")


def count_outcomes(inp, out, skip=None):
    """Piles with each outcome of ClearChimericRegions, from a stage input and a result: a region that leaves the valid
    region (skipped), a region that is gone without having been skipped (resolved), a region that stays (unresolved);
    the valid region cut at the head, at the tail, on both sides, unchanged; the pile made invalid by the 78-cell rule.
    skip[i]: ClearChimericRegions did not see pile i (invalid before phase 2)."""
    c = dict.fromkeys(OUTCOMES, 0)
    for i in range(inp.n):
        if inp.invalid[i] or (skip is not None and skip[i]):
            continue
        regs = inp.regions[int(inp.region_offsets[i]):int(inp.region_offsets[i + 1])]
        b, e = int(inp.begin[i]), int(inp.end[i])
        skipped = sum(1 for f, s in regs if b > f or e < s)
        left = int(out["region_offsets"][i + 1]) - int(out["region_offsets"][i])
        c["skipped"] += skipped > 0
        c["unresolved"] += left > 0
        c["resolved"] += len(regs) - skipped - left > 0
        if out["invalid"][i] and not out["contained"][i]:
            c["invalid"] += 1
            continue
        nb, ne = int(out["begin"][i]), int(out["end"][i])
        head, tail = nb != b, ne != e
        c["cut_both"] += head and tail
        c["cut_head"] += head and not tail
        c["cut_tail"] += tail and not head
        c["unchanged"] += not head and not tail
    return c


def oracle_trimmed_input(rs):
    """The state TrimAndAnnotatePiles (construct.cc:123-152) leaves, stated with the oracle's primitives: the first pass,
    FindValidRegion(4) + FindMedian, FindChimericRegions of the valid piles; the lists of invalid piles emptied."""
    from oracle import oracle
    n = rs.n
    p1 = oracle.Engine(15, 5).find_overlaps_and_create_piles(rs, freq=0.001, kmax=32, use_minhash=False)
    poff, ooff = p1["pile_offsets"], p1["overlap_offsets"]
    data = [p1["pile_data"][int(poff[i]):int(poff[i + 1])].copy() for i in range(n)]
    lists = [p1["overlaps"][int(ooff[i]):int(ooff[i + 1])].copy() for i in range(n)]
    begin, end = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    median, invalid = np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    regions = [np.zeros((0, 2), np.uint32) for _ in range(n)]
    for i in range(n):
        b, e, m, inv = oracle.pile_trim_and_median(data[i], 4)
        if inv:
            begin[i], end[i], invalid[i] = 0, data[i].shape[0], 1
            lists[i] = lists[i][:0]
        else:
            begin[i], end[i], median[i] = b, e, m
            regions[i] = np.asarray(oracle.find_chimeric_regions(data[i]), np.uint32).reshape(-1, 2)
    return StageInput(lists, data, regions, begin, end, median, invalid, reads=rs)
