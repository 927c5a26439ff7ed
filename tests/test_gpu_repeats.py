"""raven::ResolveRepeatInducedOverlaps on the device (rvn_resolve_repeat_induced_overlaps, raven_amd/csrc/repeats.hip)
bit-exact against the single-threaded restatement of RavenLib/src/construct.cc:493-559 (tests/host/repeats_reference.cpp):
surviving overlaps in order, every pile's regions with their flag bits, is_repetitive and the loop's counts — on the
device chain of a synthetic genome with planted repeats, on hand-built arrays, and through the C++ facade."""
import os
import subprocess

import numpy as np
import pytest

from raven_amd import hip, seqio, synth
from tests import repeats_util as ru

pytestmark = pytest.mark.gpu

ROOT = ru.ROOT


def _repeat_rich_genome(n, seed, copies=12, element=6000, div=0.015):
    """n bases with a 4-8 kb element copied `copies` times at 1-2 % divergence and low-complexity arrays (k-mer cells)."""
    rng = np.random.default_rng(seed)
    g = synth.make_genome(n, seed=seed)
    for e in range(max(1, n // 1_000_000)):
        rep = g[1000 + e * 50_000:1000 + e * 50_000 + element].copy()
        for c in range(copies):
            at = int(rng.integers(0, n - element))
            m = synth.mutate(rng, rep, div, 0.0, 0.0)[:element]
            g[at:at + m.shape[0]] = m
    for _ in range(max(2, n // 200_000)):  # tandem arrays of a short unit
        unit = rng.integers(0, 4, size=int(rng.integers(2, 7)), dtype=np.uint8)
        at, ln = int(rng.integers(0, n - 3000)), int(rng.integers(600, 3000))
        g[at:at + ln] = np.tile(unit, ln // unit.shape[0] + 1)[:ln]
    return g


def _chain_input(eng, rs, identity=0.0, seed=7):
    """First pass -> valid regions / medians -> second pass on the device: the host state the stage starts from.  Some
    piles are made invalid as ResolveContainedReads would (the second pass maps nothing when every pile is valid,
    construct.cc:343-349)."""
    rd = eng.upload(rs)
    p = eng.find_overlaps_and_create_piles(rd)
    b, e, median, invalid = p.trim_and_annotate(4)
    data, off = p.piles()
    p.close()
    begin, end = b.astype(np.uint32) << 4, e.astype(np.uint32) << 4
    invalid = (invalid | (np.random.default_rng(seed).random(rs.n) < 0.15)).astype(np.uint8)
    res = eng.find_overlaps_and_repetitive_regions(rd, begin, end, invalid, freq=0.001, kmer_len=15, identity=identity)
    invalid = (invalid | res["contained"]).astype(np.uint8)  # construct.cc:466-470
    cov = [data[int(off[i]):int(off[i + 1])] for i in range(rs.n)]
    rd.close()
    return ru.StageInput(res["overlaps"], cov, res["kmers"], begin, end, median, invalid)


def test_chain_with_planted_repeats_matches_the_restatement(tmp_path):
    ref = ru.build_reference(tmp_path)
    g = _repeat_rich_genome(2_000_000, seed=11)
    rs, _ = synth.make_reads(g, 30, 10000, seed=12)
    eng = hip.Engine(15, 5)
    inp = _chain_input(eng, rs)
    got = inp.device(eng)
    want, _ = ru.run_program(ref, inp, tmp_path, "chain")
    ru.assert_same(got, want)
    assert got["removed"] > 0 and got["iterations"] >= 2  # not vacuous: overlaps removed, the loop ran again
    assert got["is_repetitive"].sum() > 0 and (got["regions"][:, 0] & 1).sum() > 0


def _tiled_reads(genome, read_len, step):
    """Error-free reads every `step` bases: flat coverage, no repeat anywhere."""
    starts = np.arange(0, genome.shape[0] - read_len, step)
    codes = np.concatenate([genome[a:a + read_len] for a in starts])
    lengths = np.full(starts.shape[0], read_len, np.uint32)
    words, woff = synth._pack_many(codes, lengths)
    return seqio.ReadSet(np.concatenate([words, np.zeros(1, np.uint64)]), woff.astype(np.uint64), lengths,
                         np.arange(starts.shape[0], dtype=np.uint32))


def test_repeat_free_input_removes_nothing(tmp_path):
    ref = ru.build_reference(tmp_path)
    g = synth.make_genome(400_000, seed=21)
    rs = _tiled_reads(g, 8000, 800)
    eng = hip.Engine(15, 5)
    inp = _chain_input(eng, rs, identity=0.0)
    got = inp.device(eng)
    want, _ = ru.run_program(ref, inp, tmp_path, "free")
    ru.assert_same(got, want)
    assert got["removed"] == 0 and got["iterations"] == 1 and got["overlaps"].shape[0] > 100


def _ovl(l, lb, le, r, rb, re, strand=1):
    return (l, lb, le, r, rb, re, 0, strand)


def test_hand_built_arrays(tmp_path):
    """Many small components and a large one, isolated piles, overlaps of type <= 2, a self-overlap, an invalid pile
    reached through an edge, piles longer than the wave's LDS copy and a pile whose regions exceed the first try."""
    ref = ru.build_reference(tmp_path)
    rng = np.random.default_rng(5)
    cov, kmers, begin, end, median = ru.random_piles(rng, 400, min_cells=300, max_cells=1200)
    # long piles (lane 0's serial path) and a staircase of nested plateaus (more than 32 regions before the merge)
    for i in (3, 77, 250):
        cells = 4096 + 700 * (i % 3) + 1
        cov[i] = ru.repeat_profile(rng, cells, 20)
        kmers[i] = ru.kmer_cells(rng, cells)
        begin[i], end[i] = 0, cells << 4
    cells, lvl = 1800, 10
    d = np.full(cells, lvl, np.uint16)
    for s in range(10):
        lvl *= 2
        d[300 + 60 * s:cells - 300 - 60 * s] = min(lvl, 60000)
    cov[10], kmers[10], begin[10], end[10], median[10] = d, np.zeros(0, np.uint8), 0, cells << 4, 5
    n = len(cov)
    invalid = np.zeros(n, np.uint8)
    invalid[[20, 21, 399]] = 1
    L = [(end[i] - begin[i]) for i in range(n)]
    ovl = []
    for a in range(0, 200, 4):  # small components: chains of 4 dovetails (type 3 / 4)
        for b in range(a, a + 3):
            la, lb = L[b], L[b + 1]
            ovl.append(_ovl(b, begin[b] + la // 2, end[b], b + 1, begin[b + 1], begin[b + 1] + la - la // 2, 1))
    for b in range(200, 360):  # one large component
        c = 200 + (b * 7919) % 160
        if c != b:
            la = L[b]
            ovl.append(_ovl(b, begin[b] + la // 3, end[b], c, begin[c], begin[c] + min(L[c], la - la // 3), 1))
    ovl.append(_ovl(19, begin[19] + L[19] // 2, end[19], 20, begin[20], begin[20] + L[19] - L[19] // 2))  # invalid 20
    ovl.append(_ovl(30, begin[30] + 100, begin[30] + 200, 31, begin[31] + 100, begin[31] + 200))  # internal: type 0
    ovl.append(_ovl(40, begin[40], end[40], 41, begin[41], begin[41] + L[40]))  # containment: type <= 2
    ovl.append(_ovl(50, begin[50] + L[50] // 2, end[50], 50, begin[50], begin[50] + L[50] - L[50] // 2))  # self
    ovl.append(_ovl(10, begin[10] + 200 * 16, end[10], 60, begin[60], begin[60] + 1000 * 16, 0))
    ovl = np.array(ovl, dtype=hip.OVERLAP_DTYPE)
    inp = ru.StageInput(ovl, cov, kmers, begin, end, median, invalid)
    eng = hip.Engine(15, 5)
    got = inp.device(eng)
    want, _ = ru.run_program(ref, inp, tmp_path, "hand")
    ru.assert_same(got, want)
    assert got["components"] > 50 and np.diff(got["region_offsets"]).max() > 0
    # the staircase pile: more than 32 regions before the merge (the retry path), one region after it
    assert got["is_repetitive"][10] == 1
    empty = ru.StageInput(np.zeros(0, hip.OVERLAP_DTYPE), [], [], [], [], [], [])
    e = empty.device(eng)
    assert e["overlaps"].shape[0] == 0 and e["regions"].shape[0] == 0 and e["iterations"] == 1


def test_facade_program_matches_the_restatement(tmp_path):
    ref = ru.build_reference(tmp_path)
    lib = os.path.join(ROOT, "raven_amd", "lib")
    exe = str(tmp_path / "repeats_stage_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "tests", "cpp"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "repeats_stage_test.cpp"), "-L", lib, "-lraven_hip",
                           "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    g = _repeat_rich_genome(1_000_000, seed=31)
    rs, _ = synth.make_reads(g, 30, 10000, seed=32)
    eng = hip.Engine(15, 5)
    inp = _chain_input(eng, rs)
    eng.close()
    got, _ = ru.run_program(exe, inp, tmp_path, "facade")
    want, _ = ru.run_program(ref, inp, tmp_path, "facade_ref")
    got["iterations"], got["components"] = want["iterations"], want["components"]  # the facade reports no loop counts
    ru.assert_same(got, want)
    assert want["removed"] > 0
