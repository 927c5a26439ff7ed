"""GPU parity of rvn_edit_distance_batch (edlibAlign default config == global unit-cost edit distance) against
the textbook DP of the oracle, pair by pair.  Parity here is pinned by definition (any exact algorithm returns the
same number).  Which stage of edit_distance_dev a test reaches (asserted by launch counts per kernel site where noted):
  small_and_edges, long_reads_and_band_doubling, beyond_ring_capacity   < 2048 pairs: everything is "the sample" (widest
      lane window), then the wave kernel (band doubling) and the unbanded stripes;
  hifi_mix_runs_every_stage_*   > 2048 pairs: sample, the three window classes (3 / 5 / 7 slots), the second chance with the
      widest window, wave kernel, stripes — and the same batch in another order;
  batch_the_sample_turns_down   the sample's verdict "no": the main part skips the lane kernel;
  n_main_zero_one_two           2048 / 2049 / 2050 pairs;
  bounded_mode_on_the_hifi_shape   kmax through Engine.filter_overlaps_by_identity against oracle.identity_filter.
The lane kernel's per-pair code is also stepped on the CPU against the same DP (tests/test_ed_lane.py).
The routes' own edges — thresholds and capacity of the wave ring, its wraps, the workgroup ring, the stripes of the full
sweep, bounded thresholds, list sizes — are crafted in tests/ed_ring_cases.py and run by tests/test_gpu_ed_ring_cases.py."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip, seqio, synth

pytestmark = pytest.mark.gpu

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _mutate(rng, codes, sub, ins, dele):
    out = []
    for c in codes:
        u = rng.random()
        if u < dele:
            continue
        if u < dele + sub:
            c = (c + rng.integers(1, 4)) & 3
        out.append(c)
        if rng.random() < ins:
            out.append(rng.integers(0, 4))
    return np.array(out, dtype=np.uint8)


def _want(rs, p):
    a = rs.inflate(int(p["lhs_read"]))[int(p["lhs_begin"]): int(p["lhs_begin"]) + int(p["lhs_len"])]
    b = rs.inflate(int(p["rhs_read"]))[int(p["rhs_begin"]): int(p["rhs_begin"]) + int(p["rhs_len"])]
    if not p["strand"]:
        b = b.translate(COMP)[::-1]
    return oracle.edit_distance(a, b)


def _check(eng, rd, rs, pairs):
    got, ms, cells = eng.edit_distance_batch(rd, pairs)
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:  # (the oracle's DP runs outside the interpreter lock)
        wants = list(ex.map(lambda p: _want(rs, p), pairs))
    for i, p in enumerate(pairs):
        assert int(got[i]) == wants[i], (i, p, int(got[i]), wants[i])
    return ms, cells


def _pair(a, ab, al, b, bb, bl, strand):
    return (a, ab, al, b, bb, bl, strand, 0)


def test_edit_distance_small_and_edges():
    rng = np.random.default_rng(1)
    base = rng.integers(0, 4, size=700, dtype=np.uint8)
    reads = [base, _mutate(rng, base, 0.05, 0.03, 0.03), (3 - base)[::-1].copy(), rng.integers(0, 4, size=500, dtype=np.uint8),
             np.zeros(300, np.uint8), np.tile(np.array([0, 1], np.uint8), 200)]
    rs = seqio.pack_reads(reads)
    eng = hip.Engine()
    rd = eng.upload(rs)
    P = []
    for n in (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300, 700):
        P.append(_pair(0, 0, n, 1, 0, min(n + 3, len(reads[1])), 1))
        P.append(_pair(0, 5, max(0, n - 5), 0, 5, max(0, n - 5), 1))  # identical spans -> 0
        P.append(_pair(0, 0, n, 2, 700 - n, n, 0))                    # rc of the rc -> identical -> 0
        P.append(_pair(0, 0, n, 3, 0, min(n, 500), 1))                # unrelated
        P.append(_pair(4, 0, min(n, 300), 5, 0, min(n, 400), 1))      # homopolymer vs dinucleotide repeat
        P.append(_pair(0, 0, n, 1, 0, 0, 1))                          # against the empty string
    P.append(_pair(3, 17, 401, 1, 33, 555, 0))
    pairs = np.array(P, dtype=hip.ED_PAIR_DTYPE)
    _check(eng, rd, rs, pairs)


def test_edit_distance_long_reads_and_band_doubling():
    rng = np.random.default_rng(2)
    base = rng.integers(0, 4, size=9000, dtype=np.uint8)
    reads = [base,
             _mutate(rng, base, 0.002, 0.001, 0.001),   # HiFi-like: ed ~ 36  (first band suffices)
             _mutate(rng, base, 0.04, 0.03, 0.03),      # ONT-like: ed ~ 900 (several doublings)
             _mutate(rng, base, 0.10, 0.08, 0.08),      # two noisy reads: ed ~ 2300
             (3 - _mutate(rng, base, 0.04, 0.03, 0.03))[::-1].copy()]
    rs = seqio.pack_reads(reads)
    eng = hip.Engine()
    rd = eng.upload(rs)
    P = [_pair(0, 0, 9000, i, 0, int(rs.lengths[i]), 1) for i in (1, 2, 3)]
    P.append(_pair(0, 0, 9000, 4, 0, int(rs.lengths[4]), 0))
    P.append(_pair(1, 100, 5000, 2, 90, 5100, 1))
    P.append(_pair(2, 0, 4097, 3, 0, 4095, 1))
    P.append(_pair(0, 0, 9000, 1, 0, 2000, 1))  # very different lengths: k starts at |n-m|
    pairs = np.array(P, dtype=hip.ED_PAIR_DTYPE)
    ms, cells = _check(eng, rd, rs, pairs)
    assert cells == sum(int(p["lhs_len"]) * int(p["rhs_len"]) for p in pairs)


def test_edit_distance_beyond_ring_capacity():
    """unrelated 20 kb sequences: distance > 32*R*63 = 8064 -> unbanded striped fallback kernel"""
    rng = np.random.default_rng(3)
    reads = [rng.integers(0, 4, size=20000, dtype=np.uint8), rng.integers(0, 4, size=19000, dtype=np.uint8)]
    rs = seqio.pack_reads(reads)
    eng = hip.Engine()
    rd = eng.upload(rs)
    pairs = np.array([_pair(0, 0, 20000, 1, 0, 19000, 1), _pair(0, 0, 20000, 1, 0, 19000, 0),
                      _pair(1, 0, 300, 0, 0, 20000, 1)], dtype=hip.ED_PAIR_DTYPE)
    got, _, _ = eng.edit_distance_batch(rd, pairs)
    assert got[0] > 8064
    _check(eng, rd, rs, pairs)


def test_edit_distance_rejects_bad_spans():
    rs = seqio.pack_reads([np.zeros(100, np.uint8)])
    eng = hip.Engine()
    rd = eng.upload(rs)
    with pytest.raises(ValueError):
        eng.edit_distance_batch(rd, np.array([_pair(0, 50, 60, 0, 0, 10, 1)], dtype=hip.ED_PAIR_DTYPE))
    with pytest.raises(ValueError):
        eng.edit_distance_batch(rd, np.array([_pair(1, 0, 10, 0, 0, 10, 1)], dtype=hip.ED_PAIR_DTYPE))


# ---- batches of more than 2048 pairs: the stages behind the sample ---------------------------------------------------

def _noisy_pairs(rng, lengths, err, reads, P):
    """Per length one pair of reads: a random span and a copy with `err` errors (half substitutions), alternating strands
    and begins."""
    for n in lengths:
        a = rng.integers(0, 4, size=int(n), dtype=np.uint8)
        b = synth.mutate(rng, a, err / 2, err / 4, err / 4) if err < 1 else rng.integers(0, 4, size=int(n), dtype=np.uint8)
        strand = len(P) & 1
        ab, bb = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        flank = lambda k: rng.integers(0, 4, size=k, dtype=np.uint8)
        reads.append(np.concatenate([flank(ab), a, flank(7)]))
        reads.append(np.concatenate([flank(bb), b if strand else (3 - b[::-1]), flank(5)]))
        P.append(_pair(len(reads) - 2, ab, len(a), len(reads) - 1, bb, len(b), strand))


def _launches(eng):
    return {k: v[1] for k, v in eng.kernel_ms().items() if k.startswith("edit_")}


def _engine():
    eng = hip.Engine()
    eng.set_kernel_timing(True)
    return eng


def test_hifi_mix_runs_every_stage_and_is_exact_in_any_order():
    """~3 % error: the sample's 90th percentile of distance / length lands near bin 30 .. 45, which puts the bound of the
    3-slot class between 2.3 and 3.4 kb and of the 5-slot class between 5.0 and 7.2 kb; the lengths keep clear of both."""
    rng = np.random.default_rng(41)
    reads, P = [], []
    _noisy_pairs(rng, rng.integers(400, 600, size=2100), 0.03, reads, P)      # the sample (the 2048 shortest texts)
    _noisy_pairs(rng, rng.integers(800, 2200, size=700), 0.03, reads, P)      # 3 slots
    _noisy_pairs(rng, rng.integers(3600, 4800, size=30), 0.03, reads, P)      # 5 slots
    _noisy_pairs(rng, rng.integers(7500, 9000, size=24), 0.03, reads, P)      # 7 slots
    _noisy_pairs(rng, rng.integers(1500, 2100, size=24), 0.10, reads, P)      # lost by 3 slots, won by the second chance
    _noisy_pairs(rng, rng.integers(2400, 2800, size=12), 0.20, reads, P)      # beyond every lane window: wave kernel
    _noisy_pairs(rng, [16500, 17000], 1.0, reads, P)                          # unrelated, > 8064 edits: unbanded stripes
    for W in (3, 5, 7):                                                       # d just beyond 64 (W - 1)
        a = rng.integers(0, 4, size=1500, dtype=np.uint8)
        reads += [a, a[:1500 - 64 * (W - 1) - 1].copy()]
        P.append(_pair(len(reads) - 2, 0, 1500, len(reads) - 1, 0, len(reads[-1]), 1))
        P.append(_pair(len(reads) - 1, 0, len(reads[-1]), len(reads) - 2, 0, 1500, 1))
    P += [_pair(0, 3, 0, 1, 0, 500, 1), _pair(0, 0, 450, 1, 9, 0, 0), _pair(2, 0, 0, 3, 0, 0, 1)]  # empty spans
    rs = seqio.pack_reads(reads)
    pairs = np.array(P, dtype=hip.ED_PAIR_DTYPE)
    eng = _engine()
    rd = eng.upload(rs)
    eng.reset_stats()
    _check(eng, rd, rs, pairs)
    la = _launches(eng)
    # sample + three classes + second chance; the wave kernel; the stripes
    assert la["edit_lane"] >= 5 and la["edit_banded"] >= 1 and la["edit_full"] >= 1, la
    first, _, _ = eng.edit_distance_batch(rd, pairs)
    order = np.random.default_rng(42).permutation(pairs.shape[0])
    eng.reset_stats()
    again, _, _ = eng.edit_distance_batch(rd, pairs[order])
    assert np.array_equal(again, first[order])  # (the order goes through a radix sort and atomically collected lists)
    la = _launches(eng)
    assert la["edit_lane"] >= 5 and la["edit_banded"] >= 1 and la["edit_full"] >= 1, la


def test_batch_the_sample_turns_down_goes_to_the_wave_kernel():
    """The 2048 shortest pairs are unrelated spans of ~900 bases, ~470 edits apart: beyond the widest lane window (385), so
    fewer than half of the sample is decided and the main part (HiFi-like pairs the lane kernel could do) skips it."""
    rng = np.random.default_rng(43)
    reads, P = [], []
    _noisy_pairs(rng, rng.integers(880, 920, size=2060), 1.0, reads, P)
    _noisy_pairs(rng, rng.integers(1500, 2500, size=300), 0.01, reads, P)
    rs = seqio.pack_reads(reads)
    pairs = np.array(P, dtype=hip.ED_PAIR_DTYPE)
    eng = _engine()
    rd = eng.upload(rs)
    eng.reset_stats()
    _check(eng, rd, rs, pairs)
    la = _launches(eng)
    assert la["edit_lane"] == 1 and la["edit_banded"] >= 1, la


def test_n_main_zero_one_two():
    rng = np.random.default_rng(44)
    reads, P = [], []
    _noisy_pairs(rng, rng.integers(300, 700, size=2050), 0.02, reads, P)
    rs = seqio.pack_reads(reads)
    pairs = np.array(P, dtype=hip.ED_PAIR_DTYPE)
    eng = _engine()
    rd = eng.upload(rs)
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        want = np.array(list(ex.map(lambda p: _want(rs, p), pairs)), dtype=np.uint32)
    for n in (2048, 2049, 2050):
        eng.reset_stats()
        got, _, _ = eng.edit_distance_batch(rd, pairs[:n])
        assert np.array_equal(got, want[:n]), (n, np.nonzero(got != want[:n])[0][:10])
        assert _launches(eng)["edit_lane"] == (1 if n == 2048 else 2), (n, _launches(eng))


def test_bounded_mode_on_the_hifi_shape():
    """kmax (the identity filter's bounded mode) on > 2048 overlaps of reads cut from one genome with 1 - 3 % noise,
    against oracle.identity_filter, for identities that cut through the data's distribution, with planted overlaps whose
    distance is exactly the largest that passes (t) and t + 1."""
    rng = np.random.default_rng(45)
    genome = synth.make_genome(300_000, seed=46)
    reads, O = [], []

    def overlap(a, b, strand):
        ab, bb = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        flank = lambda k: rng.integers(0, 4, size=k, dtype=np.uint8)
        reads.append(np.concatenate([flank(ab), a, flank(16)]))
        reads.append(np.concatenate([flank(bb), b if strand else (3 - b[::-1]), flank(16)]))
        O.append((len(reads) - 2, ab, ab + len(a), len(reads) - 1, bb, bb + len(b), 0, strand))

    lengths = np.concatenate([rng.integers(400, 600, size=2100), rng.integers(800, 2200, size=250),
                              rng.integers(3600, 4800, size=16), rng.integers(7500, 9000, size=8)])
    for n in lengths:
        at = int(rng.integers(0, genome.shape[0] - n))
        e1, e2 = rng.uniform(0.005, 0.015, size=2)
        overlap(synth.mutate(rng, genome[at:at + n], e1 / 2, e1 / 4, e1 / 4), synth.mutate(rng, genome[at:at + n], e2 / 2, e2 / 4, e2 / 4),
                len(O) & 1)
    base_rs = seqio.pack_reads(reads)
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        dist = np.array(list(ex.map(lambda o: _want(base_rs, dict(lhs_read=o[0], lhs_begin=o[1], lhs_len=o[2] - o[1], rhs_read=o[3],
                                                                  rhs_begin=o[4], rhs_len=o[5] - o[4], strand=o[7])), O)))
    score = 1. - dist / np.array([max(o[2] - o[1], o[5] - o[4]) for o in O], dtype=np.float64)
    identities = [float(np.percentile(score, q)) for q in (30, 50, 70)]
    planted = {}
    for identity in identities:  # substitutions only, well apart: D = their number (checked below against the DP)
        for n in (500, 2000):
            t = 0
            while not (1. - float(t + 1) / float(n) < identity):
                t += 1
            for count in (t, t + 1):
                a = rng.integers(0, 4, size=n, dtype=np.uint8)
                b = a.copy()
                slots = rng.choice(n // 6, size=count, replace=False) * 6
                b[slots] = (b[slots] + 1) & 3
                overlap(a, b, count & 1)
                planted[len(O) - 1] = (identity, count, count == t)
    rs = seqio.pack_reads(reads)
    ovl = np.array(O, dtype=hip.OVERLAP_DTYPE)
    off = np.zeros(rs.n + 1, dtype=np.uint32)  # per-pile lists: pile 2 i holds overlap i
    off[1:] = np.minimum((np.arange(rs.n) + 2) // 2, len(O))
    begin = np.zeros(rs.n, np.uint32)
    end = ((rs.lengths >> 4) << 4).astype(np.uint32)
    invalid = np.zeros(rs.n, np.uint8)
    eng = _engine()
    rd = eng.upload(rs)
    with ThreadPoolExecutor(3) as ex:
        wants = list(ex.map(lambda i: oracle.identity_filter(rs, ovl.astype(oracle.OVERLAP_DTYPE), off, begin, end, invalid, i), identities))
    for identity, (want_o, want_off) in zip(identities, wants):
        kept = set(want_o["lhs_id"].tolist())
        assert 0.1 * len(O) <= len(kept) <= 0.9 * len(O), (identity, len(kept))  # from the oracle alone
        for i, (ident, count, keep) in planted.items():
            if ident == identity:
                assert (O[i][0] in kept) == keep, (identity, count, keep)
        eng.reset_stats()
        got_o, got_off = eng.filter_overlaps_by_identity(rd, ovl, off, begin, end, invalid, identity)
        assert np.array_equal(got_off, want_off)
        assert got_o.tobytes() == want_o.astype(hip.OVERLAP_DTYPE).tobytes()
        assert _launches(eng)["edit_lane"] >= 2, _launches(eng)
