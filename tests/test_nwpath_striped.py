"""The striped sweep of the alignment-path stage (nwpath.h, NwGeo: a band wider than one wave's ring, swept in stripes of
super-blocks whose top input is the hs stream of the stripe above) stepped on the CPU with forced stripe sizes: distance
and window records equal the oracle's plain-DP path and an independent Python traceback, and a band wider than the
stripes may hold is refused, not truncated.  No GPU needed (rvn_test_nw_breakpoints, bits 16-23 of its rc flags)."""
import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip, synth
from tests.test_nwpath import _oriented, _pack, _reference_records


def _noisy_pair(rng, n, sub, ins, dele):
    t = rng.integers(0, 4, size=n, dtype=np.uint8)
    return t, synth.mutate(rng, t, sub, ins, dele)


def _striped(target, read, t_begin, n, q_begin, m, rc, w, stripe_lanes, k=32, force_r=1, group_lanes=0):
    recs, dist, band, status = hip.test_nw_breakpoints(_pack(target), len(target), _pack(read), len(read), t_begin, n,
                                                       q_begin, m, rc, w, k=k, force_r=force_r, group_lanes=group_lanes,
                                                       stripe_lanes=stripe_lanes)
    assert status == 0
    return recs, dist, band


def _check(target, read, t_begin, n, q_begin, m, rc, w, stripe_lanes, k=32, force_r=1, group_lanes=0):
    """Records and distance of the striped sweep against the oracle; returns (distance, band)."""
    recs, dist, band = _striped(target, read, t_begin, n, q_begin, m, rc, w, stripe_lanes, k, force_r, group_lanes)
    rq = _oriented(np.asarray(read, dtype=np.uint8), rc)
    want, want_dist = oracle.nw_breakpoints(rq[q_begin:q_begin + m], np.asarray(target[t_begin:t_begin + n], np.uint8),
                                            q_begin, t_begin, w)
    assert dist == want_dist
    got = []
    for x, r in enumerate(recs):
        if r["first_t"] == 0xFFFFFFFF:
            continue
        assert r["first_t"] // w == t_begin // w + x
        got.append((int(r["first_t"]), int(r["first_q"])))
        got.append((int(r["last_t"]), int(r["last_q"])))
    assert got == [tuple(int(v) for v in p) for p in want]
    # and the same bytes as the one-ring sweep
    recs1, dist1, _, status1 = hip.test_nw_breakpoints(_pack(target), len(target), _pack(read), len(read), t_begin, n,
                                                       q_begin, m, rc, w, k=k)
    assert status1 == 0 and dist1 == dist and recs1.tobytes() == recs.tobytes()
    return dist, band


@pytest.mark.parametrize("rc", [0, 1])
def test_striped_ont_like_pairs(rc):
    rng = np.random.default_rng(300 + rc)
    for trial, (n, stripes) in enumerate([(500, 2), (1800, 3), (4200, 4), (9000, 8), (20_000, 16)]):
        t, q = _noisy_pair(rng, n, 0.04, 0.03, 0.03)
        tl, ql = int(rng.integers(0, 600)), int(rng.integers(0, 90))
        target = np.concatenate([rng.integers(0, 4, tl, dtype=np.uint8), t, rng.integers(0, 4, 77, dtype=np.uint8)])
        read_o = np.concatenate([rng.integers(0, 4, ql, dtype=np.uint8), q, rng.integers(0, 4, 33, dtype=np.uint8)])
        read = _oriented(read_o, rc)
        force_r = 1 if n < 5000 else 2
        nsup = -(-(-(-n // 64)) // force_r)
        lanes = max(2, -(-nsup // stripes))  # about `stripes` stripes
        dist, band = _check(target, read, tl, len(t), ql, len(q), rc, 500, lanes, force_r=force_r)
        assert band[2] == force_r and band[4] > 1 and band[0] >= dist > 0.05 * n


def test_striped_bursts_lengths_and_degenerate_spans():
    rng = np.random.default_rng(33)
    t = rng.integers(0, 4, 2500, dtype=np.uint8)
    q = np.concatenate([t[:800], rng.integers(0, 4, 300, dtype=np.uint8), t[800:1700], t[1950:]])  # +300 / -250
    for lanes in (2, 5, 16):
        assert _check(t, q, 0, len(t), 0, len(q), 0, 500, lanes)[1][4] > 1
        assert _check(q, t, 0, len(q), 0, len(t), 0, 500, lanes)[1][4] > 1
    # very different lengths: a one-sided band
    long_q = np.concatenate([t[:400], rng.integers(0, 4, 900, dtype=np.uint8)])
    _check(t[:400], long_q, 0, 400, 0, 1300, 0, 100, 2)
    _, band = _check(long_q, t[:400], 0, 1300, 0, 400, 0, 100, 2)
    assert band[4] > 1
    for n, m in [(1, 1), (1, 7), (9, 1), (64, 64), (65, 63), (129, 300), (300, 250)]:
        tt = rng.integers(0, 4, n, dtype=np.uint8)
        qq = rng.integers(0, 4, m, dtype=np.uint8)
        _check(tt, qq, 0, n, 0, m, 0, 50, 2, k=4)
    h = np.zeros(700, dtype=np.uint8)  # homopolymers: every path is optimal, the tie rule decides
    _check(h, h[:600], 0, 700, 0, 600, 0, 100, 3)
    _check(h[:600], h, 0, 600, 0, 700, 0, 100, 3)
    u, v = rng.integers(0, 4, 1500, dtype=np.uint8), rng.integers(0, 4, 1400, dtype=np.uint8)  # unrelated
    assert _check(u, v, 0, 1500, 0, 1400, 1, 64, 4)[1][4] > 1


@pytest.mark.parametrize("force_r", [1, 2, 4, 8])
def test_striped_every_blocks_per_lane_and_the_walks(force_r):
    """R = 1 .. 8 blocks per lane, and every walk (lane walk, half-size strips, group walks) over a striped band."""
    rng = np.random.default_rng(70 + force_r)
    t, q = _noisy_pair(rng, 6000, 0.04, 0.03, 0.03)
    for lanes in ((3, 4, 64) if force_r == 1 else (3, 4)):
        d, band = _check(t, q, 0, len(t), 0, len(q), 0, 500, lanes, k=8, force_r=force_r)
        assert band[2] == force_r and band[4] >= 2
        for gl in (1, 4, 16, 64):
            recs, dist, _ = _striped(t, q, 0, len(t), 0, len(q), 0, 500, lanes, 8, force_r, group_lanes=gl)
            recs0, _, _ = _striped(t, q, 0, len(t), 0, len(q), 0, 500, lanes, 8, force_r)
            assert dist == d and recs.tobytes() == recs0.tobytes()


@pytest.mark.parametrize("w", [7, 64, 500])
def test_striped_records_equal_an_independent_traceback(w):
    rng = np.random.default_rng(910 + w)
    for trial in range(4):
        n = int(rng.integers(200, 360))
        t, q = _noisy_pair(rng, n, 0.05, 0.04, 0.04)
        rc = trial & 1
        tl, ql = int(rng.integers(0, 3 * w + 5)), int(rng.integers(0, 40))
        target = np.concatenate([rng.integers(0, 4, tl, dtype=np.uint8), t, rng.integers(0, 4, 9, dtype=np.uint8)])
        read_o = np.concatenate([rng.integers(0, 4, ql, dtype=np.uint8), q, rng.integers(0, 4, 5, dtype=np.uint8)])
        read = _oriented(read_o, rc)
        recs, dist, band = _striped(target, read, tl, len(t), ql, len(q), rc, w, 2, k=16)
        assert band[4] >= 2
        want_dist, wins = _reference_records(q, t, ql, tl, w)
        assert dist == want_dist
        for x, r in enumerate(recs):
            ref = wins.get(tl // w + x)
            if ref is None or ref["first"] is None:
                assert r["first_t"] == 0xFFFFFFFF
                continue
            assert (int(r["first_t"]), int(r["first_q"])) == ref["first"]
            assert (int(r["last_t"]), int(r["last_q"])) == ref["last"]


def test_band_wider_than_the_stripes_is_refused():
    """At most 8 rings of the stripe size: a wider band is refused (status < 0), never truncated."""
    rng = np.random.default_rng(12)
    t, q = _noisy_pair(rng, 3000, 0.08, 0.06, 0.06)  # distance ~550: a band of ~10 lanes of 64 rows
    _check(t, q, 0, len(t), 0, len(q), 0, 500, 2, k=600)  # 16 lanes hold it
    with pytest.raises(ValueError):
        _striped(t, q, 0, len(t), 0, len(q), 0, 500, 1, k=600)  # 8 lanes do not
