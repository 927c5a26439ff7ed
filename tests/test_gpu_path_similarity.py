"""rvn_path_similarity_batch against the restatement (tests/host/bubble_reference.cpp: its edit distance, and the two rules
of RemoveBubbles' similarity test applied to it as assemble.cc:267-281 states them): verdict and reported distance equal
for pairs whose distance lies just under, on and just over the threshold, for the length rule on both sides of its
bound, for equal sequences and for sequences that differ everywhere; which edit-distance stage the pairs took; the
refusals."""
import numpy as np
import pytest

from raven_amd import hip
from tests import bubble_util as bu

pytestmark = pytest.mark.gpu

RATIOS = (0.8, 0.7, 0.93)
LENGTHS = (100, 1000, 20_000)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("path_similarity")
    return bu.build_reference(d), d


@pytest.fixture(scope="module")
def engine():
    e = hip.Engine(15, 5)
    e.set_kernel_timing(True)
    return e


def _want(d, l, r, ratio):
    """(similar, reported distance) by the reference's two rules on the restatement's distance d."""
    mx, mn = max(l, r), min(l, r)
    if mn < mx * ratio:
        return 0, bu.BY_LENGTH
    if 1 - d / float(mx) < ratio:
        return 0, bu.ABOVE
    return 1, d


def _check(engine, ref, seqs, pairs, ratio, tag):
    exe, d = ref
    dist = bu.distances(exe, [(seqs[a], seqs[b]) for a, b in pairs], d, tag)
    want = [_want(int(x), seqs[a].shape[0], seqs[b].shape[0], ratio) for x, (a, b) in zip(dist, pairs)]
    rd = engine.upload_codes(seqs)
    engine.reset_stats()
    similar, distance = engine.path_similarity(rd, pairs, ratio)
    assert similar.tolist() == [w[0] for w in want] and distance.tolist() == [w[1] for w in want]
    launches = {k: v[1] for k, v in engine.kernel_ms().items() if k.startswith("edit_")}
    return dist, want, launches


@pytest.fixture(scope="module")
def planted(ref):
    """Per (length, ratio) a sequence and three copies with substitutions planted so that the restatement's distance is
    kmax - 1, kmax and kmax + 1: the plant is an upper bound, so substitutions are added until the distance is there."""
    exe, d = ref
    rng = np.random.default_rng(11)
    cases = []
    for n in LENGTHS:
        a = rng.integers(0, 4, size=n).astype(np.uint8)
        order = rng.permutation(n)
        change = rng.integers(1, 4, size=n).astype(np.uint8)
        for ratio in RATIOS:
            k = bu.kmax(n, ratio)
            for target in (k - 1, k, k + 1):
                cases.append(dict(a=a, order=order, change=change, ratio=ratio, kmax=k, target=target, planted=target))
    for round_ in range(40):
        todo = [c for c in cases if c.get("distance") != c["target"]]
        if not todo:
            break
        for c in todo:
            b = c["a"].copy()
            at = c["order"][:c["planted"]]
            b[at] = (b[at] + c["change"][at]) & 3
            c["b"] = b
        for c, x in zip(todo, bu.distances(exe, [(c["a"], c["b"]) for c in todo], d, "plant%d" % round_)):
            c["distance"] = int(x)
            if c["distance"] != c["target"]:
                c["planted"] = min(c["a"].shape[0], max(0, c["planted"] + c["target"] - c["distance"]))
    return cases


@pytest.mark.parametrize("ratio", RATIOS)
def test_distances_just_under_on_and_over_the_threshold(engine, ref, planted, ratio):
    cases = [c for c in planted if c["ratio"] == ratio]
    seqs, pairs = [], []
    for c in cases:
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [c["a"], c["b"]]
    pairs += [(b, a) for a, b in pairs]
    dist, want, launches = _check(engine, ref, seqs, pairs, ratio, "t%g" % ratio)
    # every plant reached its aim: on each side of every threshold there is a pair, and both verdicts are asserted
    assert all(c["distance"] == c["target"] for c in cases)
    for c, w in zip(cases, want):
        assert w == ((1, c["distance"]) if c["distance"] <= c["kmax"] else (0, bu.ABOVE))
    assert [w[0] for w in want[:len(cases)]] == [1, 1, 0] * len(LENGTHS)
    # every threshold lies inside the wave ring (the largest: 6 000 for 20 000 bases at 0.7): the usual route, one sweep
    assert (launches["edit_wide"], launches["edit_full"]) == (0, 0)


def test_the_length_rule_on_both_sides_of_its_bound(engine, ref):
    """min = ceil(mx x 0.8) - 1 and ceil(mx x 0.8) (the product in double, as the reference forms it: for mx = 5, 10, 15,
    1235 it is not the exact 0.8 mx); the shorter sequence is a prefix of the longer, so what passes the length rule has a
    distance of mx - min."""
    rng = np.random.default_rng(12)
    seqs, pairs, sides = [], [], []
    for mx in (5, 10, 15, 64, 100, 101, 1000, 1235, 4095, 12_345):
        a = rng.integers(0, 4, size=mx).astype(np.uint8)
        bound = int(np.ceil(mx * 0.8))
        for mn in (bound - 1, bound):
            pairs.append((len(seqs), len(seqs) + 1) if mn & 1 else (len(seqs) + 1, len(seqs)))
            seqs += [a, a[:mn].copy()]
            sides.append(mn < mx * 0.8)
    dist, want, _ = _check(engine, ref, seqs, pairs, 0.8, "len")
    assert [w[1] == bu.BY_LENGTH for w in want] == sides and sum(sides) == len(sides) // 2
    assert all(w[0] == 1 for w, s in zip(want, sides) if not s)  # (mx - min <= 0.2 mx: the score passes)


def test_equal_sequences_and_sequences_that_differ_everywhere(engine, ref):
    rng = np.random.default_rng(13)
    seqs, pairs = [], []
    for n in (1, 2, 31, 32, 33, 64, 100, 1000, 5000):
        a = rng.integers(0, 4, size=n).astype(np.uint8)
        seqs += [a, a.copy(), np.zeros(n, np.uint8), np.ones(n, np.uint8)]
        k = len(seqs) - 4
        pairs += [(k, k + 1), (k, k), (k + 2, k + 3), (k + 3, k + 2)]
    for ratio in (0.8, 1.0, 0.0):
        dist, want, _ = _check(engine, ref, seqs, pairs, ratio, "eq%g" % ratio)
        assert [w[0] for w in want] == [1, 1, int(ratio == 0.0), int(ratio == 0.0)] * 9


@pytest.fixture(scope="module")
def long_pairs():
    """The smallest pairs beyond the wave ring (8 064): 41 000 bases at the 0.8 rule, kmax = 8 200.  Distances of about
    2 000, between 8 064 and kmax, and above kmax.  For the 0.85 rule pairs of unequal lengths: 60 000
    bases (kmax = 9 000) against 52 000 of them, 8 000 deleted in one piece, with 500 and with 1 200 substitutions."""
    rng = np.random.default_rng(14)
    a = rng.integers(0, 4, size=41_000).astype(np.uint8)
    b = rng.integers(0, 4, size=60_000).astype(np.uint8)
    short = np.concatenate([b[:25_000], b[33_000:]])
    return [a, bu.plant(rng, a, 2_000), bu.plant(rng, a, 8_150), bu.plant(rng, a, 9_000), b, bu.plant(rng, short, 500),
            bu.plant(rng, short, 1_200)]


@pytest.mark.parametrize("lanes", [0, 128, 64, 1])
def test_thresholds_beyond_the_wave_ring(engine, ref, long_pairs, lanes):
    """Pairs whose kmax lies beyond the wave ring go straight to the workgroup ring: no lane window, no wave ring (their
    launch counts stay 0), so the pair 2 000 edits apart is the ring's as well, in the one sweep it makes.  The ring's size
    (engine option ed_wide_lanes) decides what is left for the full sweep: the default 512 lanes and 128 lanes (every lane
    then takes a second super-block: 41 000 bases are 161 of them) hold kmax = 8 200; a ring of 64 lanes ends at 8 064,
    decides the first pair and hands the others on; 1 switches the ring off (lane window, wave ring, full sweep).  The
    full sweep's exact answer above kmax is reported as above.  Same verdicts and distances every way."""
    pairs = [(0, 1), (0, 2), (3, 0), (2, 0)]
    engine.set_option("ed_wide_lanes", lanes)
    try:
        dist, want, launches = _check(engine, ref, long_pairs, pairs, 0.8, "ring%d" % lanes)
        assert dist[0] <= 2_000 and 8_064 < dist[1] <= 8_200 < dist[2] and dist[3] == dist[1]
        assert want == [(1, int(dist[0])), (1, int(dist[1])), (0, bu.ABOVE), (1, int(dist[1]))]
        route = (launches["edit_lane"], launches["edit_banded"], launches["edit_wide"], launches["edit_full"])
        assert route == {0: (0, 0, 1, 0), 128: (0, 0, 1, 0), 64: (0, 0, 1, 1), 1: (1, 1, 0, 1)}[lanes]
        if lanes == 0:  # unequal lengths at 0.85, one pair under kmax = 9 000 and one over, both beyond the wave ring
            dist, want, launches = _check(engine, ref, long_pairs, [(4, 5), (6, 4)], 0.85, "ring85")
            assert 8_064 < dist[0] <= 9_000 < dist[1] and want == [(1, int(dist[0])), (0, bu.ABOVE)]
            assert (launches["edit_lane"], launches["edit_banded"], launches["edit_wide"], launches["edit_full"]) == (0, 0, 1, 0)
    finally:
        engine.set_option("ed_wide_lanes", -1)


def test_thresholds_inside_and_beyond_the_wave_ring_in_one_call(engine, ref, long_pairs):
    """One call whose pairs alternate between the two batches of path_similarity_batch — thresholds the wave ring holds
    (short sequences, and one rejected by length) and thresholds beyond it (41 000 bases) — in an order that is neither
    batch's: every answer lands at its own pair, and the second batch's scratch does not disturb the first's results."""
    rng = np.random.default_rng(15)
    short = rng.integers(0, 4, size=3_000).astype(np.uint8)
    seqs = list(long_pairs[:4]) + [short, bu.plant(rng, short, 100), bu.plant(rng, short, 700), short[:2_000].copy()]
    pairs = [(4, 5), (0, 2), (6, 4), (3, 0), (4, 7), (1, 0), (5, 4), (0, 1), (4, 4), (2, 0)]
    dist, want, launches = _check(engine, ref, seqs, pairs, 0.8, "mixed")
    assert [w[0] for w in want] == [1, 1, 0, 0, 0, 1, 1, 1, 1, 1] and want[4][1] == bu.BY_LENGTH and want[8] == (1, 0)
    assert launches["edit_wide"] == 1 and launches["edit_full"] == 0 and launches["edit_banded"] + launches["edit_lane"] >= 1


def test_refusals_and_empty_batches(engine):
    rd = engine.upload_codes([np.zeros(10, np.uint8), np.zeros(0, np.uint8), np.ones(9, np.uint8)])
    s, dist = engine.path_similarity(rd, np.zeros((0, 2), np.uint32))
    assert s.shape == (0,) and dist.shape == (0,)
    with pytest.raises(ValueError, match="pair 1 names an unknown path"):
        engine.path_similarity(rd, [(0, 2), (0, 3)])
    with pytest.raises(ValueError, match="path 1 .*has no bases"):
        engine.path_similarity(rd, [(0, 2), (1, 0)])
    with pytest.raises(ValueError, match="not a number"):
        engine.path_similarity(rd, [(0, 2)], float("nan"))
    for lanes in (2, 63, 100, 576, 1024):
        with pytest.raises(ValueError, match="ed_wide_lanes is 64 .. 512 in steps of 64"):
            engine.set_option("ed_wide_lanes", lanes)
    assert engine.set_option("ed_wide_lanes", 256) == 0 and engine.set_option("ed_wide_lanes", -1) == 256
    s, dist = engine.path_similarity(rd, [(0, 2), (2, 0), (0, 0)])
    assert s.tolist() == [0, 0, 1] and dist.tolist() == [bu.ABOVE, bu.ABOVE, 0]
