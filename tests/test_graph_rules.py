"""The per-edge rules of the assembly graph on the CPU: the restatement of ConstructAssemblyGraph's edge loop,
RemoveTransitiveEdges and the long-edge loop (tests/host/graph_reference.cpp) pinned by hand-derived expectations, and the
host build of raven_amd/csrc/graph_rules.h (tests/host/graph_rules_host.cpp) equal to it on seeded random inputs."""
import numpy as np
import pytest

from tests import graph_util as gu


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("graph_rules")
    return gu.build_reference(d), gu.build_rules_program(d), d


def _triangle(len_j, len_k, len_c):
    """a -> b -> c and a -> c: edge 0 a -> b, 2 b -> c, 4 a -> c (odd ids: their pairs, lengths that never compare)"""
    t = gu.EdgeTable()
    a, b, c = t.nodes(3)
    t.join(a, b, len_j, 1)
    t.join(b, c, len_k, 1)
    t.join(a, c, len_c, 1000)
    return t


# (m, two-step sum, is a -> c marked), a -> c of length 25 m.  By hand: a sum s is comparable when 22 m <= s <= 28 m (s in
# the band of 25 m; both bounds are integers) or 25 m lies in the band of s, that is 25 m / 1.12 <= s <= 25 m / 0.88 =
# 28.409.. m.  So 22 m - 1 never is, 22 m and 28 m are, and 28 m + 1 is exactly when 0.409.. m >= 1, from m = 3 on
# (m = 2: 57 * 0.88 = 50.16 > 50; m = 3: 85 * 0.88 = 74.8 <= 75).
HAND = [(m, s, want) for m, last in ((1, 0), (2, 0), (3, 1), (100, 1), (40000, 1), (150_000_000, 1))
        for s, want in ((22 * m - 1, 0), (22 * m, 1), (28 * m, 1), (28 * m + 1, last))]
# the symmetric branch alone: 25 m = 2500, s above 28 m = 2800: 2840 * 0.88 = 2499.2 <= 2500, 2841 * 0.88 = 2500.08 > 2500;
# and with the roles swapped (s = 2500 against a direct edge of 2840 / 2841)
SYMMETRIC = [((1000, 1840, 2500), 1), ((1000, 1841, 2500), 0), ((1500, 1000, 2840), 1), ((1500, 1000, 2841), 0)]


def test_hand_computed_triangles(programs):
    ref, host, d = programs
    triples = [(s // 2, s - s // 2, 25 * m) for m, s, _ in HAND] + [t for t, _ in SYMMETRIC]
    want = np.array([w for _, _, w in HAND] + [w for _, w in SYMMETRIC], np.uint8)
    assert np.array_equal(gu.comparable(ref, triples, d, "hand_ref"), want)
    assert np.array_equal(gu.comparable(host, triples, d, "hand_host"), want)
    # the marks themselves, in insertion order, with the pair list: a -> c (4), its pair (5), whose ends are c' and a'
    for (lj, lk, lc), w in zip(triples, want):
        got = gu.reference_marks(ref, _triangle(lj, lk, lc), d, "tri")
        assert got["order"].tolist() == ([4, 5] if w else [])
        assert got["pairs"].tolist() == ([[4, 0]] if w else [])


def test_hand_computed_wrapping_sum(programs):
    """jt->length + kt->length wraps in 32 bits before the comparison: 2^31 + (2^31 + 2500) is 2500"""
    ref, host, d = programs
    triples = [(1 << 31, (1 << 31) + 2500, 2500), (1 << 31, (1 << 31) + 2500, 2900), (0xFFFFFFFF, 2501, 2500),
               ((1 << 31) - 1, 1 << 31, 0xFFFFFFFF)]
    want = np.array([1, 0, 1, 1], np.uint8)
    assert np.array_equal(gu.comparable(ref, triples, d, "wrap_ref"), want)
    assert np.array_equal(gu.comparable(host, triples, d, "wrap_host"), want)


def test_hand_computed_insertion_order_and_parallel_edges(programs):
    ref, _, d = programs
    # parallel edges a -> c: candidate[c] ends up with the later one (id 6); only its length decides
    for first, second, want in ((2500, 9000, []), (9000, 2500, [6, 7])):
        t = gu.EdgeTable()
        a, b, c = t.nodes(3)
        t.join(a, b, 1000, 1)
        t.join(b, c, 1500, 1)
        t.join(a, c, first, 50000)
        t.join(a, c, second, 50000)
        assert gu.reference_marks(ref, t, d, "par")["order"].tolist() == want
    # an edge first inserted as the PAIR of a mark made from an earlier node: nodes a, b, c = 0, 2, 4.  From a (node 0) the
    # triangle marks a -> c (4) and then its pair c' -> a' (5).  The pair triangle c' -> b' -> a' (lengths 1000 + 1500
    # against 2500) marks edge 5 again from node 5: no new insertion.  The sequence stays 4, 5.
    t = gu.EdgeTable()
    a, b, c = t.nodes(3)
    t.join(a, b, 1000, 1500)
    t.join(b, c, 1500, 1000)
    t.join(a, c, 2500, 2500)
    got = gu.reference_marks(ref, t, d, "ord")
    assert got["order"].tolist() == [4, 5] and got["pairs"].tolist() == [[4, 0]]
    # the other way round: only the pair triangle compares (from node c' = 5, after node 0 found nothing): 5 first, then 4
    t = gu.EdgeTable()
    a, b, c = t.nodes(3)
    t.join(a, b, 1000, 1500)
    t.join(b, c, 1500, 1000)
    t.join(a, c, 9000, 2500)
    got = gu.reference_marks(ref, t, d, "ord2")
    assert got["order"].tolist() == [5, 4] and got["pairs"].tolist() == [[4, 0]]


def test_hand_computed_long_edges(programs):
    ref, host, d = programs
    t = gu.EdgeTable()
    v, x, y, z, u, q = t.nodes(6)
    for h in (x, y, z):
        t.join(v, h, 100)  # edges 0, 2, 4 leave v; their pairs 1, 3, 5 leave x', y', z' (out-degree 1 each)
    t.join(u, q, 100)  # out-degree 1: never marked, whatever it weighs
    # weight(kt) > 2 * weight(jt) for another jt: 2.0 against 1.0 is a tie (not marked), 2.5 is marked with its pair
    w = [1.0, 1.0, 2.0, 2.0, 2.5, 2.5, 99.0, 99.0]
    got = gu.reference_marks(ref, t, d, "long", weight=w)
    assert got["long"].tolist() == [0, 0, 0, 0, 1, 1, 0, 0] and got["n_long"] == 2
    # equal minima: each is the other's "other"; zero and negative weights: -3 * 2 < -5, so -5 is long beside -3, and
    # beside a lone minimum of -3 every other edge is compared with -3, the minimum itself with the second smallest
    got = gu.reference_marks(ref, t, d, "long2", weight=[1.0, 1.0, 1.0, 1.0, 2.5, 2.5, 0.0, 0.0])
    assert got["long"].tolist() == [0, 0, 0, 0, 1, 1, 0, 0]
    got = gu.reference_marks(ref, t, d, "long3", weight=[-3.0, -3.0, -5.0, -5.0, 0.0, 0.0, 0.0, 0.0])
    # -5: others are -3 (-6 < -5: marked) ; -3: others -5, 0 (-10 < -3: marked); 0: -10 < 0: marked
    assert got["long"].tolist() == [1, 1, 1, 1, 1, 1, 0, 0] and got["n_long"] == 6
    pairs = [(1.0, 2.0), (1.0, 2.5), (-3.0, -5.0), (-5.0, -3.0), (0.0, 0.0), (0.0, 1e-300), (-0.0, 0.0)]
    assert gu.long_rule(host, pairs, d).tolist() == [0, 1, 1, 1, 0, 1, 0]


def test_host_rules_match_the_restatement_on_random_triples(programs):
    ref, host, d = programs
    rng = np.random.default_rng(20240)
    n = 20_000
    lc = rng.integers(100, 1 << 20, size=n).astype(np.int64)
    s = (lc * rng.uniform(0.7, 1.4, size=n)).astype(np.int64)
    edge = rng.random(n) < 0.25  # a quarter within +-2 of a band edge (either branch's)
    factor = rng.choice([0.88, 1.12, 1 / 0.88, 1 / 1.12], size=n)
    s[edge] = (lc[edge] * factor[edge]).astype(np.int64) + rng.integers(-2, 3, size=int(edge.sum()))
    big = rng.random(n) < 0.15  # lengths above 2^31 whose sum wraps to s
    lj = rng.integers(0, np.maximum(s, 1))
    lk = s - lj
    lj[big] += 1 << 31
    lk[big] += 1 << 31
    huge = rng.random(n) < 0.05  # and candidates beside 2^32
    lc[huge] = (1 << 32) - 1 - rng.integers(0, 1000, size=int(huge.sum()))
    triples = np.stack([lj, lk, lc], axis=1).astype(np.uint64).astype(np.uint32)
    a = gu.comparable(ref, triples, d, "rnd_ref")
    b = gu.comparable(host, triples, d, "rnd_host")
    assert np.array_equal(a, b)
    assert 0.2 * n < a.sum() < 0.9 * n and a[edge].min() == 0 and a[edge].max() == 1 and a[big].max() == 1


def test_edge_records_match_the_restatement(programs):
    ref, host, d = programs
    inp = gu.random_overlaps(np.random.default_rng(77), 500, 20_000)
    want, _ = gu.run_construct(ref, inp, d, "rec_ref")
    got, _ = gu.run_construct(host, inp, d, "rec_host", marks=False)
    gu.assert_same_tables(got, want)
    fin = want["finalized"]
    assert want["n_edges"] > 4000 and (fin["score"] == 4).sum() > 500 and (fin["score"] == 3).sum() > 500
    assert (fin["strand"] == 0).sum() > 500 and (fin["strand"] == 1).sum() > 500
    assert (want["sequence_to_node"] < 0).sum() > 20 and want["n_edges"] < 2 * inp.overlaps.shape[0]
    # a type-4 overlap by hand: lhs 0 = [0, 5000), rhs 1 = [0, 6000), same strand, lhs [0, 2000) on rhs [4000, 6000): the
    # rhs continues into the lhs.  tail = node(rhs) = 2, head = node(lhs) = 0, length = -(0 - 4000) = 4000, the pair's
    # -((6000 - 6000) - (5000 - 2000)) = 3000, from 0 ^ 1 to 2 ^ 1
    one = gu.ConstructInput(np.array([(0, 0, 2000, 1, 4000, 6000, 0, 1)], dtype=gu.hip.OVERLAP_DTYPE), [0, 0], [5000, 6000],
                            [10, 20], [0, 0])
    for exe, marks in ((ref, True), (host, False)):
        r, _ = gu.run_construct(exe, one, d, "one", marks=marks)
        assert r["tail"].tolist() == [2, 1] and r["head"].tolist() == [0, 3] and r["length"].tolist() == [4000, 3000]
        assert r["finalized"]["score"].tolist() == [4] and r["node_coverage"].tolist() == [10, 10, 20, 20]
    # an edge on an invalid pile: both programs refuse it
    bad = gu.ConstructInput(one.overlaps, one.begin, one.end, one.median, [0, 1])
    for exe in (ref, host):
        assert gu.run_construct(exe, bad, d, "bad", ok=(3,))[0] is None


def test_chain_conditions_hold_on_a_synthetic_list(programs):
    """What the GPU chain test asserts of its input (edges, marks, a type-4 overlap) the restatement alone meets on a
    tiled synthetic list: reads every 1 kb of a line, each overlapping the next five, half of them listed from the far
    read's side (type 4)."""
    ref, _, d = programs
    inp = gu.tiled_overlaps(200)
    want, _ = gu.run_construct(ref, inp, d, "tiled")
    assert want["n_edges"] > 0 and want["order"].shape[0] > 0 and (want["finalized"]["score"] == 4).sum() > 0
