"""The assembly graph on the device (raven_amd/csrc/graph.hip: rvn_construct_assembly_graph, rvn_graph_from_edges,
rvn_graph_mark_transitive, rvn_graph_mark_long_edges) equal to the single-threaded restatement of
ConstructAssemblyGraph's edge loop, RemoveTransitiveEdges and the long-edge loop (tests/host/graph_reference.cpp): every
fetched array, the marked ids in the order the reference's set first receives them and the transitive pair list as
sequences — on crafted and random edge tables, on hand-built overlap arrays, and on the device chain of a synthetic genome."""
import numpy as np
import pytest

from raven_amd import hip, synth
from tests import graph_util as gu
from tests import repeats_util as ru
from tests.test_graph_rules import HAND, SYMMETRIC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return gu.build_reference(tmp_path_factory.mktemp("graph_ref"))


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(15, 5)
    yield e
    e.close()


def _device_marks(eng, table):
    t, h, ln = table.arrays()
    g = eng.graph_from_edges(table.n_nodes, t, h, ln)
    assert g.n_nodes == table.n_nodes and g.n_edges == t.shape[0] and g.n_live_edges == int((t != gu.EMPTY).sum())
    f = g.fetch()
    assert np.array_equal(f["tail"], t) and np.array_equal(f["head"], h) and np.array_equal(f["length"], ln)
    order, pairs = g.mark_transitive()
    return g, order, pairs


def _check(eng, ref, table, tmp_path, tag):
    want = gu.reference_marks(ref, table, tmp_path, tag)
    g, order, pairs = _device_marks(eng, table)
    gu.assert_same_marks(order, pairs, want)
    g.close()
    return want


def test_boundary_triangles(eng, ref, tmp_path):
    """the triangles of tests/test_graph_rules.py, side by side in one table: triangle i marks 6 i + 4 and its pair or nothing"""
    triples = [(s // 2, s - s // 2, 25 * m) for m, s, _ in HAND] + [t for t, _ in SYMMETRIC] + \
              [(1 << 31, (1 << 31) + 2500, 2500), (1 << 31, (1 << 31) + 2500, 2900)]
    expect = [w for _, _, w in HAND] + [w for _, w in SYMMETRIC] + [1, 0]
    t = gu.EdgeTable()
    for lj, lk, lc in triples:
        a, b, c = t.nodes(3)
        t.join(a, b, lj, 1)
        t.join(b, c, lk, 1)
        t.join(a, c, lc, 1000)
    want = _check(eng, ref, t, tmp_path, "tri")
    assert want["order"].tolist() == [x for i, w in enumerate(expect) if w for x in (6 * i + 4, 6 * i + 5)]


def _crafted():
    """name -> table"""
    out = {}
    for name, first, second in (("parallel_earlier_comparable", 2500, 9000), ("parallel_later_comparable", 9000, 2500)):
        t = gu.EdgeTable()
        a, b, c = t.nodes(3)
        t.join(a, b, 1000, 1)
        t.join(b, c, 1500, 1)
        t.join(a, c, first, 50000)
        t.join(a, c, second, 50000)
        out[name] = t
    t = gu.EdgeTable()  # a self-loop on v: v -> v -> x against v -> x, v -> v -> v against v -> v, v -> x -> y against v -> y
    v, x, y = t.nodes(3)
    t.join(v, v, 10, 10)
    t.join(v, x, 100, 100)
    t.join(x, y, 100, 100)
    t.join(v, y, 205, 205)
    out["self_loop_on_v"] = t
    t = gu.EdgeTable()  # a self-loop on head(jt): v -> x -> x against v -> x
    v, x, y = t.nodes(3)
    t.join(v, x, 1000, 7)
    t.join(x, x, 100, 100)
    t.join(x, y, 500, 9)
    t.join(v, y, 1450, 11)
    out["self_loop_on_head"] = t
    for name, loop in (("back_to_v_without_loop", False), ("back_to_v_with_loop", True)):
        t = gu.EdgeTable()  # head(kt) == v
        v, x = t.nodes(2)
        t.join(v, x, 1000, 1000)
        t.join(x, v, 1000, 1000)
        if loop:
            t.join(v, v, 2100, 2100)
        out[name] = t
    t = gu.EdgeTable()  # empty slots between live ones, a head without out-edges, a node without any edge
    a, b, c, lone, sink = t.nodes(5)
    t.hole()
    t.join(a, b, 1000, 1500)
    t.hole()
    t.hole()
    t.join(b, c, 1500, 1000)
    t.join(a, sink, 77, 77)
    t.join(a, c, 2500, 2500)
    t.hole()
    out["holes_and_sinks"] = t
    t = gu.EdgeTable()  # first inserted as the pair of a mark made from an earlier node, then found again as itself
    a, b, c = t.nodes(3)
    t.join(a, b, 1000, 1500)
    t.join(b, c, 1500, 1000)
    t.join(a, c, 9000, 2500)  # only the pair triangle compares: 5 before 4
    a2, b2, c2 = t.nodes(3)
    t.join(a2, b2, 1000, 1500)
    t.join(b2, c2, 1500, 1000)
    t.join(a2, c2, 2500, 2500)
    out["pair_inserted_first"] = t
    t = gu.EdgeTable()  # one edge reached by several (jt, kt), some comparable, some not; the first in list order counts
    v, y = t.nodes(2)
    xs = t.nodes(6)
    for i, x in enumerate(xs):
        t.join(v, x, 1000 + i, 1)
    t.join(v, y, 3000, 3000)
    for i, x in enumerate(xs):
        t.join(x, y, (500, 2000, 1990, 9000, 2010, 1700)[i], 2)
    out["several_walks_to_one_edge"] = t
    out["nodes_without_edges"] = gu.EdgeTable(8)
    out["no_nodes"] = gu.EdgeTable(0)
    return out


@pytest.mark.parametrize("name", sorted(_crafted()))
def test_crafted_tables(eng, ref, tmp_path, name):
    want = _check(eng, ref, _crafted()[name], tmp_path, name)
    marked = {"parallel_earlier_comparable": 0, "parallel_later_comparable": 2, "nodes_without_edges": 0, "no_nodes": 0,
              "back_to_v_without_loop": 0}
    if name in marked:
        assert want["order"].shape[0] == marked[name]
    else:
        assert want["order"].shape[0] > 0
    if name == "pair_inserted_first":
        assert want["order"].tolist()[:2] == [5, 4]


@pytest.mark.parametrize("degree", [1, 63, 64, 65, 129, 5000])
def test_out_degrees_across_the_wave_and_tile_boundaries(eng, ref, tmp_path, degree):
    """one node of `degree` out-edges whose heads have 1 - 70 out-edges (1 - 5 for the small ones) back into the fan"""
    rng = np.random.default_rng(degree)
    t = gu.EdgeTable()
    t.nodes(3)  # nodes before the fan that have no edges
    gu.fan(t, rng, degree, 70 if degree == 5000 else 5)
    want = _check(eng, ref, t, tmp_path, "fan")
    live = len(t.tail)
    assert 0 < want["order"].shape[0] < live if degree > 1 else want["order"].shape[0] >= 0


@pytest.fixture(scope="module")
def random_tables():
    return {n: gu.random_table(np.random.default_rng(seed), n) for n, seed in ((3, 1), (50, 2), (2000, 3))}


@pytest.mark.parametrize("n", [3, 50, 2000])
def test_random_tables(eng, ref, tmp_path, random_tables, n):
    t = random_tables[n]
    triangles, comparable = gu.triangle_counts(t)
    assert 0.2 * triangles <= comparable <= 0.8 * triangles
    want = _check(eng, ref, t, tmp_path, "rnd")
    live = sum(1 for x in t.tail if x != gu.EMPTY)
    assert 0 < want["order"].shape[0] < live  # marks, and live edges that stay unmarked


def _long_check(eng, ref, table, weight, tmp_path, tag):
    want = gu.reference_marks(ref, table, tmp_path, tag, weight=weight)
    t, h, ln = table.arrays()
    g = eng.graph_from_edges(table.n_nodes, t, h, ln)
    flags, count = g.mark_long_edges(weight)
    g.close()
    assert np.array_equal(flags, want["long"]) and count == want["n_long"] == int(flags.sum())
    return want


def test_long_edges_on_crafted_weights(eng, ref, tmp_path):
    t = gu.EdgeTable()
    v, x, y, z, u, q = t.nodes(6)
    for h in (x, y, z):
        t.join(v, h, 100)
    t.join(u, q, 100)  # out-degree 1
    t.hole()
    cases = {
        "tie_at_twice_the_minimum": ([1.0, 1.0, 2.0, 2.0, 2.5, 2.5, 99.0, 99.0, 0, 0], [0, 0, 0, 0, 1, 1, 0, 0, 0, 0]),
        "equal_minima": ([1.0, 1.0, 1.0, 1.0, 2.5, 2.5, 0.0, 0.0, 0, 0], [0, 0, 0, 0, 1, 1, 0, 0, 0, 0]),
        "one_below": ([0.4, 0.4, 1.0, 1.0, 1.0, 1.0, 5.0, 5.0, 0, 0], [0, 0, 1, 1, 1, 1, 0, 0, 0, 0]),
        "negative_and_zero": ([-3.0, -3.0, -5.0, -5.0, 0.0, 0.0, 0.0, 0.0, 0, 0], [1, 1, 1, 1, 1, 1, 0, 0, 0, 0]),
        "zeros": ([0.0, 0.0, -0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0], [0] * 10),
        "out_degree_one_beside_a_heavy_pair": ([1.0, 9.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0, 0], [0] * 10),
    }
    for name, (w, expect) in cases.items():
        want = _long_check(eng, ref, t, w, tmp_path, name)
        assert want["long"].tolist() == expect, name
    # a node whose out-edges are pairs of other nodes' edges: the pair's weight is its own
    t2 = gu.EdgeTable()
    a, b, c = t2.nodes(3)
    t2.join(a, c, 100)       # 0: a -> c, 1: c' -> a'
    t2.join(b, c, 100)       # 2: b -> c, 3: c' -> b'
    want = _long_check(eng, ref, t2, [1.0, 1.0, 1.0, 3.0], tmp_path, "pairs")
    assert want["long"].tolist() == [0, 0, 1, 1]


@pytest.mark.parametrize("n", [3, 50, 2000])
def test_long_edges_on_random_weights(eng, ref, tmp_path, random_tables, n):
    t = random_tables[n]
    rng = np.random.default_rng(100 + n)
    w = rng.choice([0.0, 0.5, 1.0, 1.0, 2.0, 2.0, 3.0, -1.0], size=len(t.tail)) * rng.choice([1.0, 1.0, 1.0, 1.37], size=len(t.tail))
    w[1::2] = w[0::2]  # an edge and its pair weigh the same, as the layout leaves them
    want = _long_check(eng, ref, t, w, tmp_path, "rndw")
    assert 0 < want["n_long"] < len(t.tail)
    fan = gu.EdgeTable()
    gu.fan(fan, rng, 129, 3)
    wf = rng.uniform(0.5, 3.0, size=len(fan.tail))
    assert _long_check(eng, ref, fan, wf, tmp_path, "fanw")["n_long"] > 0


def _ovl(l, lb, le, r, rb, re, strand=1):
    return (l, lb, le, r, rb, re, 0, strand)


def _hand_built_construct():
    """piles 0 .. 9: 1, 4 and 8 invalid, 6 a valid region of length zero; overlaps of every type on both strands"""
    begin = np.array([0, 100, 200, 0, 50, 300, 700, 0, 0, 160], np.uint32)
    end = np.array([10000, 9000, 12200, 8000, 5000, 10300, 700, 9000, 7000, 10160], np.uint32)
    invalid = np.array([0, 1, 0, 0, 1, 0, 0, 0, 1, 0], np.uint8)
    median = np.array([11, 12, 13, 14, 15, 16, 17, 18, 19, 20], np.uint16)
    o = []
    for strand in (1, 0):
        o.append(_ovl(0, 4000, 6000, 2, 5200, 7200, strand))                      # 0 internal
        o.append(_ovl(3, 0, 8000, 2, 1200, 9200, strand))                         # 1 lhs contained
        o.append(_ovl(2, 1200, 9200, 3, 0, 8000, strand))                         # 2 rhs contained
        if strand:
            o.append(_ovl(0, 6000, 10000, 2, 200, 4200, strand))                  # 3 suffix of 0 on prefix of 2
            o.append(_ovl(5, 300, 4300, 9, 6160, 10160, strand))                  # 4 prefix of 5 on suffix of 9
        else:
            o.append(_ovl(0, 6000, 10000, 2, 8200, 12200, strand))                # 3 on the opposite strand
            o.append(_ovl(5, 300, 4300, 9, 160, 4160, strand))                    # 4 on the opposite strand
        o.append(_ovl(1, 4000, 6000, 7, 4000, 6000, strand))                      # internal on an invalid pile: dropped, no error
        o.append(_ovl(6, 700, 700, 7, 0, 100, strand))                            # a zero-length region
    return gu.ConstructInput(np.array(o, dtype=hip.OVERLAP_DTYPE), begin, end, median, invalid)


def test_construct_on_hand_built_arrays(eng, ref, tmp_path):
    inp = _hand_built_construct()
    want, _ = gu.run_construct(ref, inp, tmp_path, "hand")
    g = inp.device(eng)
    got = g.fetch()
    gu.assert_same_tables(got, want)
    assert g.n_nodes == want["n_nodes"] == 14 and g.n_edges == want["n_edges"]
    assert want["sequence_to_node"].tolist() == [0, -1, 2, 4, -1, 6, 8, 10, -1, 12]
    scores = want["finalized"]["score"].tolist()
    assert scores.count(3) >= 2 and scores.count(4) >= 2 and set(want["finalized"]["strand"].tolist()) == {0, 1}
    order, pairs = g.mark_transitive()
    gu.assert_same_marks(order, pairs, want)
    g.close()
    # random overlaps x pile states, and the tiled list with its transitive edges
    for tag, big in (("rand", gu.random_overlaps(np.random.default_rng(5), 300, 6000)), ("tiled", gu.tiled_overlaps(400))):
        want, _ = gu.run_construct(ref, big, tmp_path, tag)
        g = big.device(eng)
        gu.assert_same_tables(g.fetch(), want)
        order, pairs = g.mark_transitive()
        gu.assert_same_marks(order, pairs, want)
        g.close()
        assert want["n_edges"] > 1000 and (want["finalized"]["score"] == 4).sum() > 0
    assert want["order"].shape[0] > 0
    # empty inputs: no piles, no valid pile, no overlaps
    none = np.zeros(0, hip.OVERLAP_DTYPE)
    for inp in (gu.ConstructInput(none, [], [], [], []), gu.ConstructInput(none, [0, 0], [500, 900], [3, 4], [1, 1]),
                gu.ConstructInput(none, [0, 0], [500, 900], [3, 4], [0, 1])):
        want, _ = gu.run_construct(ref, inp, tmp_path, "empty")
        g = inp.device(eng)
        gu.assert_same_tables(g.fetch(), want)
        assert g.n_edges == 0 and g.n_nodes == want["n_nodes"] and g.mark_transitive()[0].shape[0] == 0
        g.close()


def test_invalid_arguments_leave_the_engine_usable(eng, ref, tmp_path):
    good = _hand_built_construct()

    def usable():
        g = good.device(eng)
        assert g.n_edges > 0
        g.close()

    def variant(**kw):
        d = dict(overlaps=good.overlaps.copy(), begin=good.begin.copy(), end=good.end.copy(), median=good.median, invalid=good.invalid.copy())
        d.update(kw)
        return gu.ConstructInput(d["overlaps"], d["begin"], d["end"], d["median"], d["invalid"])

    o = good.overlaps.copy()
    o[3]["rhs_id"] = 10
    end = good.end.copy()
    end[3] = 0
    begin = good.begin.copy()
    begin[3] = 5
    inv = good.invalid.copy()
    inv[2] = 1  # overlap 3 is of type 3 between piles 0 and 2
    o2 = good.overlaps.copy()
    o2[5]["strand"] = 2
    for bad, message in ((variant(overlaps=o), "unknown pile"), (variant(begin=begin, end=end), "ends before it begins"),
                         (variant(invalid=inv), "names an invalid pile"), (variant(overlaps=o2), "strand other than 0 or 1")):
        with pytest.raises(ValueError, match=message):
            bad.device(eng)
        usable()
    # the restatement refuses the edge on an invalid pile as well
    assert gu.run_construct(ref, variant(invalid=inv), tmp_path, "bad", ok=(3,))[0] is None
    t = gu.EdgeTable()
    a, b, c = t.nodes(3)
    t.join(a, b, 10)
    t.join(b, c, 10)
    tl, hd, ln = t.arrays()
    with pytest.raises(ValueError, match="odd number"):
        eng.graph_from_edges(6, tl[:3], hd[:3], ln[:3])
    usable()
    for which in (tl, hd):
        x = which.copy()
        x[2] = 6
        with pytest.raises(ValueError, match="unknown node"):
            eng.graph_from_edges(6, x if which is tl else tl, x if which is hd else hd, ln)
        usable()
    x = tl.copy()
    x[3] = gu.EMPTY
    with pytest.raises(ValueError, match="empty pair slot"):
        eng.graph_from_edges(6, x, hd, ln)
    usable()
    g = eng.graph_from_edges(6, tl, hd, ln)
    with pytest.raises(ValueError, match="no completed rvn_graph_mark_transitive"):  # nothing to fetch before a marking
        hip._check(hip.lib().rvn_graph_fetch_transitive(g._h, None, None, None))
    with pytest.raises(ValueError, match="not a number"):
        g.mark_long_edges([1.0, 1.0, float("nan"), 1.0])
    flags, count = g.mark_long_edges([1.0, 1.0, 1.0, 1.0])
    assert count == 0 and flags.sum() == 0
    g.close()
    usable()


def _repeat_rich_genome(n, seed, copies=12, element=6000, div=0.015):
    """n bases with a 6 kb element copied `copies` times at 1.5 % divergence and tandem arrays of a short unit (the
    genome tests/test_gpu_repeats.py builds)"""
    rng = np.random.default_rng(seed)
    g = synth.make_genome(n, seed=seed)
    for e in range(max(1, n // 1_000_000)):
        rep = g[1000 + e * 50_000:1000 + e * 50_000 + element].copy()
        for c in range(copies):
            at = int(rng.integers(0, n - element))
            m = synth.mutate(rng, rep, div, 0.0, 0.0)[:element]
            g[at:at + m.shape[0]] = m
    for _ in range(max(2, n // 200_000)):
        unit = rng.integers(0, 4, size=int(rng.integers(2, 7)), dtype=np.uint8)
        at, ln = int(rng.integers(0, n - 3000)), int(rng.integers(600, 3000))
        g[at:at + ln] = np.tile(unit, ln // unit.shape[0] + 1)[:ln]
    return g


def chain_input(eng, rs, identity=0.0, seed=7):
    """first pass -> resolve (valid regions, medians; some piles made invalid) -> second pass -> repeats on the device:
    the arguments of rvn_construct_assembly_graph"""
    rd = eng.upload(rs)
    p = eng.find_overlaps_and_create_piles(rd)
    b, e, median, invalid = p.trim_and_annotate(4)
    data, off = p.piles()
    p.close()
    begin, end = b.astype(np.uint32) << 4, e.astype(np.uint32) << 4
    invalid = (invalid | (np.random.default_rng(seed).random(rs.n) < 0.15)).astype(np.uint8)
    res = eng.find_overlaps_and_repetitive_regions(rd, begin, end, invalid, freq=0.001, kmer_len=15, identity=identity)
    invalid = (invalid | res["contained"]).astype(np.uint8)
    cov = [data[int(off[i]):int(off[i + 1])] for i in range(rs.n)]
    rd.close()
    stage = ru.StageInput(res["overlaps"], cov, res["kmers"], begin, end, median, invalid)
    rep = stage.device(eng)
    return gu.ConstructInput(rep["overlaps"], begin, end, median, invalid)


def test_chain_matches_the_restatement(eng, ref, tmp_path):
    g = _repeat_rich_genome(2_000_000, seed=11)
    rs, _ = synth.make_reads(g, 30, 10000, seed=12)
    inp = chain_input(eng, rs)
    want, _ = gu.run_construct(ref, inp, tmp_path, "chain")
    graph = inp.device(eng)
    gu.assert_same_tables(graph.fetch(), want)
    order, pairs = graph.mark_transitive()
    gu.assert_same_marks(order, pairs, want)
    graph.close()
    assert want["n_edges"] > 0 and order.shape[0] > 0 and (want["finalized"]["score"] == 4).sum() > 0
