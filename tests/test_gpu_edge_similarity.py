"""rvn_graph_edge_similarity (raven_amd/csrc/edge_similarity.hip) against the restatement
(tests/host/edge_similarity_reference.cpp): the two slice lengths, the distance and the score of every edge slot equal, the
scores by bit pattern; which route the edges took (the direct one copies no base: no slice_pack launch), the chunks of the
packed route, and the routes of distances beyond the wave ring."""
import numpy as np
import pytest

from raven_amd import hip
from tests import edge_sim_util as eu
from tests import unitig_util as uu

pytestmark = pytest.mark.gpu

WAVE_RING = 8064


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("edge_similarity")
    return eu.build_reference(d), d


@pytest.fixture(scope="module")
def engine():
    e = hip.Engine(15, 5)
    e.set_kernel_timing(True)
    return e


def _check(engine, ref, case, tag, piles=None, want=None):
    """The device call on a case equals the restatement; returns (restatement, launches of the call)."""
    exe, d = ref
    want = eu.reference(exe, case, d, tag) if want is None else want
    rd, tl, g = eu.device(engine, case, piles)
    engine.reset_stats()
    got = g.edge_similarity(tl)
    eu.assert_same(got, want)
    return want, eu.launches(engine)


def test_single_segment_graph_every_strand_combination_copies_no_base(engine, ref):
    rng = np.random.default_rng(1)
    case, begin, end = eu.single_segment_case(rng)
    live = [(t & 1, h & 1) for t, h in zip(case.table.tail, case.table.head)]
    assert set(live) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    want, la = _check(engine, ref, case, "single", piles=(begin, end))
    assert la["slice_pack"] == 0 and la["edge_pairs"] == 2
    assert (want["lhs_length"] > 0).sum() > 100 and len(set(want["distance"].tolist())) > 50
    # related overlaps on all four combinations: an overlap and its mirror image, mutated
    related = eu.overlap_case(rng, (40, 200, 700, 1500, 90, 333, 64, 1000), 0.12, flip=True)
    assert {(t & 1, h & 1) for t, h in zip(related.table.tail[0::2], related.table.head[0::2])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    want, la = _check(engine, ref, related, "related")
    assert la["slice_pack"] == 0
    assert (want["distance"][0::2] > 0).all() and (want["distance"] < 0.3 * want["lhs_length"]).all()  # overlaps with errors


def test_multi_segment_and_mixed_graphs(engine, ref):
    rng = np.random.default_rng(2)
    multi = eu.overlap_case(rng, (1, 5, 90, 400, 1200, 2500), 0.1, multi=True, flip=True)
    assert sum(len(t) == 3 for t in multi.tiling) >= 20
    want, la = _check(engine, ref, multi, "multi")
    assert la["slice_pack"] == 1 and (want["distance"] > 0).any()
    mixed = eu.overlap_case(rng, (30, 64, 333, 900, 1000, 77, 2100, 8, 640), 0.15, multi="mixed")
    kinds = {(len(mixed.tiling[t]) > 1, len(mixed.tiling[h]) > 1) for t, h in zip(mixed.table.tail, mixed.table.head)}
    assert kinds == {(False, False), (True, False), (False, True)}
    want, la = _check(engine, ref, mixed, "mixed")
    assert la["slice_pack"] == 1
    # unitigs that rvn_graph_create_unitigs appended, on a graph that joins them
    tiled = uu.random_tiled_case(rng, n_chains=10, max_chain=6)
    rd, tl, g, u = uu.device_run(engine, tiled, 0)
    grown = uu.next_round(tiled, dict(u.fetch(), alive=np.ones(tiled.n_nodes + u.n_new_nodes, np.uint8)))
    assert u.n_new_nodes >= 4
    exe, d = ref
    g2 = engine.graph_from_edges(grown.n_nodes, *grown.table.arrays())
    eu.assert_same(g2.edge_similarity(tl), eu.reference(exe, grown, d, "grown"))


def test_crafted_length_cases_empty_slots_parallel_edges_and_a_permuted_table(engine, ref):
    case, hand = eu.hand_case()
    case.table.hole()
    e = case.join(0, 2, 20, 10)  # parallel to edge 0, and once more with another length
    case.join(0, 2, 23, 0xFFFFFFFF)
    case.table.hole()
    want, la = _check(engine, ref, case, "hand")
    for x, (l, r, dist, score) in hand.items():
        assert (want["lhs_length"][x], want["rhs_length"][x], want["distance"][x]) == (l, r, dist)
    E = len(case.table.tail)
    assert want["distance"][[12, 13, E - 2, E - 1]].tolist() == [eu.SLOT_EMPTY] * 4 and np.isnan(want["score"][[12, 13]]).all()
    assert want["score"][e] == 1.0 and np.isnan(want["score"][8]) and want["distance"][8] == 0 and want["score"][10] == 0.0
    assert la["slice_pack"] == 0
    # the same on nodes of several segments, and with the edge pairs in another order: per-edge values unchanged
    rng = np.random.default_rng(3)
    multi = eu.overlap_case(rng, (10, 10, 64, 300, 301, 900), 0.1, multi="mixed")
    multi.table.hole()
    multi.join(0, 3, 0xFFFFFFF0, multi.length(0))
    multi.join(2, 5, multi.length(2), 0)
    want, _ = _check(engine, ref, multi, "multi_lengths")
    shuffled, order = eu.permuted(multi, rng)
    want2, _ = _check(engine, ref, shuffled, "shuffled")
    at = np.array([2 * int(p) + k for p in order for k in (0, 1)])
    for k in ("lhs_length", "rhs_length", "distance"):
        assert np.array_equal(want2[k], want[k][at])
    assert np.array_equal(eu.bits(want2["score"]), eu.bits(want["score"][at]))


@pytest.mark.parametrize("multi", [False, True])
def test_slice_lengths_at_the_block_and_lane_window_edges(engine, ref, multi):
    """1, 63, 64, 65 (the 64-row blocks) and 385, 386 (the widest lane window's threshold for equal lengths), each with
    distance 0 and with every base different."""
    rng = np.random.default_rng(4 + int(multi))
    lengths = (1, 63, 64, 65, 385, 386)
    same = eu.overlap_case(rng, lengths, 0, multi=multi)
    want, _ = _check(engine, ref, same, "same%d" % multi)
    assert want["lhs_length"][0::2].tolist() == list(lengths) and not want["distance"][0::2].any()
    assert (want["score"][0::2] == 1.0).all()
    other = eu.overlap_case(rng, lengths, "different", multi=multi)
    want, _ = _check(engine, ref, other, "other%d" % multi)
    assert want["lhs_length"][0::2].tolist() == list(lengths) and want["distance"][0::2].tolist() == list(lengths)
    assert not want["score"][0::2].any()


def test_forced_chunking_gives_the_same_as_one_chunk(engine, ref):
    rng = np.random.default_rng(6)
    case = eu.overlap_case(rng, [int(x) for x in rng.integers(500, 900, size=12)], 0.1, multi=True)
    want, la = _check(engine, ref, case, "chunks")
    assert la["slice_pack"] == 1
    # 1 KB = 128 packed words = 4 096 bases a chunk; the 24 edges' slices sum to 30 000 bases and more
    assert int(want["lhs_length"].sum()) + int(want["rhs_length"].sum()) > 30_000
    before = engine.set_option("edge_slices_budget_kb", 1)
    try:
        _, la = _check(engine, ref, case, "chunks", want=want)
    finally:
        engine.set_option("edge_slices_budget_kb", before)
    assert la["slice_pack"] >= 3
    _, la = _check(engine, ref, case, "chunks", want=want)
    assert la["slice_pack"] == 1


@pytest.fixture(scope="module")
def long_pair(ref):
    """Two unrelated sequences of 17 000 bases as tail and head of one edge of length 0 (its pair is as long as its tail: no
    overlap), and the restatement's values."""
    exe, d = ref
    rng = np.random.default_rng(7)
    a, b = (rng.integers(0, 4, size=17_000).astype(np.uint8) for _ in range(2))
    case = uu.Case([])
    t, h = eu.whole_read_node(case, a), eu.whole_read_node(case, b)
    case.join(t, h, 0, 17_000)
    want = eu.reference(exe, case, d, "long")
    # a precondition of the input, not a tolerance: the pair lies beyond the wave ring
    assert want["distance"][0] > WAVE_RING and want["lhs_length"].tolist() == [17_000, 0]
    return case, want, (a, b)


def _edit(la):
    return {k: la[k] for k in ("edit_wide", "edit_full")}


def test_beyond_the_wave_ring_the_workgroup_ring_then_the_full_sweep(engine, ref, long_pair):
    case, want, (a, b) = long_pair
    _, la = _check(engine, ref, case, "long", want=want)
    assert _edit(la) == dict(edit_wide=1, edit_full=0) and la["edit_banded"] == 1
    try:
        engine.set_option("ed_wide_lanes", 64)  # a ring of 8 064: the pair is handed on
        _, la = _check(engine, ref, case, "long", want=want)
        assert _edit(la) == dict(edit_wide=1, edit_full=1)
        engine.set_option("ed_wide_lanes", 1)  # no workgroup ring
        _, la = _check(engine, ref, case, "long", want=want)
        assert _edit(la) == dict(edit_wide=0, edit_full=1)
    finally:
        engine.set_option("ed_wide_lanes", -1)
    # the old callers' route is untouched: the same two strings through rvn_edit_distance_batch, in the same engine
    rd = engine.upload_codes([a, b])
    pairs = np.zeros(1, hip.ED_PAIR_DTYPE)
    pairs[0] = (0, 0, a.shape[0], 1, 0, b.shape[0], 1, 0)
    engine.reset_stats()
    dist = engine.edit_distance_batch(rd, pairs)[0]
    assert dist.tolist() == [int(want["distance"][0])]
    assert _edit(eu.launches(engine)) == dict(edit_wide=0, edit_full=1)


def test_beyond_the_wave_ring_on_packed_slices(engine, ref):
    """The same size on nodes of three segments each, beside short edges: the chunk's pairs take the same route."""
    rng = np.random.default_rng(8)
    case = eu.overlap_case(rng, (17_000, 120), None, multi=True)
    want, la = _check(engine, ref, case, "long_multi")
    assert want["distance"][0] > WAVE_RING
    assert la["slice_pack"] == 1 and la["edit_wide"] == 1 and la["edit_full"] == 0


def test_refusals_and_the_empty_graph(engine, ref):
    rng = np.random.default_rng(9)
    case = eu.overlap_case(rng, (50, 60), 0.1)
    rd, tl, g = eu.device(engine, case)
    small = engine.graph_from_edges(case.n_nodes - 2, [0, 3], [2, 1], [5, 5])
    with pytest.raises(ValueError, match="the tiling has %d nodes, the graph %d" % (case.n_nodes, case.n_nodes - 2)):
        small.edge_similarity(tl)
    other = engine.upload_codes(case.reads)
    tl.reads = other
    with pytest.raises(ValueError, match="another read set"):
        g.edge_similarity(tl)
    tl.reads = rd
    exe, d = ref
    eu.assert_same(g.edge_similarity(tl), eu.reference(exe, case, d, "after_refusals"))
    none = engine.graph_from_edges(case.n_nodes, [], [], [])
    got = none.edge_similarity(tl)
    assert all(got[k].shape[0] == 0 for k in got)
