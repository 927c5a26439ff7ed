"""rvn_tiling_slices_as_reads (raven_amd/csrc/unitigs.hip) against rvn_reads_upload_codes of the slice strings
(biosoup::NucleicAcid::InflateData(begin, length) as tests/edge_sim_util.py states it on numpy strings): every packed word,
every offset and every length equal; the refusals, each leaving the tiling as it was."""
import numpy as np
import pytest

from raven_amd import hip
from tests import edge_sim_util as eu
from tests import unitig_util as uu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = hip.Engine(15, 5)
    e.set_kernel_timing(True)
    return e


def _device(engine, case):
    rd = engine.upload_codes(case.reads)
    return rd, engine.tiling_from_segments(rd, *case.tiling_arrays())


def _check(engine, case, slices, tiling):
    strings = [eu.slice_string(case, *s) for s in slices]
    got = tiling.slices_as_reads(*eu.slice_arrays(slices))
    words, woff, lens = got.fetch()[:3]
    want = engine.upload_codes(strings).fetch()
    ew, eo = uu.pack_all(strings)
    assert got.n == len(slices) and lens.tolist() == [s.shape[0] for s in strings]
    assert np.array_equal(woff, eo) and np.array_equal(words, ew)
    assert np.array_equal(words, want[0]) and np.array_equal(woff, want[1]) and np.array_equal(lens, want[2])
    return strings


def test_crafted_and_random_slices_and_the_same_list_permuted(engine):
    rng = np.random.default_rng(1)
    case, nodes = eu.crafted_slice_case(rng)
    rd, tl = _device(engine, case)
    crafted = eu.crafted_slices(case, nodes)
    engine.reset_stats()
    strings = _check(engine, case, crafted, tl)
    assert eu.launches(engine)["slice_pack"] == 1
    assert any(s.shape[0] == 0 for s in strings) and strings[-1].shape[0] == 0  # a slice of no bases is a read of length 0

    tiled = eu.slice_case(rng)
    rd2, tl2 = _device(engine, tiled)
    slices = eu.random_slices(rng, tiled, 1000)
    _check(engine, tiled, slices, tl2)
    order = rng.permutation(len(slices))
    _check(engine, tiled, [slices[int(i)] for i in order], tl2)
    # only empty slices, then none at all: no word, no launch
    engine.reset_stats()
    words, woff, lens = tl2.slices_as_reads([0, 1], [tiled.length(0), 0], [9, 0]).fetch()[:3]
    assert words.shape[0] == 0 and woff.tolist() == [0, 0, 0] and lens.tolist() == [0, 0]
    empty = tl2.slices_as_reads([], [], [])
    assert empty.n == 0 and eu.launches(engine)["slice_pack"] == 0


def test_slices_of_a_grown_tiling(engine):
    """Nodes that rvn_graph_create_unitigs appended: lists of several cut segments."""
    rng = np.random.default_rng(2)
    case = uu.random_tiled_case(rng, n_chains=12, max_chain=7)
    rd, tl, g, u = uu.device_run(engine, case, 0)
    grown = uu.next_round(case, dict(u.fetch(), alive=np.ones(case.n_nodes + u.n_new_nodes, np.uint8)))
    assert u.n_new_nodes >= 6 and grown.n_nodes == tl.n_nodes
    slices = [(int(x), b, ln) for x in range(case.n_nodes, grown.n_nodes)
              for b, ln in ((0, 0xFFFFFFFF), (grown.length(int(x)) // 3, 70), (33, grown.length(int(x))))]
    _check(engine, grown, slices + eu.random_slices(rng, grown, 200), tl)


def test_refusals_leave_the_tiling_as_it_was(engine):
    rng = np.random.default_rng(3)
    case, (a, b, c) = eu.crafted_slice_case(rng)
    rd, tl = _device(engine, case)
    before = tl.fetch()
    good = [(a, 5, 100), (b ^ 1, 0, 0xFFFFFFFF), (c, 0, 1)]

    def unchanged():
        now = tl.fetch()
        assert all(np.array_equal(before[k], now[k]) for k in before)
        _check(engine, case, good, tl)

    unchanged()
    with pytest.raises(ValueError, match="node %d \\(slice 1\\) is not in the tiling" % case.n_nodes):
        tl.slices_as_reads([a, case.n_nodes], [0, 0], [1, 1])
    unchanged()
    other = engine.upload_codes(case.reads)
    tl.reads = other
    with pytest.raises(ValueError, match="another read set"):
        tl.slices_as_reads([a], [0], [1])
    tl.reads = rd
    unchanged()
    # 2^32 packed words: 2^21 slices of 65 536 bases (2 048 words) each, all of one node
    big = uu.Case([rng.integers(0, 4, size=65536).astype(np.uint8)])
    u = big.node([(0, 0, 65536, 0)])
    rd2, tl2 = _device(engine, big)
    k = 1 << 21
    engine.reset_stats()
    with pytest.raises(ValueError, match="2\\^32 packed words or more"):
        tl2.slices_as_reads(np.full(k, u, np.uint32), np.zeros(k, np.uint32), np.full(k, 0xFFFFFFFF, np.uint32))
    assert eu.launches(engine)["slice_pack"] == 0
    assert tl2.fetch()["node_length"].tolist() == [65536, 65536]
    unchanged()
