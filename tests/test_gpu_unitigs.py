"""raven::CreateUnitigs on the device (rvn_graph_create_unitigs, raven_amd/csrc/unitigs.hip) against the restatement
(tests/host/unitig_reference.cpp): every table, every new node's tiling and every packed word equal; the refusals; unitigs
of error-free reads equal to the genome they were cut from; unitig sequences as the targets of a polishing round."""
import numpy as np
import pytest

from raven_amd import hip
from tests import polish_util as pu2
from tests import unitig_util as uu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("unitigs")
    return uu.build_reference(d), d


@pytest.fixture(scope="module")
def engine():
    return hip.Engine(15, 5)


def _check(engine, ref, case, eps, tag="c", min_unitig_size=9999):
    exe, d = ref
    want = uu.reference(exe, case, eps, d, tag, min_unitig_size)
    rd, tl, g, u = uu.device_run(engine, case, eps, min_unitig_size)
    uu.assert_same_as_reference(case, want, tl, u)
    return want, rd, tl


@pytest.mark.parametrize("k", [1, 2, 3, 63, 64, 65, 1023, 1024, 1025])
def test_chains_of_every_length_in_both_orientations(engine, ref, k):
    """One chain between two dead ends, on random strands (so either orientation creates) and with every node on the
    reverse strand (the pair creates); the jumping needs ceil(log2 2k) rounds."""
    for seed, flip in ((k, None), (k + 1, "all")):
        rng = np.random.default_rng(seed)
        case, ids = uu.cheap_line_case(rng, k)
        if flip:
            case.table = uu.EdgeTable(case.n_nodes)
            for i in range(k - 1):
                case.join(2 * i + 1, 2 * i + 3, 7, 9)
        want, _, _ = _check(engine, ref, case, 0)
        assert want["begin"].shape[0] == (2 if k > 1 else 0)
        if flip and k > 1:
            assert want["begin"][0] == 2 * (k - 1) and want["end"][0] == 0  # the pair chain holds node 0
    if k >= 63:
        want, _, _ = _check(engine, ref, case, 1)
        assert want["member_offsets"].tolist() == [0, k - 2, 2 * (k - 2)]


def test_a_chain_of_100_000_nodes(engine, ref):
    case, ids = uu.cheap_line_case(np.random.default_rng(99), 100_000)
    want, _, _ = _check(engine, ref, case, 42)
    assert want["member_offsets"].tolist() == [0, 100_000 - 84, 2 * (100_000 - 84)] and want["is_unitig"].tolist() == [1, 1]
    assert want["length"][0] > 1_000_000


@pytest.mark.parametrize("k", [1, 2, 65, 4097])
def test_cycles(engine, ref, k):
    case, ids = uu.cheap_line_case(np.random.default_rng(k), k, circular=True)
    case.count = [3] * case.n_nodes
    want, _, _ = _check(engine, ref, case, 42, min_unitig_size=100)  # (neither trim nor size rule applies to a cycle)
    assert want["is_circular"].tolist() == [1, 1] and want["member_offsets"].tolist() == [0, k, 2 * k]
    assert want["begin"][0] == min(min(ids), min(u ^ 1 for u in ids)) and want["edge_tail"].shape[0] == 0
    assert want["is_unitig"][0] == (1 if 3 * k > 5 and want["length"][0] > 100 else 0)


@pytest.mark.parametrize("eps", [0, 1, 42])
def test_epsilon_on_each_side_of_the_threshold(engine, ref, eps):
    for extra in (1, 2, 3):
        case, ids = uu.line_case(np.random.default_rng(eps * 10 + extra), 2 * eps + extra)
        want, _, _ = _check(engine, ref, case, eps)
        assert want["begin"].shape[0] == (0 if extra == 1 else 2)


def test_chain_ends_empty_slots_and_interleaved_chains(engine, ref):
    """Chains that end in a junction, in a dead end and beside a removed node slot; a node without edges; cycles; many
    short chains interleaved in id order, so that the numbering is not the chain order; nodes of several segments."""
    exe, d = ref
    total = 0
    for seed in range(4):
        rng = np.random.default_rng(500 + seed)
        case = uu.random_tiled_case(rng, n_chains=40, max_chain=7)
        case.node(uu.random_segments(rng, case.reads))  # a node with no edges
        case.node([], present=False)  # a removed slot (graph.nodes[i] == nullptr)
        case.table.hole()
        want, _, _ = _check(engine, ref, case, seed % 2, "mix%d" % seed)
        total += want["begin"].shape[0]
        firsts = want["members"][want["member_offsets"][:-1:2].astype(np.int64)]
        assert (np.diff(want["begin"][::2].astype(np.int64)) < 0).any() or (np.diff(firsts.astype(np.int64)) < 0).any()
        assert want["edge_tail"].shape[0] > 0 and want["is_circular"].any() and not want["is_circular"].all()
    assert total > 100


def test_a_chain_cannot_be_its_own_pair(engine, ref):
    """In a pair-symmetric table a chain that held both u and u ^ 1 would have to pass an edge w -> w ^ 1, whose pair slot
    holds the same tail and head: w then has two out-edges and is a junction.  So the nearest such table makes no unitig
    through w, on either side."""
    case = uu.Case(uu.random_reads(np.random.default_rng(4), 3, 50, 50))
    a, w, b = uu.simple_nodes(case, 3)
    case.join(a, w, 5, 5)
    case.join(w, w ^ 1, 6, 6)
    want, _, _ = _check(engine, ref, case, 0)
    assert want["begin"].shape[0] == 0 and want["marked"].sum() == 0


def test_second_round_over_composite_nodes(engine, ref):
    """Raven's sequence: epsilon = 42, the removal applied to the host's table, rvn_graph_from_edges again with the grown
    node count, epsilon = 0 over nodes that are unitigs themselves (their tilings were appended by the first call)."""
    exe, d = ref
    rng = np.random.default_rng(77)
    case, ids = uu.cheap_line_case(rng, 100)
    more, _ = uu.cheap_line_case(rng, 90)  # a second chain, behind the first in id order, over the first's reads
    base = case.n_nodes
    lens = [r.shape[0] for r in case.reads]
    case.tiling += [[(t[0][0], 0, lens[t[0][0]], t[0][3])] for t in more.tiling]
    for name in ("count", "coverage", "present", "is_unitig"):
        setattr(case, name, getattr(case, name) + getattr(more, name))
    case.table.n_nodes = case.n_nodes
    for t, h, ln in zip(more.table.tail[::2], more.table.head[::2], more.table.length[::2]):
        case.join(t + base, h + base, min(ln, 30), 20)
    case.count = [2] * case.n_nodes
    want1 = uu.reference(exe, case, 42, d, "r1", 1000)
    rd, tl, g, u1 = uu.device_run(engine, case, 42, 1000)
    uu.assert_same_as_reference(case, want1, tl, u1)
    assert want1["begin"].shape[0] == 4 and want1["edge_tail"].shape[0] == 8
    case2 = uu.next_round(case, want1)
    want2 = uu.reference(exe, case2, 0, d, "r2", 1000)
    _, _, _, u2 = uu.device_run(engine, case2, 0, 1000, reads=rd, tiling=tl)
    uu.assert_same_as_reference(case2, want2, tl, u2)
    assert want2["begin"].shape[0] == 4 and (want2["members"] >= case.n_nodes).sum() == 4
    assert want2["member_offsets"][1] == 42 + 1 + 42 and want2["is_unitig"][0] == 1
    # GetUnitigs' nodes, old and new, through the call that materialises any node of the tiling
    words, woff, lens_ = tl.as_reads(want2["selected"]).fetch()[:3]
    seqs = {case2.n_nodes + j: s for j, s in enumerate(want2["sequences"])}
    ew, eo = uu.pack_all([seqs[int(x)] if int(x) in seqs else case2.sequence(int(x)) for x in want2["selected"]])
    assert want2["selected"].shape[0] >= 2 and np.array_equal(woff, eo) and np.array_equal(words, ew)


def test_packing_every_source_and_destination_phase(engine, ref):
    """Unitigs of two members: the first contributes d bases (its out-edge's length: the destination phase, 0 .. 32, 0 being
    an edge of length 0 and 32 a whole word), the second is one segment that starts at base s of its read (the source
    phase), on either strand; 40 bases of it, so that every piece spans two source words somewhere."""
    case = uu.Case(uu.random_reads(np.random.default_rng(8), 8, 96, 96))
    for d_ in range(33):
        for s in range(32):
            for st in (0, 1):
                a = case.node([(d_ % 8, 3, 40, 0)])
                b = case.node([((d_ + s) % 8, s, 40 + (s + d_) % 3, st)])
                case.join(a, b, d_, 40 + (s + d_) % 3 if (s + d_) % 5 == 0 else (s * 7 + d_) % 41)  # (some pair edges as long as their tail)
    want, _, _ = _check(engine, ref, case, 0)
    assert want["begin"].shape[0] == 2 * 33 * 32 * 2


def test_packing_segment_lengths_and_word_ends(engine, ref):
    """Segments of 0, 1, 31, 32, 33 and 64 bases in every order of two, forty one-base segments inside one output word, an
    edge as long as its tail, unitigs that end with a word of 1 base and of 32."""
    rng = np.random.default_rng(9)
    case = uu.Case(uu.random_reads(rng, 6, 128, 128))
    tail_node = lambda: case.node([(1, 5, 20, 1)])
    for x in uu.SEGMENT_LENGTHS:
        for y in uu.SEGMENT_LENGTHS:
            for st in (0, 1):
                if x + y == 0:
                    continue
                a = case.node([(0, 7, x, st), (2, 11, y, st ^ 1), (3, 0, 0, 0)])
                case.join(a, tail_node(), x + y, 20)  # the whole of a: the edge is as long as its tail
    ones = case.node([(i % 6, 3 * i, 1, i % 2) for i in range(40)] + [(4, 0, 30, 0)])
    case.join(ones, tail_node(), 70, 3)
    for total in (33, 64):  # a last word of 1 base and of 32
        a = case.node([(5, 1, 50, 0)])
        b = case.node([(5, 60, total - 13, 1)])
        case.join(a, b, 13, total - 13)
    want, _, _ = _check(engine, ref, case, 0)
    assert want["length"][-2] == 64 and want["length"][-4] == 33 and (want["length"] == 90).any()


def test_refusals_leave_the_engine_usable(engine, ref):
    exe, d = ref
    rng = np.random.default_rng(10)
    good, _ = uu.line_case(rng, 5)
    rd = engine.upload_codes(good.reads)
    off, r, b, ln, st = good.tiling_arrays()

    def works():
        want = uu.reference(exe, good, 0, d, "ok")
        _, tl, _, u = uu.device_run(engine, good, 0, reads=rd)
        uu.assert_same_as_reference(good, want, tl, u)

    # a segment that runs past its read, names an unknown read, has a strand of 2
    for bad in ((r, b, ln + np.uint32(good.reads[0].shape[0]), st), (r + np.uint32(len(good.reads)), b, ln, st), (r, b, ln, st + np.uint8(2))):
        with pytest.raises(ValueError, match="segment 0"):
            engine.tiling_from_segments(rd, off, *bad)
    with pytest.raises(ValueError, match="runs past its read"):
        engine.tiling_from_piles(rd, [0, 0], [0], [good.reads[0].shape[0] + 1])
    works()
    # a chain edge longer than its tail's sequence: the message names it
    case, _ = uu.line_case(rng, 4)
    case.table.length[2] = case.length(case.table.tail[2]) + 1
    assert uu.reference(exe, case, 0, d, "long", ok=(4,)) is None
    rd2 = engine.upload_codes(case.reads)
    tl2 = engine.tiling_from_segments(rd2, *case.tiling_arrays())
    t, h, le = case.table.arrays()
    g = engine.graph_from_edges(case.n_nodes, t, h, le)
    with pytest.raises(ValueError, match="chain edge 2 is longer"):
        g.create_unitigs(tl2, case.count, case.coverage, 0)
    assert tl2.n_nodes == case.n_nodes  # nothing was appended
    works()
    # an edge table that is not pair-symmetric
    t2 = t.copy()
    t2[3] ^= 2
    g2 = engine.graph_from_edges(case.n_nodes, t2, h, np.zeros_like(le))
    with pytest.raises(ValueError, match="edge 2 and its pair slot are not a pair"):
        g2.create_unitigs(tl2, case.count, case.coverage, 0)
    works()
    # a tiling with fewer nodes than the graph
    g3 = engine.graph_from_edges(case.n_nodes + 2, t, h, np.zeros_like(le))
    with pytest.raises(ValueError, match="fewer nodes"):
        g3.create_unitigs(tl2, case.count + [1, 1], case.coverage + [0, 0], 0)
    works()
    # a unitig of 2^32 bases or more: 70 000 nodes of 65 536 bases, all of one read
    big = uu.Case([rng.integers(0, 4, size=65536).astype(np.uint8)])
    k = 70_000
    big.tiling = [[(0, 0, 65536, i & 1)] for i in range(2 * k)]
    big.count, big.coverage, big.present, big.is_unitig = [1] * (2 * k), [0] * (2 * k), [1] * (2 * k), [0] * (2 * k)
    big.table.n_nodes = 2 * k
    big.table.tail = [x for i in range(k - 1) for x in (2 * i, 2 * i + 3)]
    big.table.head = [x for i in range(k - 1) for x in (2 * i + 2, 2 * i + 1)]
    big.table.length = [65536] * (2 * (k - 1))
    with pytest.raises(ValueError, match="new node %d would have 2\\^32 bases or more" % (2 * k)):
        uu.device_run(engine, big, 0)
    works()
    # selections and nodes that do not exist, a read set that is not the tiling's
    _, tl, _, u = uu.device_run(engine, good, 0, reads=rd)
    with pytest.raises(ValueError):
        u.as_reads(2)
    with pytest.raises(ValueError, match="not in the tiling"):
        tl.as_reads([tl.n_nodes])
    tl.reads = rd2
    with pytest.raises(ValueError, match="another read set"):
        tl.as_reads([0])
    tl.reads = rd
    works()


def test_empty_graphs_give_empty_tables(engine):
    rd = engine.upload_codes([np.zeros(40, np.uint8)])
    empty = np.zeros(0, np.uint32)
    tl = engine.tiling_from_segments(rd, np.zeros(1, np.uint64), empty, empty, empty, np.zeros(0, np.uint8))
    g = engine.graph_from_edges(0, empty, empty, empty)
    u = g.create_unitigs(tl, empty, np.zeros(0, np.uint16), 42)
    f = u.fetch()
    assert u.n_new_nodes == 0 and u.n_new_edges == 0 and f["member_offsets"].tolist() == [0] and f["marked"].shape[0] == 0
    assert u.as_reads().n == 0


def _genome_case(seed, genome_len=30_000, read_len=2500, step=500):
    """Error-free reads every `step` bases of a genome, on random strands, trimmed by a valid region of their own, joined
    with their true offsets: (genome, noisy reads of it, read codes, pile begin / end, the edge table along the genome)."""
    truths, _, _, noisy, _ = pu2.make_case(genome_len=genome_len, coverage=20, read_len=2500, seed=seed)
    genome = np.asarray(truths[0], np.uint8)
    rng = np.random.default_rng(seed)
    starts = list(range(0, genome_len - read_len + 1, step))
    reads, begin, end, span, node = [], [], [], [], []
    for i, o in enumerate(starts):
        s = genome[o:o + read_len]
        strand = int(rng.integers(0, 2))
        b, e = int(rng.integers(0, 50)), read_len - int(rng.integers(0, 50))
        reads.append((3 - s[::-1]).astype(np.uint8) if strand else s)
        begin.append(b)
        end.append(e)
        # the valid region on the genome, and the node of this pile that reads along the genome
        span.append((o + read_len - e, o + read_len - b) if strand else (o + b, o + e))
        node.append(2 * i + strand)
    table = uu.EdgeTable(2 * len(starts))
    for i in range(len(starts) - 1):
        table.join(node[i], node[i + 1], span[i + 1][0] - span[i][0], span[i + 1][1] - span[i][1])
    return genome, noisy, reads, begin, end, span, table


def test_unitigs_of_error_free_reads_are_the_genome(engine):
    """Independent of the restatement: the unitig of reads cut from a genome and joined with their true offsets is the
    genome stretch they cover, base for base; its pair is the reverse complement."""
    genome, _, reads, begin, end, span, table = _genome_case(21)
    rd = engine.upload_codes(reads)
    n = len(reads)
    tl = engine.tiling_from_piles(rd, np.repeat(np.arange(n), 2), begin, end)
    g = engine.graph_from_edges(2 * n, *table.arrays())
    u = g.create_unitigs(tl, np.ones(2 * n), np.full(2 * n, 30), 0)
    f = u.fetch()
    assert u.n_new_nodes == 2 and f["count"].tolist() == [n, n] and f["is_unitig"].tolist() == [1, 1] and f["coverage"].tolist() == [30, 30]
    stretch = genome[span[0][0]:span[-1][1]]
    words, woff, lens = u.as_reads(hip.UNITIGS_ALL).fetch()[:3]
    fwd = 0 if f["begin"][0] in (0, 1) and f["begin"][0] == table.tail[0] else 1  # which of the two runs along the genome
    want = [stretch, (3 - stretch[::-1]).astype(np.uint8)]
    ew, eo = uu.pack_all([want[fwd], want[fwd ^ 1]])
    assert lens.tolist() == [stretch.shape[0]] * 2 and np.array_equal(woff, eo) and np.array_equal(words, ew)
    only = u.as_reads().fetch()
    assert np.array_equal(only[0], uu.pack(want[fwd])) and only[2].tolist() == [stretch.shape[0]]


def test_unitig_sequences_are_polishing_targets_where_they_lie(engine):
    """rvn_unitigs_as_reads as the targets of a polishing round over noisy reads, against the same round with the same
    sequences uploaded through rvn_reads_upload_codes: consensus, lengths and ratio byte-identical, the two target sets equal."""
    genome, noisy, reads, begin, end, span, table = _genome_case(33)
    rd = engine.upload_codes(reads)
    n = len(reads)
    tl = engine.tiling_from_piles(rd, np.repeat(np.arange(n), 2), begin, end)
    u = engine.graph_from_edges(2 * n, *table.arrays()).create_unitigs(tl, np.ones(2 * n), np.full(2 * n, 30), 0)
    resident = u.as_reads(hip.UNITIGS_ALL)
    f = u.fetch()
    stretch = genome[span[0][0]:span[-1][1]]
    seqs = [stretch, (3 - stretch[::-1]).astype(np.uint8)]
    if f["begin"][0] != table.tail[0]:
        seqs.reverse()
    via_host = engine.upload_codes(seqs)
    a, b = via_host.fetch(), resident.fetch()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    nd = engine.upload(noisy)
    ch, rh, sh = engine.polish_round(via_host, nd)
    lh = engine.polish_layers()
    cr, rr, sr = engine.polish_round(resident, nd)
    assert np.array_equal(lh, engine.polish_layers()) and sh["n_windows"] == sr["n_windows"] > 100
    assert len(ch) == len(cr) == 2 and all(np.array_equal(x, y) for x, y in zip(ch, cr))
    assert np.array_equal(np.asarray(rh), np.asarray(rr)) and max(rr) > 0.8  # (every read maps best to one of the two orientations)
