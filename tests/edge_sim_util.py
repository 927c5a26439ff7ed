"""Shared pieces of the edge-similarity tests: the restatement (tests/host/edge_similarity_reference.cpp), the host build of
the slice and edge rules (tests/host/slice_rules_host.cpp), their binary formats, slices as numpy strings, and builders of
graphs whose overlaps are known by construction."""
import os
import subprocess

import numpy as np

from tests.graph_util import ROOT, Reader, _run
from tests.unitig_util import Case

SLOT_EMPTY = 0xFFFFFFFF
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_reference(tmp_path, sanitize=False):
    exe = str(tmp_path / ("edge_similarity_reference_san" if sanitize else "edge_similarity_reference"))
    subprocess.check_call(["g++", "-std=c++17"] + (SANITIZE if sanitize else ["-O2"]) +
                          ["-o", exe, os.path.join(ROOT, "tests", "host", "edge_similarity_reference.cpp")])
    return exe


def build_rules_program(tmp_path, sanitize=False):
    exe = str(tmp_path / ("slice_rules_host_san" if sanitize else "slice_rules_host"))
    subprocess.check_call(["g++", "-std=c++17"] + (SANITIZE if sanitize else ["-O2"]) +
                          ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "raven_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "slice_rules_host.cpp")])
    return exe


def bits(x):
    """float64 values as their bit patterns: NaNs compare like any other value."""
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---- slices ------------------------------------------------------------------------------------------------------------------

def slice_string(case, node, begin, length):
    """biosoup::NucleicAcid::InflateData(begin, length) of a node, on its numpy string."""
    s = case.sequence(int(node))
    if begin >= s.shape[0]:
        return np.zeros(0, np.uint8)
    return s[begin:begin + min(int(length), s.shape[0] - int(begin))]


def slice_arrays(slices):
    a = np.asarray(slices, np.int64).reshape(-1, 3)
    return a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32)


def host_slices(exe, case, slices, tmp_path, tag="s"):
    """The host build of the slice rule: (lengths, word offsets, words, strings by segment_slice)."""
    soff, rd, bg, ln, st = case.tiling_arrays()
    nd, b, l = slice_arrays(slices)
    blob = b"".join([case.reads_blob(), np.uint32(case.n_nodes).tobytes(), soff.tobytes(), rd.tobytes(), bg.tobytes(), ln.tobytes(),
                     st.tobytes(), np.uint32(nd.shape[0]).tobytes(), nd.tobytes(), b.tobytes(), l.tobytes()])
    out, _ = _run(exe, "slices", blob, tmp_path, tag)
    r = Reader(out)
    lens = r.take(np.uint32, nd.shape[0])
    woff = r.take(np.uint64, nd.shape[0] + 1)
    words = r.take(np.uint64, woff[-1])
    boff = r.take(np.uint64, nd.shape[0] + 1)
    bases = r.take(np.uint8, boff[-1])
    assert r.done()
    return lens, woff, words, [bases[int(boff[i]):int(boff[i + 1])] for i in range(nd.shape[0])]


def host_edges(exe, tail_len, edge_len, head_len, tmp_path, tag="e"):
    t, e, h = (np.asarray(x, np.uint32) for x in (tail_len, edge_len, head_len))
    out, _ = _run(exe, "edges", np.uint32(t.shape[0]).tobytes() + t.tobytes() + e.tobytes() + h.tobytes(), tmp_path, tag)
    r = Reader(out)
    return r.take(np.uint32, t.shape[0]), r.take(np.uint32, t.shape[0])


def slice_case(rng, n_nodes=40, n_reads=12):
    """Nodes that are tilings of 1 .. 6 segments of both strands (lengths 0, 1, 31, 32, 33, 64 and random ones)."""
    from tests.unitig_util import random_reads, random_segments
    case = Case(random_reads(rng, n_reads, 120, 260))
    for _ in range(n_nodes // 2):
        case.node(random_segments(rng, case.reads, max_segments=6))
    return case


def crafted_slice_case(rng):
    """Node a: boundaries at 40, 73, 73 (a zero-length segment inside), 137, 150, 214; b: one segment on strand 1; c: no bases."""
    from tests.unitig_util import random_reads
    case = Case(random_reads(rng, 6, 200, 260))
    a = case.node([(0, 7, 40, 0), (1, 11, 33, 1), (2, 0, 0, 0), (3, 5, 64, 1), (4, 9, 13, 0), (5, 100, 64, 1)])
    b = case.node([(2, 30, 90, 1)])
    c = case.node([(3, 17, 0, 0)])
    return case, (a, b, c)


def crafted_slices(case, nodes):
    """begin at 0, 31, 32, 33; ends on a segment edge; spans of three segments and more; a zero-length segment inside;
    length 0; begin == length(u) and beyond; len beyond the end (the clamp)."""
    a, b, c = nodes
    out = []
    for u in (a, a ^ 1, b, b ^ 1):
        L = case.length(u)
        for begin in (0, 31, 32, 33):
            for ln in (0, 1, 31, 32, 33, 64, 65, L, 0xFFFFFFFF):
                out.append((u, begin, ln))
        out += [(u, L, 5), (u, L + 1, 5), (u, 0xFFFFFFFF, 0xFFFFFFFF), (u, L - 1, 1), (u, L - 1, 2), (u, 0, L), (u, 0, L + 1)]
    # node a: ends on the edges 40, 73, 137; from an edge; across the zero-length segment; three segments and more
    out += [(a, 0, 40), (a, 5, 35), (a, 40, 33), (a, 39, 1), (a, 40, 1), (a, 72, 2), (a, 73, 64), (a, 41, 96), (a, 39, 99),
            (a, 10, 140), (a, 1, 213), (a, 0, 214), (a ^ 1, 64, 13), (a ^ 1, 60, 90), (a ^ 1, 3, 200)]
    out += [(c, 0, 0), (c, 0, 7), (c, 1, 7), (c ^ 1, 0, 0xFFFFFFFF)]
    return out


def random_slices(rng, case, n):
    out = []
    for _ in range(n):
        u = int(rng.integers(0, case.n_nodes))
        L = case.length(u)
        begin = int(rng.choice([0, 31, 32, 33, L, L + 1, int(rng.integers(0, L + 2))]))
        ln = int(rng.choice([0, 1, 32, L, 0xFFFFFFFF, int(rng.integers(0, L + 2)), int(rng.integers(0, L + 2))]))
        out.append((u, begin, ln))
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def reference_blob(case):
    t, h, ln = case.table.arrays()
    seqs = [case.sequence(u) for u in range(case.n_nodes)]
    off = np.zeros(case.n_nodes + 1, np.uint64)
    if seqs:
        np.cumsum([s.shape[0] for s in seqs], out=off[1:])
    return b"".join([np.uint32(case.n_nodes).tobytes(), np.uint64(t.shape[0]).tobytes(), t.tobytes(), h.tobytes(), ln.tobytes(),
                     off.tobytes(), (np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)).tobytes()])


def reference(exe, case, tmp_path, tag="r"):
    """The restatement on a case: dict(lhs_length, rhs_length, distance, score, seconds = the loop's own time)."""
    b, p = _run(exe, "similarity", reference_blob(case), tmp_path, tag)
    E = len(case.table.tail)
    r = Reader(b)
    out = dict(lhs_length=r.take(np.uint32, E), rhs_length=r.take(np.uint32, E), distance=r.take(np.uint32, E),
               score=r.take(np.float64, E))
    assert r.done()
    out["seconds"] = float(p.stderr.split()[1]) if p.stderr.startswith("similarity ") else None
    return out


def distances(exe, pairs, tmp_path, tag="d"):
    """The restatement's edit distance of every (a, b) of code arrays."""
    parts = [np.uint32(len(pairs)).tobytes()]
    for a, b in pairs:
        a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
        parts += [np.uint64(a.shape[0]).tobytes(), np.uint64(b.shape[0]).tobytes(), a.tobytes(), b.tobytes()]
    out, _ = _run(exe, "distance", b"".join(parts), tmp_path, tag)
    return np.frombuffer(out, np.uint32).copy()


def edge_strings(case, e):
    """(lhs, rhs) of edge e by the rule, on numpy strings."""
    t, h, L = case.table.tail[e], case.table.head[e], case.table.length[e]
    lhs = slice_string(case, t, L, 0xFFFFFFFF)
    return lhs, slice_string(case, h, 0, lhs.shape[0])


def assert_same(got, want):
    """All four arrays of the device call equal the restatement's, the scores by bit pattern."""
    for k in ("lhs_length", "rhs_length", "distance"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert np.array_equal(bits(got["score"]), bits(want["score"])), "score"


# ---- graphs --------------------------------------------------------------------------------------------------------------

def codes(text):
    return np.array(["ACGT".index(c) for c in text], np.uint8)


def whole_read_node(case, seq):
    """A node pair whose forward node is the whole of a new read."""
    case.reads.append(np.asarray(seq, np.uint8))
    return case.node([(len(case.reads) - 1, 0, len(seq), 0)])


def hand_case():
    """Edges whose values are derived by hand (every node the whole of a read of its own).  Returns (case, expected): per
    edge id (lhs_length, rhs_length, distance, score as the double arithmetic of graph_repr.cc:254 gives it, None = NaN)."""
    case = Case([])
    O = "ACGTTGCAAC"  # the overlap, ten bases
    X, Y = "GGATCCGGATCCTTAAGGCC", "TTTTGGGGCC"
    want = {}
    # identical overlap: lhs = O, rhs = O.  Its pair is one base longer than the mirror image of the overlap: lhs = rc(O)
    # without its first base, rhs = the first nine bases of rc(O): a shift by one, distance 2 — an edge and its pair differ
    a, b = whole_read_node(case, codes(X + O)), whole_read_node(case, codes(O + Y))
    e = case.join(a, b, len(X), len(Y) + 1)
    want[e] = (10, 10, 0, 1.0)
    want[e + 1] = (9, 9, 2, 1 - 2 / 9.0)
    # one substitution in ten bases
    O1 = O[:4] + "A" + O[5:]  # T -> A at position 4
    c, d = whole_read_node(case, codes(X + O)), whole_read_node(case, codes(O1 + Y))
    e = case.join(c, d, len(X), len(Y))
    want[e] = (10, 10, 1, 1 - 1 / 10.0)
    want[e + 1] = (10, 10, 1, 1 - 1 / 10.0)
    # one insertion: the head holds O with a G behind its fourth base; its first ten bases lack O's last one
    O2 = O[:4] + "G" + O[4:]
    f, g = whole_read_node(case, codes(X + O)), whole_read_node(case, codes(O2 + Y))
    e = case.join(f, g, len(X), len(Y))
    want[e] = (10, 10, 2, 1 - 2 / 10.0)
    # the pair: rc(O2) = GTTGCA C ACGT against rc(O) and one base of rc(X) = GTTGCA ACGT G: the C goes, a G comes
    want[e + 1] = (11, 11, 2, 1 - 2 / 11.0)
    # head shorter than the overlap: rhs clamped to the head's six bases, all of them O's first six
    h, i = whole_read_node(case, codes(X + O)), whole_read_node(case, codes(O[:6]))
    e = case.join(h, i, len(X), 0)
    want[e] = (10, 6, 4, 1 - 4 / 10.0)
    want[e + 1] = (6, 6, 6, 0.0)  # the pair: CAACGT against GTTGCA (the test holds every entry to a plain DP as well)
    # L == length(tail), and L wrapped in 32 bits: no lhs, no rhs, distance 0, 0 / 0.
    j, k = whole_read_node(case, codes(X + O)), whole_read_node(case, codes(O + Y))
    e = case.join(j, k, len(X + O), 0xFFFFFFF0)
    want[e] = (0, 0, 0, None)
    want[e + 1] = (0, 0, 0, None)
    # a head of no bases: rhs is empty, the distance is lhs' length, the score 0
    m, n = whole_read_node(case, codes(X + O)), whole_read_node(case, codes(""))
    e = case.join(m, n, len(X), 0)
    want[e] = (10, 0, 10, 0.0)
    want[e + 1] = (0, 0, 0, None)  # the pair's tail has no bases
    return case, want


def dp_distance(a, b):
    """The textbook DP, row by row."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    prev = np.arange(b.shape[0] + 1)
    for i in range(a.shape[0]):
        cur = np.empty_like(prev)
        cur[0] = i + 1
        sub = prev[:-1] + (b != a[i])
        for j in range(b.shape[0]):
            cur[j + 1] = min(sub[j], prev[j + 1] + 1, cur[j] + 1)
        prev = cur
    return int(prev[-1])


def mutate(rng, seq, rate):
    """Substitutions, insertions and deletions at about `rate` per base."""
    out = []
    for x in np.asarray(seq, np.uint8):
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(int(rng.integers(0, 4)))
        elif r < rate:
            x = (int(x) + int(rng.integers(1, 4))) & 3
        out.append(int(x))
    return np.asarray(out, np.uint8)


def single_segment_case(rng, n_reads=24, read_len=(300, 700), overlap=(1, 260), rate=0.1, n_edges=60):
    """Reads along a genome (with errors), node 2 i / 2 i + 1 = the valid region of read i and its reverse complement, as
    rvn_tiling_from_piles makes them; edges between random node pairs of either strand, lengths around the tail's length.
    Returns (case, pile_begin, pile_end)."""
    case = Case([rng.integers(0, 4, size=int(rng.integers(*read_len))).astype(np.uint8) for _ in range(n_reads)])
    begin = [int(rng.integers(0, 20)) for _ in case.reads]
    end = [r.shape[0] - int(rng.integers(0, 20)) for r in case.reads]
    for i in range(n_reads):
        case.node([(i, begin[i], end[i] - begin[i], 0)])
    for _ in range(n_edges):
        t, h = int(rng.integers(0, 2 * n_reads)), int(rng.integers(0, 2 * n_reads))
        ov = [int(rng.integers(*overlap)) for _ in range(2)]
        case.join(t, h, max(case.length(t) - ov[0], 0), max(case.length(h ^ 1) - ov[1], 0))
    return case, np.asarray(begin, np.uint32), np.asarray(end, np.uint32)


def overlap_case(rng, lengths, rate, multi=False, strands=True, flip=False, mutator=None):
    """Per entry of `lengths` an edge whose overlap has that many bases on the tail: the head starts with a copy of the
    tail's end mutated at `rate` (rate 0: identical; rate None: an unrelated head; rate "different": the overlap is all A
    on the tail and all C on the head, so the distance is its length).  flip: a node of the edge is, at random, the odd node
    of its pair (the stored read holds the reverse complement), so every strand combination occurs with related overlaps.
    mutator: another function of (rng, sequence, rate) in the place of mutate (tools/time_edge_similarity.py: a vectorised one).  multi: every node is
    cut into three segments of reads of either strand; multi = "mixed": every third node is, so that edges of both routes and of one node of each kind occur."""
    case = Case([])

    def node(seq):
        seq = np.asarray(seq, np.uint8)
        odd = int(flip and rng.integers(0, 2))  # the node asked for is u ^ 1: u is made of the reverse complement
        if odd:
            seq = (3 - seq[::-1]).astype(np.uint8)
        if not multi or seq.shape[0] < 3 or (multi == "mixed" and (case.n_nodes // 2) % 3 != 0):
            return whole_read_node(case, seq) ^ odd
        cuts = sorted(int(x) for x in rng.integers(0, seq.shape[0] + 1, size=2))
        segs = []
        for lo, hi in ((0, cuts[0]), (cuts[0], cuts[1]), (cuts[1], seq.shape[0])):
            part = seq[lo:hi]
            st = int(rng.integers(0, 2)) if strands else 0
            pad = int(rng.integers(0, 9))
            stored = (3 - part[::-1]).astype(np.uint8) if st else part
            case.reads.append(np.concatenate([rng.integers(0, 4, size=pad).astype(np.uint8), stored,
                                              rng.integers(0, 4, size=3).astype(np.uint8)]))
            segs.append((len(case.reads) - 1, pad, hi - lo, st))
        return case.node(segs) ^ odd

    for n in lengths:
        front = rng.integers(0, 4, size=int(rng.integers(0, 50))).astype(np.uint8)
        ov = rng.integers(0, 4, size=n).astype(np.uint8)
        if rate is None:
            copy = rng.integers(0, 4, size=n).astype(np.uint8)
        elif rate == "different":
            ov, copy = np.zeros(n, np.uint8), np.ones(n, np.uint8)
        else:
            copy = (mutator or mutate)(rng, ov, rate) if rate else ov
        back = rng.integers(0, 4, size=int(rng.integers(0, 50))).astype(np.uint8)
        t, h = node(np.concatenate([front, ov])), node(np.concatenate([copy, back]))
        case.join(t, h, front.shape[0], back.shape[0])
    return case


def permuted(case, rng):
    """The same case with its edge pairs in another order: (case, order) with new pair p = old pair order[p]."""
    E = len(case.table.tail)
    order = rng.permutation(E // 2)
    out = Case(case.reads)
    out.tiling, out.count, out.coverage, out.present, out.is_unitig = case.tiling, case.count, case.coverage, case.present, case.is_unitig
    out.table.n_nodes = case.table.n_nodes
    for p in order:
        for x in (2 * int(p), 2 * int(p) + 1):
            out.table.tail.append(case.table.tail[x])
            out.table.head.append(case.table.head[x])
            out.table.length.append(case.table.length[x])
    return out, order


def device(engine, case, piles=None):
    """(reads, tiling, graph) of a case on the device; piles = (begin, end): the tiling by rvn_tiling_from_piles."""
    rd = engine.upload_codes(case.reads)
    if piles is None:
        tl = engine.tiling_from_segments(rd, *case.tiling_arrays())
    else:
        tl = engine.tiling_from_piles(rd, np.arange(case.n_nodes, dtype=np.uint32) // 2, piles[0], piles[1])
    return rd, tl, engine.graph_from_edges(case.n_nodes, *case.table.arrays())


def launches(engine):
    return {k: int(v[1]) for k, v in engine.kernel_ms().items()}
