"""Shared pieces of the unitig tests: the restatement (tests/host/unitig_reference.cpp), the host build of unitig_rules.h
(tests/host/unitig_rules_host.cpp), their binary formats, and a builder of graphs whose nodes are tilings of reads."""
import os
import subprocess

import numpy as np

from tests.graph_util import EMPTY, ROOT, EdgeTable, Reader, _run

TABLE_KEYS = ("begin", "end", "is_circular", "count", "length", "coverage", "is_unitig", "member_offsets", "members", "marked",
              "edge_tail", "edge_head", "edge_length")


def build_reference(tmp_path):
    exe = str(tmp_path / "unitig_reference")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "host", "unitig_reference.cpp")])
    return exe


def build_rules_program(tmp_path, sanitize=False):
    exe = str(tmp_path / ("unitig_rules_host_san" if sanitize else "unitig_rules_host"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I",
                           os.path.join(ROOT, "raven_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "unitig_rules_host.cpp")])
    return exe


def pack(codes):
    """2-bit packed words of one sequence as the device holds them: base x of a word at bits 2x, zero above the last."""
    c = np.asarray(codes, np.uint64)
    w = np.zeros((c.shape[0] + 31) // 32, np.uint64)
    for x in range(32):
        part = c[x::32]
        w[:part.shape[0]] |= part << np.uint64(2 * x)
    return w


def pack_all(seqs):
    """(words, word offsets) of a list of sequences, every one on a word boundary."""
    words = [pack(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, np.uint64)
    if seqs:
        np.cumsum([w.shape[0] for w in words], out=off[1:])
    return (np.concatenate(words) if words else np.zeros(0, np.uint64)), off


class Case:
    """Reads, a tiling of them per node, and an edge table over the nodes.  Nodes come in pairs (2i, 2i + 1)."""

    def __init__(self, reads):
        self.reads = [np.asarray(r, np.uint8) for r in reads]
        self.table = EdgeTable()
        self.tiling = []  # per node: list of (read, begin, length, strand)
        self.count, self.coverage, self.present, self.is_unitig = [], [], [], []

    @property
    def n_nodes(self):
        return len(self.tiling)

    def node(self, segments, count=1, coverage=0, rc_segments=None, rc_count=None, present=True):
        """A node pair: the forward node's segments; its pair is their reverse complement unless stated.  Returns the
        forward id."""
        segments = [tuple(int(x) for x in s) for s in segments]
        if rc_segments is None:
            rc_segments = [(r, b, ln, st ^ 1) for r, b, ln, st in reversed(segments)]
        u = self.n_nodes
        self.tiling += [segments, [tuple(int(x) for x in s) for s in rc_segments]]
        self.count += [count, count if rc_count is None else rc_count]
        self.coverage += [coverage, coverage]
        self.present += [int(present)] * 2
        self.is_unitig += [0, 0]
        self.table.n_nodes = self.n_nodes
        return u

    def join(self, t, h, length, length_pair):
        return self.table.join(t, h, length, length_pair)

    def sequence(self, u):
        parts = [np.zeros(0, np.uint8)]
        for r, b, ln, st in self.tiling[u]:
            s = self.reads[r][b:b + ln]
            parts.append((3 - s[::-1]).astype(np.uint8) if st else s)
        return np.concatenate(parts)

    def length(self, u):
        return sum(s[2] for s in self.tiling[u])

    def tiling_arrays(self):
        off = np.zeros(self.n_nodes + 1, np.uint64)
        if self.n_nodes:
            np.cumsum([len(t) for t in self.tiling], out=off[1:])
        flat = np.array([s for t in self.tiling for s in t], np.int64).reshape(-1, 4)
        return off, flat[:, 0].astype(np.uint32), flat[:, 1].astype(np.uint32), flat[:, 2].astype(np.uint32), flat[:, 3].astype(np.uint8)

    def reads_blob(self):
        off = np.zeros(len(self.reads) + 1, np.uint64)
        if self.reads:
            np.cumsum([r.shape[0] for r in self.reads], out=off[1:])
        flat = np.concatenate(self.reads) if self.reads else np.zeros(0, np.uint8)
        return np.uint32(len(self.reads)).tobytes() + off.tobytes() + flat.tobytes()

    def reference_blob(self, epsilon, min_unitig_size):
        t, h, ln = self.table.arrays()
        seqs = [self.sequence(u) for u in range(self.n_nodes)]
        off = np.zeros(self.n_nodes + 1, np.uint64)
        if seqs:
            np.cumsum([s.shape[0] for s in seqs], out=off[1:])
        return b"".join([np.uint32(self.n_nodes).tobytes(), np.uint64(t.shape[0]).tobytes(), t.tobytes(), h.tobytes(), ln.tobytes(),
                         np.asarray(self.present, np.uint8).tobytes(), np.asarray(self.count, np.uint32).tobytes(),
                         np.asarray(self.coverage, np.uint16).tobytes(), np.asarray(self.is_unitig, np.uint8).tobytes(), off.tobytes(),
                         (np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)).tobytes(),
                         np.uint32(epsilon).tobytes(), np.uint32(min_unitig_size).tobytes()])


def reference(exe, case, epsilon, tmp_path, tag="u", min_unitig_size=9999, ok=(0,)):
    """The restatement on a case: the tables the device fetches, `sequences` (per new node), `alive`, `selected`; None with
    an exit code of `ok` other than 0."""
    b, _ = _run(exe, "unitigs", case.reference_blob(epsilon, min_unitig_size), tmp_path, tag, ok)
    if b is None:
        return None
    r = Reader(b)
    U, M, NE = int(r.one(np.uint32)), int(r.one(np.uint64)), int(r.one(np.uint64))
    E = len(case.table.tail)
    out = dict(begin=r.take(np.uint32, U), end=r.take(np.uint32, U), is_circular=r.take(np.uint8, U), count=r.take(np.uint32, U),
               length=r.take(np.uint32, U), coverage=r.take(np.uint16, U), is_unitig=r.take(np.uint8, U),
               member_offsets=r.take(np.uint64, U + 1), members=r.take(np.uint32, M), marked=r.take(np.uint8, E),
               edge_tail=r.take(np.uint32, NE), edge_head=r.take(np.uint32, NE), edge_length=r.take(np.uint32, NE))
    off = r.take(np.uint64, U + 1)
    bases = r.take(np.uint8, off[-1])
    out["sequences"] = [bases[int(off[j]):int(off[j + 1])] for j in range(U)]
    out["alive"] = r.take(np.uint8, case.n_nodes + U)
    out["selected"] = r.take(np.uint32, r.one(np.uint32))
    assert r.done()
    return out


def member_prefixes(case, want):
    """keep[k] per member of the restatement's tables: the length of the member's out-edge, the whole member at the end of
    a linear unitig (what the sequence rule says, from the edge table alone)."""
    out_edge = {}
    for i, t in enumerate(case.table.tail):
        if t != EMPTY:
            out_edge.setdefault(t, []).append(i)
    keep = []
    off = want["member_offsets"]
    for j in range(want["begin"].shape[0]):
        ms = want["members"][int(off[j]):int(off[j + 1])]
        for k, u in enumerate(ms):
            last = k == len(ms) - 1 and not want["is_circular"][j]
            keep.append(case.length(int(u)) if last else case.table.length[out_edge[int(u)][0]])
    return np.asarray(keep, np.uint32)


def expected_tilings(case, want, keep):
    """The new nodes' segment lists by the prefix rule, restated: a prefix keeps every segment that starts in front of its
    last base; the first L bases of (r, b, l, 0) are (r, b, L, 0), of (r, b, l, 1) are (r, b + l - L, L, 1)."""
    res, k = [], 0
    off = want["member_offsets"]
    for j in range(want["begin"].shape[0]):
        segs = []
        for u in want["members"][int(off[j]):int(off[j + 1])]:
            L, at = int(keep[k]), 0
            k += 1
            for r, b, ln, st in case.tiling[int(u)]:
                if at >= L:
                    break
                take = min(ln, L - at)
                segs.append((r, b + (ln - take) if st else b, take, st))
                at += ln
        res.append(segs)
    return res


def host_words(exe, case, want, keep, tmp_path, tag="w"):
    """The host build of unitig_rules.h on the restatement's member lists: (tilings per new node, packed words, word offsets)."""
    off, rd, bg, ln, st = case.tiling_arrays()
    blob = b"".join([case.reads_blob(), np.uint32(case.n_nodes).tobytes(), off.tobytes(), rd.tobytes(), bg.tobytes(), ln.tobytes(),
                     st.tobytes(), np.uint32(want["begin"].shape[0]).tobytes(), want["member_offsets"].tobytes(),
                     want["members"].tobytes(), keep.tobytes()])
    b, _ = _run(exe, "words", blob, tmp_path, tag)
    r = Reader(b)
    U = want["begin"].shape[0]
    soff = r.take(np.uint64, U + 1)
    S = int(soff[-1])
    cols = [r.take(np.uint32, S) for _ in range(4)]
    woff = r.take(np.uint64, U + 1)
    words = r.take(np.uint64, woff[-1])
    assert r.done()
    tilings = [[tuple(int(c[i]) for c in cols) for i in range(int(soff[j]), int(soff[j + 1]))] for j in range(U)]
    return tilings, words, woff


# ---- builders -----------------------------------------------------------------------------------------------------------

def random_reads(rng, n, lo=200, hi=400):
    return [rng.integers(0, 4, size=int(rng.integers(lo, hi + 1))).astype(np.uint8) for _ in range(n)]


def simple_nodes(case, k, rng=None, count=1, coverage=None):
    """k node pairs, node pair i = the whole of read i (reads must exist); returns the forward ids."""
    ids = []
    for _ in range(k):
        i = case.n_nodes // 2
        cov = int(rng.integers(1, 60000)) if (rng is not None and coverage is None) else (coverage or 0)
        ids.append(case.node([(i, 0, case.reads[i].shape[0], 0)], count=count, coverage=cov))
    return ids


def chain(case, nodes, rng, circular=False):
    """Edges along `nodes` (any strand), lengths at most the tail's (and the pair tail's) length."""
    last = len(nodes) if circular else len(nodes) - 1
    for i in range(last):
        t, h = nodes[i], nodes[(i + 1) % len(nodes)]
        case.join(t, h, int(rng.integers(0, case.length(t) + 1)), int(rng.integers(0, case.length(h ^ 1) + 1)))


def line_case(rng, k, circular=False, flip=None, count=1, read_len=(40, 90)):
    """One chain (or cycle) of k node pairs over k reads; flip[i] puts node i on its reverse strand."""
    case = Case(random_reads(rng, k, *read_len))
    ids = simple_nodes(case, k, rng, count=count)
    if flip is not None:
        ids = [u ^ int(f) for u, f in zip(ids, flip)]
    if k > 1 or circular:
        chain(case, ids, rng, circular)
    return case, ids


SEGMENT_LENGTHS = (0, 1, 31, 32, 33, 64)


def random_segments(rng, reads, max_segments=4):
    segs = []
    for _ in range(int(rng.integers(1, max_segments + 1))):
        r = int(rng.integers(0, len(reads)))
        n = reads[r].shape[0]
        ln = int(rng.choice(SEGMENT_LENGTHS)) if rng.random() < 0.5 else int(rng.integers(0, n + 1))
        ln = min(ln, n)
        segs.append((r, int(rng.integers(0, n - ln + 1)), ln, int(rng.integers(0, 2))))
    return segs


def random_tiled_case(rng, n_chains=12, max_chain=9, n_reads=20):
    """Chains and cycles of nodes with several segments each (lengths 0, 1, 31, 32, 33, 64 and random ones, both strands; a
    node's pair has segments of its own with the same total), on either strand, interleaved in id order, some ending in
    a junction."""
    case = Case(random_reads(rng, n_reads, 60, 140))
    lengths = [int(rng.integers(1, max_chain + 1)) for _ in range(n_chains)]
    pool = []
    for _ in range(sum(lengths)):
        segs = random_segments(rng, case.reads)
        total = sum(s[2] for s in segs)
        rc = None
        if rng.random() < 0.5:  # an unrelated pair sequence of the same length, cut differently
            r = max(range(len(case.reads)), key=lambda i: case.reads[i].shape[0])
            if total <= case.reads[r].shape[0]:
                cut = int(rng.integers(0, total + 1))
                rc = [(r, 0, cut, 1), (r, cut, total - cut, 0)]
        pool.append(case.node(segs, count=int(rng.integers(1, 9)), coverage=int(rng.integers(0, 65536)), rc_segments=rc,
                              rc_count=int(rng.integers(1, 9))))
    rng.shuffle(pool)
    at = 0
    for L in lengths:
        ids = [u ^ int(rng.integers(0, 2)) for u in pool[at:at + L]]
        at += L
        circular = rng.random() < 0.3
        chain(case, ids, rng, circular)
        if not circular and rng.random() < 0.5:  # a junction behind the chain: two more edges leave its last node
            j = case.node(random_segments(rng, case.reads), coverage=7)
            chain(case, [ids[-1], j], rng)
            x = case.node(random_segments(rng, case.reads), coverage=9)
            y = case.node(random_segments(rng, case.reads), coverage=11)
            chain(case, [j, x], rng)
            chain(case, [j, y], rng)
    return case


# ---- the device side ------------------------------------------------------------------------------------------------------

def device_run(engine, case, epsilon, min_unitig_size=9999, reads=None, tiling=None):
    """(reads, tiling, graph, unitigs) of rvn_graph_create_unitigs on a case; reads / tiling of an earlier call are reused."""
    rd = reads if reads is not None else engine.upload_codes(case.reads)
    tl = tiling if tiling is not None else engine.tiling_from_segments(rd, *case.tiling_arrays())
    t, h, ln = case.table.arrays()
    g = engine.graph_from_edges(case.n_nodes, t, h, ln)
    u = g.create_unitigs(tl, case.count, case.coverage, epsilon, min_unitig_size)
    return rd, tl, g, u


def fetched_tilings(tiling, first, count):
    f = tiling.fetch()
    off = f["offsets"]
    return [[(int(f["read"][i]), int(f["begin"][i]), int(f["length"][i]), int(f["strand"][i]))
             for i in range(int(off[u]), int(off[u + 1]))] for u in range(first, first + count)], f["node_length"]


def assert_same_as_reference(case, want, tiling, unitigs):
    """Every table, every new node's tiling and every packed word of the device call equal the restatement's."""
    got = unitigs.fetch()
    U = want["begin"].shape[0]
    assert unitigs.first_node == case.n_nodes and unitigs.first_edge == len(case.table.tail) and unitigs.n_new_nodes == U
    for k in TABLE_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert tiling.n_nodes == case.n_nodes + U
    tilings, node_length = fetched_tilings(tiling, case.n_nodes, U)
    assert tilings == expected_tilings(case, want, member_prefixes(case, want))
    assert np.array_equal(node_length[case.n_nodes:], want["length"])
    assert np.array_equal(node_length[:case.n_nodes], [case.length(u) for u in range(case.n_nodes)])
    if U:
        from raven_amd import hip
        words, woff, lens = unitigs.as_reads(hip.UNITIGS_ALL).fetch()[:3]
        ew, eo = pack_all(want["sequences"])
        assert np.array_equal(lens, want["length"]) and np.array_equal(woff, eo) and np.array_equal(words, ew)
        chosen = [j for j in range(0, U, 2) if want["is_unitig"][j]]
        words, woff, lens = unitigs.as_reads(hip.UNITIGS_SELECTED).fetch()[:3]
        ew, eo = pack_all([want["sequences"][j] for j in chosen])
        assert np.array_equal(lens, want["length"][chosen]) and np.array_equal(woff, eo) and np.array_equal(words, ew)
    return got


def next_round(case, want):
    """The graph after the call, as raven goes on with it: the new nodes (their tilings by the prefix rule) and edges
    appended, the marked edges and the nodes RemoveEdges drops taken out."""
    nxt = Case(case.reads)
    nxt.tiling = [list(t) for t in case.tiling] + expected_tilings(case, want, member_prefixes(case, want))
    nxt.count = list(case.count) + want["count"].tolist()
    nxt.coverage = list(case.coverage) + want["coverage"].tolist()
    nxt.is_unitig = list(case.is_unitig) + want["is_unitig"].tolist()
    nxt.present = want["alive"].tolist()
    t = nxt.table
    t.n_nodes = nxt.n_nodes
    t.tail = [EMPTY if m else x for x, m in zip(case.table.tail, want["marked"])] + want["edge_tail"].tolist()
    t.head = [0 if m else x for x, m in zip(case.table.head, want["marked"])] + want["edge_head"].tolist()
    t.length = [0 if m else x for x, m in zip(case.table.length, want["marked"])] + want["edge_length"].tolist()
    return nxt


def cheap_line_case(rng, k, n_reads=64, circular=False, read_len=(40, 70)):
    """A chain of k node pairs whose nodes share n_reads reads (node i = the whole of read i % n_reads), mixed strands."""
    case = Case(random_reads(rng, n_reads, *read_len))
    lens = [r.shape[0] for r in case.reads]
    flips = rng.integers(0, 2, size=k)
    cov = rng.integers(0, 65536, size=k)
    for i in range(k):
        r = i % n_reads
        case.tiling += [[(r, 0, lens[r], 0)], [(r, 0, lens[r], 1)]]
    case.count = [1] * (2 * k)
    case.coverage = np.repeat(cov, 2).tolist()
    case.present = [1] * (2 * k)
    case.is_unitig = [0] * (2 * k)
    case.table.n_nodes = 2 * k
    ids = [2 * i + int(flips[i]) for i in range(k)]
    cut = rng.integers(0, 40, size=(k, 2))
    for i in range(k if circular else k - 1):
        case.join(ids[i], ids[(i + 1) % k], int(cut[i, 0]), int(cut[i, 1]))
    return case, ids
