"""Shared pieces of the assembly-graph tests: the restatement (tests/host/graph_reference.cpp, g++ with the oracle's
GetOverlapType), the host build of graph_rules.h (tests/host/graph_rules_host.cpp), their binary input / output format
(the convention of tests/repeats_util.py), and builders of edge tables."""
import os
import subprocess

import numpy as np

from raven_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = 0xFFFFFFFF  # tail of an empty edge slot


def build_reference(tmp_path):
    exe = str(tmp_path / "graph_reference")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "oracle"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "graph_reference.cpp"),
                           os.path.join(ROOT, "oracle", "poa_oracle.cpp")])
    return exe


def build_rules_program(tmp_path):
    exe = str(tmp_path / "graph_rules_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I",
                           os.path.join(ROOT, "raven_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "graph_rules_host.cpp")])
    return exe


def _run(exe, mode, blob, tmp_path, tag, ok=(0,)):
    src, dst = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".out"))
    with open(src, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, mode, src, dst], capture_output=True, text=True)
    assert p.returncode in ok, (p.returncode, p.stderr)
    return (open(dst, "rb").read() if p.returncode == 0 else None), p


class Reader:
    def __init__(self, b):
        self.b, self.pos = b, 0

    def take(self, dtype, count):
        a = np.frombuffer(self.b, dtype, int(count), self.pos).copy()
        self.pos += a.nbytes
        return a

    def one(self, dtype):
        return self.take(dtype, 1)[0]

    def done(self):
        return self.pos == len(self.b)


def _marks(r):
    order = r.take(np.uint32, r.one(np.uint64))
    pairs = r.take(np.uint32, 2 * int(r.one(np.uint64))).reshape(-1, 2)
    return order, pairs


class EdgeTable:
    """Flattened graph.edges: edge 2j and 2j + 1 are a pair, tail EMPTY = no edge in the slot."""

    def __init__(self, n_nodes=0):
        self.n_nodes = n_nodes
        self.tail, self.head, self.length = [], [], []

    def nodes(self, k):
        """k more node pairs; returns the ids of their forward nodes."""
        first = self.n_nodes
        self.n_nodes += 2 * k
        return list(range(first, first + 2 * k, 2))

    def join(self, t, h, length, length_pair=None):
        """t -> h and its pair h ^ 1 -> t ^ 1; returns the id of t -> h."""
        self.tail += [t, h ^ 1]
        self.head += [h, t ^ 1]
        self.length += [length & 0xFFFFFFFF, (length if length_pair is None else length_pair) & 0xFFFFFFFF]
        return len(self.tail) - 2

    def hole(self):
        self.tail += [EMPTY, EMPTY]
        self.head += [0, 0]
        self.length += [0, 0]

    def arrays(self):
        return (np.asarray(self.tail, np.uint32), np.asarray(self.head, np.uint32), np.asarray(self.length, np.uint32))

    def blob(self, weight=None):
        t, h, ln = self.arrays()
        b = np.uint32(self.n_nodes).tobytes() + np.uint64(t.shape[0]).tobytes() + t.tobytes() + h.tobytes() + ln.tobytes()
        if weight is None:
            return b + np.uint8(0).tobytes()
        return b + np.uint8(1).tobytes() + np.asarray(weight, np.float64).tobytes()


def reference_marks(exe, table, tmp_path, tag="g", weight=None):
    """The restatement on an edge table: dict(order, pairs[, long, n_long])."""
    b, _ = _run(exe, "graph", table.blob(weight), tmp_path, tag)
    r = Reader(b)
    order, pairs = _marks(r)
    out = dict(order=order, pairs=pairs)
    if weight is not None:
        out["long"] = r.take(np.uint8, len(table.tail))
        out["n_long"] = int(r.one(np.uint64))
    assert r.done()
    return out


def comparable(exe, triples, tmp_path, tag="c"):
    """verdict per (len_j, len_k, len_c), from the restatement's triangles or from the host build of graph_rules.h."""
    t = np.ascontiguousarray(triples, dtype=np.uint32).reshape(-1, 3)
    b, _ = _run(exe, "comparable", np.uint64(t.shape[0]).tobytes() + t.tobytes(), tmp_path, tag)
    return np.frombuffer(b, np.uint8).copy()


def long_rule(exe, pairs, tmp_path, tag="l"):
    w = np.ascontiguousarray(pairs, dtype=np.float64).reshape(-1, 2)
    b, _ = _run(exe, "long", np.uint64(w.shape[0]).tobytes() + w.tobytes(), tmp_path, tag)
    return np.frombuffer(b, np.uint8).copy()


class ConstructInput:
    """The arguments of rvn_construct_assembly_graph."""

    def __init__(self, overlaps, begin, end, median, invalid):
        self.overlaps = np.ascontiguousarray(overlaps, dtype=hip.OVERLAP_DTYPE)
        self.begin = np.asarray(begin, np.uint32)
        self.end = np.asarray(end, np.uint32)
        self.median = np.asarray(median, np.uint16)
        self.invalid = np.asarray(invalid, np.uint8)
        self.n = self.begin.shape[0]

    def blob(self):
        return b"".join([np.uint32(self.n).tobytes(), np.uint64(self.overlaps.shape[0]).tobytes()] +
                        [np.ascontiguousarray(a).tobytes() for a in (self.overlaps, self.begin, self.end, self.median, self.invalid)])

    def device(self, engine):
        return engine.construct_assembly_graph(self.overlaps, self.begin, self.end, self.median, self.invalid)


CONSTRUCT_KEYS = ("sequence_to_node", "node_pile", "node_coverage", "tail", "head", "length", "edge_overlap", "finalized")


def run_construct(exe, inp, tmp_path, tag="k", marks=True, ok=(0,)):
    """`construct` of the restatement (marks=True: with the MARKS of the graph) or of the host build of graph_rules.h:
    the dict Graph.fetch() returns (+ order, pairs), or None with an exit code of `ok` other than 0; and the stderr."""
    b, p = _run(exe, "construct", inp.blob(), tmp_path, tag, ok)
    if b is None:
        return None, p.stderr
    r = Reader(b)
    nn, ne = int(r.one(np.uint32)), int(r.one(np.uint64))
    out = dict(n_nodes=nn, n_edges=ne)
    out["sequence_to_node"] = r.take(np.int32, inp.n)
    out["node_pile"] = r.take(np.uint32, nn)
    out["node_coverage"] = r.take(np.uint16, nn)
    for k in ("tail", "head", "length"):
        out[k] = r.take(np.uint32, ne)
    out["edge_overlap"] = r.take(np.uint64, ne // 2)
    out["finalized"] = r.take(hip.OVERLAP_DTYPE, ne // 2)
    if marks:
        out["order"], out["pairs"] = _marks(r)
    assert r.done()
    return out, p.stderr


def assert_same_tables(got, want):
    for k in CONSTRUCT_KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def assert_same_marks(order, pairs, want):
    """the insertion-ordered ids and the transitive pairs, as sequences"""
    assert order.shape == want["order"].shape and np.array_equal(order, want["order"])
    assert pairs.shape == want["pairs"].shape and np.array_equal(pairs, want["pairs"])


def band(m):
    """a -> c of length 25 m: the lengths 22 m and 28 m are exactly 0.88 and 1.12 of it"""
    return 25 * m, 22 * m, 28 * m


def random_table(rng, n, max_degree=300):
    """2 n nodes on a line with heavy-tailed out-degrees (1 .. max_degree), mostly forward edges to near neighbours on
    the forward strand, some anywhere on either strand, parallel edges, self-loops and empty slots.  An edge is as long
    as the distance it spans times a factor in 0.85 .. 1.18, so that a two-step walk is often, not always, within 12 % of
    the direct edge."""
    t = EdgeTable(2 * n)
    pos = np.sort(rng.integers(0, 20_000 * n, size=n))
    deg = np.minimum((rng.pareto(1.2, size=n) * 2).astype(np.int64) + 1, min(max_degree, 4 * n))
    for a in range(n):
        for _ in range(int(deg[a])):
            if rng.random() < 0.1:
                b, sa, sb = int(rng.integers(0, n)), int(rng.integers(0, 2)), int(rng.integers(0, 2))
            else:
                b, sa, sb = min(n - 1, a + int(rng.integers(1, 9))), 0, 0
            d = abs(int(pos[b]) - int(pos[a])) + 1
            t.join(2 * a + sa, 2 * b + sb, int(d * rng.uniform(0.85, 1.18)) + 1, int(d * rng.uniform(0.85, 1.18)) + 1)
            if rng.random() < 0.03:
                t.hole()
    return t


def is_comparable(a, b):
    eps = 0.12
    return (a >= b * (1 - eps) and a <= b * (1 + eps)) or (b >= a * (1 - eps) and b <= a * (1 + eps))


def triangle_counts(table):
    """(two-step walks v -> x -> y that have a direct edge v -> y, those of them that are comparable): what the tests
    assert of the inputs they draw, counted apart from the programs under test."""
    out = {}
    for i, (tl, hd) in enumerate(zip(table.tail, table.head)):
        if tl != EMPTY:
            out.setdefault(tl, []).append(i)
    triangles = comparable_ = 0
    M = 0xFFFFFFFF
    for v, edges in out.items():
        cand = {table.head[j]: j for j in edges}
        for j in edges:
            for k in out.get(table.head[j], ()):
                c = cand.get(table.head[k])
                if c is not None:
                    triangles += 1
                    comparable_ += is_comparable(float((table.length[j] + table.length[k]) & M), float(table.length[c]))
    return triangles, comparable_


def fan(t, rng, d, max_r):
    """A node v with d out-edges to d fresh heads; head i has 1 .. max_r out-edges to other heads (and to itself), as
    long as makes v -> head -> target compare with v -> target about half of the time (a negative difference wraps, and
    the sum wraps back).  Returns v."""
    v = t.nodes(1)[0]
    heads = t.nodes(d)
    lv = [10_000 + 37 * i for i in range(d)]
    for i in range(d):
        t.join(v, heads[i], lv[i], 3)
    for i in range(d):
        for k in range(int(rng.integers(1, max_r + 1))):
            g = (i * 7 + k * 13) % d
            t.join(heads[i], heads[g], int(lv[g] * rng.uniform(0.8, 1.25)) - lv[i], 5)
    return v


def overlap_type(o, begin, end):
    """GetOverlapType (overlap_utils.cc:82-113) in 32-bit unsigned arithmetic: only to keep generated inputs off the
    combination the entry point rejects (an edge on an invalid pile)."""
    M = 0xFFFFFFFF
    lb0, rb0 = int(begin[o["lhs_id"]]), int(begin[o["rhs_id"]])
    ll, rl = (int(end[o["lhs_id"]]) - lb0) & M, (int(end[o["rhs_id"]]) - rb0) & M
    lb, le = (int(o["lhs_begin"]) - lb0) & M, (int(o["lhs_end"]) - lb0) & M
    if o["strand"]:
        rb, re = (int(o["rhs_begin"]) - rb0) & M, (int(o["rhs_end"]) - rb0) & M
    else:
        rb, re = (rl - ((int(o["rhs_end"]) - rb0) & M)) & M, (rl - ((int(o["rhs_begin"]) - rb0) & M)) & M
    lr, rr = (ll - le) & M, (rl - re) & M
    overhang = (min(lb, rb) + min(lr, rr)) & M
    ls, rs = (le - lb) & M, (re - rb) & M
    if ls < ((ls + overhang) & M) * 0.875 or rs < ((rs + overhang) & M) * 0.875:
        return 0
    if lb <= rb and lr <= rr:
        return 1
    if rb <= lb and rr <= lr:
        return 2
    return 3 if lb > rb else 4


def random_overlaps(rng, n_piles, m, invalid_share=0.2, finalize_on_invalid=False):
    """m overlaps of every type on both strands over n_piles piles with valid regions inside reads of 2 - 30 kb, a share
    of the piles invalid and some valid regions of length zero.  Unless finalize_on_invalid, overlaps that would make
    an edge on an invalid pile are moved to valid piles."""
    length = rng.integers(2000, 30000, size=n_piles)
    begin = (rng.integers(0, 300, size=n_piles) * (rng.random(n_piles) < 0.5)).astype(np.uint32)
    end = (length - rng.integers(0, 300, size=n_piles) * (rng.random(n_piles) < 0.5)).astype(np.uint32)
    zero = rng.random(n_piles) < 0.03  # zero-length valid regions, valid or not
    end[zero] = begin[zero]
    invalid = (rng.random(n_piles) < invalid_share).astype(np.uint8)
    if not finalize_on_invalid:
        invalid[0] = 0
    median = rng.integers(1, 200, size=n_piles).astype(np.uint16)
    valid_ids = np.flatnonzero(invalid == 0)
    o = np.zeros(m, dtype=hip.OVERLAP_DTYPE)
    for i in range(m):
        if finalize_on_invalid or rng.random() < 0.15:
            a, b = int(rng.integers(0, n_piles)), int(rng.integers(0, n_piles))
        else:
            a, b = int(rng.choice(valid_ids)), int(rng.choice(valid_ids))
        la, lb = int(end[a] - begin[a]), int(end[b] - begin[b])
        strand = int(rng.integers(0, 2))
        kind = int(rng.integers(0, 5))
        span = int(rng.integers(100, max(101, min(la, lb) // 2 + 101)))
        span_a, span_b = min(span, la), min(span, lb)
        if kind == 0:  # internal
            ab = int(rng.integers(0, max(1, la - span_a + 1)))
            bb = int(rng.integers(0, max(1, lb - span_b + 1)))
        elif kind == 1:  # the whole of a inside b
            ab, span_a = 0, la
            span_b = min(lb, la)
            bb = int(rng.integers(0, max(1, lb - span_b + 1)))
        elif kind == 2:  # the whole of b inside a
            bb, span_b = 0, lb
            span_a = min(la, lb)
            ab = int(rng.integers(0, max(1, la - span_a + 1)))
        elif kind == 3:  # suffix of a, prefix of b (in a's orientation)
            ab, bb = la - span_a, 0
        else:  # prefix of a, suffix of b
            ab, bb = 0, lb - span_b
        if kind >= 3 and not strand:  # rhs coordinates are mirrored on the opposite strand
            bb = lb - span_b - bb
        jit = lambda: int(rng.integers(0, 40)) if rng.random() < 0.5 else 0
        o[i] = (a, int(begin[a]) + max(0, ab + jit()), int(begin[a]) + max(1, ab + span_a - jit()),
                b, int(begin[b]) + max(0, bb + jit()), int(begin[b]) + max(1, bb + span_b - jit()), 0, strand)
    if not finalize_on_invalid:
        keep = [i for i in range(m) if not ((invalid[o[i]["lhs_id"]] or invalid[o[i]["rhs_id"]]) and
                                            overlap_type(o[i], begin, end) >= 3)]
        o = o[keep]
    return ConstructInput(o, begin, end, median, invalid)


def tiled_overlaps(n_reads, read_len=10000, step=1000, reach=5):
    """Error-free reads every `step` bases of a line, every tenth pile invalid and left out; each read overlaps the next
    `reach`, every other overlap listed from the far read's side (type 4).  i -> i + 2 is as long as i -> i + 1 -> i + 2:
    transitive edges by construction."""
    invalid = (np.arange(n_reads) % 10 == 7).astype(np.uint8)
    ids = np.flatnonzero(invalid == 0)
    o = []
    for r, a in enumerate(ids):
        for d in range(1, reach + 1):
            if r + d >= ids.shape[0]:
                break
            b = int(ids[r + d])
            if (r + d) % 2:
                o.append((int(a), step * d, read_len, b, 0, read_len - step * d, 0, 1))
            else:
                o.append((b, 0, read_len - step * d, int(a), step * d, read_len, 0, 1))
    return ConstructInput(np.array(o, dtype=hip.OVERLAP_DTYPE), np.zeros(n_reads, np.uint32), np.full(n_reads, read_len, np.uint32),
                          np.full(n_reads, 30, np.uint16), invalid)
