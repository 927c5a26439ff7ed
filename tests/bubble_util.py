"""Shared pieces of the RemoveBubbles tests: the restatement (tests/host/bubble_reference.cpp), the host build of the path
rule and of the similarity threshold (tests/host/bubble_rules_host.cpp), their binary formats, path strings in numpy, and
builders of graphs with bubbles whose node sequences are cut from one genome."""
import os
import subprocess

import numpy as np

from tests.graph_util import ROOT, Reader, _run
from tests.unitig_util import Case

ABOVE, BY_LENGTH = 0xFFFFFFFE, 0xFFFFFFFF


def build_reference(tmp_path, sanitize=False):
    exe = str(tmp_path / ("bubble_reference_san" if sanitize else "bubble_reference"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host", "bubble_reference.cpp")])
    return exe


def build_rules_program(tmp_path, sanitize=False):
    exe = str(tmp_path / ("bubble_rules_host_san" if sanitize else "bubble_rules_host"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I",
                           os.path.join(ROOT, "raven_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "bubble_rules_host.cpp")])
    return exe


def reference_blob(case):
    t, h, ln = case.table.arrays()
    seqs = [case.sequence(u) for u in range(case.n_nodes)]
    off = np.zeros(case.n_nodes + 1, np.uint64)
    if seqs:
        np.cumsum([s.shape[0] for s in seqs], out=off[1:])
    return b"".join([np.uint32(case.n_nodes).tobytes(), np.uint64(t.shape[0]).tobytes(), t.tobytes(), h.tobytes(), ln.tobytes(),
                     np.asarray(case.present, np.uint8).tobytes(), np.asarray(case.count, np.uint32).tobytes(), off.tobytes(),
                     (np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)).tobytes()])


def reference(exe, case, tmp_path, tag="b"):
    """The restatement's RemoveBubbles on a case: popped, n_junctions, node_alive, edge_alive, tests (per similarity test
    lhs, lhs_label, rhs, rhs_label, l, r, distance, similar), seconds (the loop's own time)."""
    b, p = _run(exe, "bubbles", reference_blob(case), tmp_path, tag)
    r = Reader(b)
    out = dict(popped=int(r.one(np.uint32)), n_junctions=int(r.one(np.uint32)))
    out["node_alive"] = r.take(np.uint8, case.n_nodes)
    out["edge_alive"] = r.take(np.uint8, len(case.table.tail))
    out["tests"] = []
    for _ in range(int(r.one(np.uint32))):
        t = {}
        for side in ("lhs", "rhs"):
            k = int(r.one(np.uint32))
            t[side] = r.take(np.uint32, k)
            t[side + "_label"] = r.take(np.uint32, k)
        t["l"], t["r"] = int(r.one(np.uint64)), int(r.one(np.uint64))
        t["distance"], t["similar"] = int(r.one(np.uint32)), int(r.one(np.uint8))
        out["tests"].append(t)
    assert r.done()
    out["seconds"] = float(p.stderr.split()[1]) if p.stderr.startswith("bubbles ") else None
    return out


def distances(exe, pairs, tmp_path, tag="d"):
    """The restatement's edit distance of every (a, b) of code arrays."""
    parts = [np.uint32(len(pairs)).tobytes()]
    for a, b in pairs:
        a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
        parts += [np.uint64(a.shape[0]).tobytes(), np.uint64(b.shape[0]).tobytes(), a.tobytes(), b.tobytes()]
    out, _ = _run(exe, "distance", b"".join(parts), tmp_path, tag)
    return np.frombuffer(out, np.uint32).copy()


def path_string(case, nodes, labels):
    """Per member but the last the first min(label, length) bases of the node, then the whole last node."""
    parts = [np.zeros(0, np.uint8)]
    for i, u in enumerate(nodes):
        s = case.sequence(int(u))
        parts.append(s if i == len(nodes) - 1 else s[:min(int(labels[i]), s.shape[0])])
    return np.concatenate(parts)


def flatten(paths):
    """[(nodes, labels)] -> (offsets, nodes, labels) as rvn_tiling_paths_as_reads takes them."""
    off = np.zeros(len(paths) + 1, np.uint64)
    if paths:
        np.cumsum([len(p[0]) for p in paths], out=off[1:])
    cat = lambda k, dt: np.concatenate([np.asarray(p[k], dt) for p in paths]) if paths else np.zeros(0, dt)
    return off, cat(0, np.uint32), cat(1, np.uint32)


def host_paths(exe, case, paths, tmp_path, tag="p"):
    """The host build of the path rule: (lengths, word offsets, words)."""
    soff, rd, bg, ln, st = case.tiling_arrays()
    off, nd, lb = flatten(paths)
    blob = b"".join([case.reads_blob(), np.uint32(case.n_nodes).tobytes(), soff.tobytes(), rd.tobytes(), bg.tobytes(), ln.tobytes(),
                     st.tobytes(), np.uint32(len(paths)).tobytes(), off.tobytes(), nd.tobytes(), lb.tobytes()])
    b, _ = _run(exe, "paths", blob, tmp_path, tag)
    r = Reader(b)
    lens = r.take(np.uint32, len(paths))
    woff = r.take(np.uint64, len(paths) + 1)
    words = r.take(np.uint64, woff[-1])
    assert r.done()
    return lens, woff, words


def host_kmax(exe, maxlen, ratio, tmp_path, tag="k"):
    m = np.asarray(maxlen, np.uint32)
    b, _ = _run(exe, "kmax", np.uint32(m.shape[0]).tobytes() + np.float64(ratio).tobytes() + m.tobytes(), tmp_path, tag)
    return np.frombuffer(b, np.uint32).copy()


def kmax(mx, ratio):
    """The largest x with !(1 - x / mx < ratio), by the rule itself."""
    keeps = lambda x: not (1.0 - float(x) / float(mx) < ratio)
    t = int(max(0.0, min(float(mx), (1.0 - ratio) * mx)))
    while t < mx and keeps(t + 1):
        t += 1
    while t > 0 and not keeps(t):
        t -= 1
    return t


def plant(rng, seq, k):
    """k substitutions at distinct positions: an upper bound of k on the distance."""
    out = np.array(seq, np.uint8)
    at = rng.choice(out.shape[0], size=k, replace=False)
    out[at] = (out[at] + rng.integers(1, 4, size=k).astype(np.uint8)) & 3
    return out


# ---- graphs whose nodes lie on one genome ---------------------------------------------------------------------------------

class GenomeGraph:
    """Nodes are windows of a random genome (each its own read, some with substitutions); an edge t -> h is as long as the
    distance between the two windows' starts, its pair as the distance between their ends.  Every path between two nodes
    then spells the same stretch of the genome, up to the substitutions."""

    def __init__(self, rng, genome_len):
        self.rng = rng
        self.genome = rng.integers(0, 4, size=genome_len).astype(np.uint8)
        self.case = Case([])
        self.pos = {}

    def node(self, at, length, subs=0, count=1, unrelated=False):
        s = self.genome[at:at + length]
        if unrelated:
            s = self.rng.integers(0, 4, size=length).astype(np.uint8)
        elif subs:
            s = plant(self.rng, s, subs)
        self.case.reads.append(np.asarray(s, np.uint8))
        u = self.case.node([(len(self.case.reads) - 1, 0, length, 0)], count=count)
        self.pos[u] = (at, at + length)
        return u

    def join(self, t, h, length=None, length_pair=None):
        a = self.pos[h][0] - self.pos[t][0] if length is None else length
        b = self.pos[h][1] - self.pos[t][1] if length_pair is None else length_pair
        return self.case.join(t, h, a, b)


def diamond(seed=1, b_subs=0, count_a=1, b_unrelated=False, inner=100, outer=100):
    """B -> a -> E, B -> b -> E: ids B = 0, a = 2, b = 4, E = 6; edges B->a 0, B->b 2, a->E 4, b->E 6."""
    g = GenomeGraph(np.random.default_rng(seed), 2 * outer + inner + 200)
    B = g.node(0, outer)
    a = g.node(outer, inner, count=count_a)
    b = g.node(outer, inner, subs=b_subs, unrelated=b_unrelated)
    E = g.node(outer + inner, outer)
    g.join(B, a)
    g.join(B, b)
    g.join(a, E)
    return g, (B, a, b, E)


def shared_node():
    """B -> a -> {c, d} -> E and a dead end B -> z: from B both paths run through a (nothing to do); from a the bubble is
    plain.  Ids B = 0, a = 2, c = 4, d = 6, E = 8, z = 10; edges in the order (B, a), (B, z), (a, c), (a, d), (c, E), (d, E)."""
    g = GenomeGraph(np.random.default_rng(2), 800)
    B, a, c, dd, E, z = g.node(0, 100), g.node(100, 100), g.node(200, 100), g.node(200, 100), g.node(300, 100), g.node(100, 100)
    for t, h in ((B, a), (B, z), (a, c), (a, dd), (c, E), (dd, E)):
        g.join(t, h)
    return g


def node_with_its_pair():
    """B -> a -> E and B -> a' -> E: a has two out-edges (E and B'), which would make the bubble complex, but the two paths
    the search finds hold a node together with its pair."""
    g = GenomeGraph(np.random.default_rng(3), 800)
    B, a, E = g.node(0, 100), g.node(100, 100), g.node(200, 100)
    g.join(B, a)
    g.join(B, a ^ 1, 100, 100)
    g.join(a, E)
    g.join(a ^ 1, E, 100, 100)
    return g


def at_the_reach(last):
    """B -> a of 499 990 bases, a -> E of `last`, beside B -> b -> E of 100 each: E is 499 990 + last bases away through a.
    The pair of B -> a is as long, so the paired bubble is out of reach either way."""
    g = GenomeGraph(np.random.default_rng(4), 600)
    B, a, b, E = g.node(0, 100), g.node(100, 100), g.node(100, 100), g.node(200, 100)
    g.join(B, a, 499_990, 499_990)
    g.join(B, b)
    g.join(a, E, last, 100)
    g.join(b, E)
    return g


def chain_with_bubbles(rng, n_bubbles=30, node_len=300, step=100, arm=600):
    """A chain along a genome with a bubble every few nodes: plain ones (two single-node arms), complex ones (an arm's node
    has a second out-edge to a dead end, or a second in-edge from one) whose arms are similar (a few substitutions),
    dissimilar (an unrelated arm: about 300 edits in 1 000 bases) or of very different length.  Returns the GenomeGraph."""
    g = GenomeGraph(rng, (3 * step + arm) * n_bubbles + node_len + 4000)
    at = 0
    prev = g.node(at, node_len)
    for i in range(n_bubbles):
        kind = i % 5
        for _ in range(int(rng.integers(1, 3))):  # the chain between two bubbles
            at += step
            nxt = g.node(at, node_len)
            g.join(prev, nxt)
            prev = nxt
        begin = prev
        end = g.node(at + step + arm, node_len)
        a = g.node(at + step, arm, count=int(rng.integers(1, 4)))
        b = g.node(at + step, arm, subs=0 if kind == 0 else 7, count=int(rng.integers(1, 4)), unrelated=kind == 3)
        g.join(begin, a)
        g.join(begin, b)
        g.join(a, end)
        if kind == 4:  # the arm through b spells far fewer bases
            g.join(b, end, 3, 3)
        else:
            g.join(b, end)
        if kind in (1, 3, 4):  # a dead end behind b: b has two out-edges, the bubble is complex
            g.join(b, g.node(at + step + arm, node_len, unrelated=True))
        if kind == 2:  # a second way into a
            g.join(g.node(at, node_len, unrelated=True), a)
        at += step + arm
        prev = end
    return g


def forced_miss(rng):
    """Two junctions I < J: J -> I, J -> z -> w -> F, I -> a -> E, I -> b -> E, E -> F, y -> I.  From J the search first
    meets the inner bubble, whose two paths share I (nothing to do, nothing to ask for); once I's own bubble is popped it
    goes on to F, and the paths it finds then (I has a second in-edge: complex) were in nobody's prediction."""
    g = GenomeGraph(rng, 1200)
    I = g.node(100, 100)
    J = g.node(0, 100)
    z = g.node(100, 200, subs=2)
    w = g.node(300, 100, subs=1)
    a = g.node(200, 100)
    b = g.node(200, 100, count=2)
    E = g.node(300, 100)
    F = g.node(400, 100)
    y = g.node(0, 100, unrelated=True)
    g.join(J, I)
    g.join(J, z)
    g.join(I, a)
    g.join(I, b)
    g.join(z, w)
    g.join(a, E)
    g.join(b, E)
    g.join(w, F)
    g.join(E, F)
    g.join(y, I)
    return g, dict(I=I, J=J, z=z, w=w, a=a, b=b, E=E, F=F, y=y)


def random_paths(rng, case, n):
    """Paths of 1 .. 6 nodes of a case, any nodes (a path needs no edges to have a string), labels around the node's
    length: 0, 1, length - 1, length, length + 1, 2^32 - 16 and random ones."""
    paths = []
    for _ in range(n):
        nodes = rng.integers(0, case.n_nodes, size=int(rng.integers(1, 7)))
        labels = []
        for u in nodes:
            L = case.length(int(u))
            labels.append(int(rng.choice([0, 1, max(L - 1, 0), L, L + 1, 0xFFFFFFF0, int(rng.integers(0, L + 1))])))
        paths.append((nodes.astype(np.uint32), np.asarray(labels, np.uint32)))
    return paths
