"""Shared pieces of the force-directed layout tests: the yardstick (tests/host/layout_reference.cpp: the reference's loop
restated, g++ without contraction), the host build of raven_amd/csrc/layout.h (tests/host/layout_host.cpp), their case
file, and the generator of chain graphs with random chords and transitive neighbours."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["g++", "-std=c++17", "-O2", "-ffp-contract=off"]


def build_reference(tmp_path):
    exe = str(tmp_path / "layout_reference")
    subprocess.check_call(FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "host", "layout_reference.cpp")])
    return exe


def build_host_program(tmp_path, sanitize=False):
    exe = str(tmp_path / ("layout_host_san" if sanitize else "layout_host"))
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(FLAGS + extra + ["-I", os.path.join(ROOT, "raven_amd", "csrc"), "-o", exe,
                                           os.path.join(ROOT, "tests", "host", "layout_host.cpp")])
    return exe


class Case:
    """The arguments of rvn_layout_force_directed."""

    def __init__(self, off, xy, adj_off, adj, n_iterations=100):
        self.off = np.ascontiguousarray(off, dtype=np.uint32)
        self.xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self.adj_off = np.ascontiguousarray(adj_off, dtype=np.uint64)
        self.adj = np.ascontiguousarray(adj, dtype=np.uint32)
        self.n_iterations = n_iterations
        assert self.xy.shape[0] == int(self.off[-1]) and self.adj_off.shape[0] == self.xy.shape[0] + 1
        assert self.adj.shape[0] == int(self.adj_off[-1])

    @property
    def n(self):
        return self.xy.shape[0]

    def write(self, path, snapshots):
        with open(path, "wb") as f:
            f.write(np.array([self.off.shape[0] - 1, self.n, self.n_iterations, len(snapshots)], np.uint32).tobytes())
            f.write(np.uint64(self.adj.shape[0]).tobytes())
            for a in (self.off, self.xy, self.adj_off, self.adj, np.asarray(snapshots, np.uint32)):
                f.write(np.ascontiguousarray(a).tobytes())

    def device(self, engine, n_iterations=None):
        return engine.layout_force_directed(self.off, self.xy, self.adj_off, self.adj,
                                            self.n_iterations if n_iterations is None else n_iterations)

    def component(self, c):
        """Component c as a case of its own."""
        b, e = int(self.off[c]), int(self.off[c + 1])
        a0, a1 = int(self.adj_off[b]), int(self.adj_off[e])
        return Case([0, e - b], self.xy[b:e], self.adj_off[b:e + 1] - np.uint64(a0), self.adj[a0:a1] - np.uint32(b),
                    self.n_iterations)

    def permuted(self, perm):
        """The same single component with point i moved to position perm[i]: positions and adjacency move along."""
        assert self.off.shape[0] == 2
        perm = np.asarray(perm)
        inv = np.empty_like(perm)
        inv[perm] = np.arange(self.n)
        lists = [perm[self.adj[int(self.adj_off[i]):int(self.adj_off[i + 1])]] for i in inv]
        return Case(self.off, self.xy[inv], offsets(lists), np.concatenate(lists + [np.zeros(0, np.int64)]), self.n_iterations)


def offsets(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return off


def join(cases):
    """Several cases as the components of one."""
    off, xy, lists_off, adj = [0], [], [np.zeros(1, np.uint64)], []
    for c in cases:
        base, abase = off[-1], lists_off[-1][-1]
        off += [base + int(o) for o in c.off[1:]]
        xy.append(c.xy)
        lists_off.append(c.adj_off[1:] + abase)
        adj.append(c.adj + np.uint32(base))
    return Case(off, np.concatenate(xy), np.concatenate(lists_off), np.concatenate(adj), cases[0].n_iterations)


def chain_with_chords(rng, m, chords=0.1, transitive=0.05):
    """Neighbour lists of one component of m points: a chain, chords between random pairs, some transitive
    neighbours — per point in the reference's order: in-edges, out-edges, transitive."""
    ins, outs, trans = [[] for _ in range(m)], [[] for _ in range(m)], [[] for _ in range(m)]
    edges = [(i, i + 1) for i in range(m - 1)]
    edges += [tuple(rng.integers(0, m, 2)) for _ in range(int(chords * m) + 1)]
    for a, b in edges:
        outs[int(a)].append(int(b))
        ins[int(b)].append(int(a))
    for _ in range(int(transitive * m) + 1):
        a, b = rng.integers(0, m, 2)
        trans[int(a)].append(int(b))
    return [np.array(ins[i] + outs[i] + trans[i], dtype=np.int64) for i in range(m)]


def random_case(rng, sizes, n_iterations=100):
    """Components of the given sizes, start positions uniform in [0, 1) as the reference draws them."""
    cases = []
    for m in sizes:
        lists = chain_with_chords(rng, m)
        cases.append(Case([0, m], rng.random((m, 2)), offsets(lists), np.concatenate(lists), n_iterations))
    return join(cases)


def explicit_case(xy, edges, n_iterations):
    """One component from positions and undirected edges (each end lists the other)."""
    m = len(xy)
    lists = [[] for _ in range(m)]
    for a, b in edges:
        lists[a].append(b)
        lists[b].append(a)
    lists = [np.array(x, dtype=np.int64) for x in lists]
    return Case([0, m], np.array(xy, dtype=np.float64), offsets(lists), np.concatenate(lists + [np.zeros(0, np.int64)]),
                n_iterations)


def run_program(exe, case, tmp_path, snapshots=None, tag="x", host_stats=False):
    """Positions after each snapshot (default: the last iteration) as float64[len(snapshots), n, 2]; with host_stats
    also layout_host's flagged iterations per component and deepest tree."""
    snapshots = [case.n_iterations] if snapshots is None else snapshots
    src, dst = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".out"))
    case.write(src, snapshots)
    p = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    b = open(dst, "rb").read()
    k = len(snapshots) * case.n * 2
    pos = np.frombuffer(b, np.float64, k, 0).reshape(len(snapshots), case.n, 2).copy()
    if not host_stats:
        assert len(b) == 8 * k
        return pos
    n_comp = case.off.shape[0] - 1
    flagged = np.frombuffer(b, np.uint64, n_comp, 8 * k).copy()
    depth = int(np.frombuffer(b, np.uint32, 1, 8 * k + 8 * n_comp)[0])
    assert len(b) == 8 * k + 8 * n_comp + 4
    return pos, flagged, depth


def same_doubles(a, b):
    """== on the doubles (a signed zero may differ), no NaN on either side."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and not np.isnan(a).any() and bool((a == b).all())


# Crafted geometry.  With the origin and (1, 1) in a component its root cell is nucleus (0.5, 0.5), width 0.5 + 0.01: the
# point (0.5, 0.5) sits on the root's nucleus, i.e. on a corner of all four children, and the points with one coordinate
# 0.5 on the boundary between two of them ((0.5 + w) - w == 0.5 for w = 0.51 / 2: the first child that accepts wins).
def crafted_cases(n_iterations=3):
    grid = [(0.0, 0.0), (1.0, 1.0), (0.5, 0.5), (0.5, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 0.5), (0.5, 1.0), (1.0, 0.5),
            (0.0, 0.5), (0.5, 0.0), (0.125, 0.875)]
    ring = [(i, (i + 1) % len(grid)) for i in range(len(grid))] + [(2, 7), (2, 9)]
    line = [(0.03125 * i, 0.0) for i in range(1, 20)]
    diag = [(0.05 * i, 0.05 * i) for i in range(12)]
    close = [(0.3, 0.3), (0.3005, 0.3001), (0.302, 0.299), (0.7, 0.2), (0.1, 0.9), (0.9, 0.9), (0.6, 0.6001)]
    chain = lambda pts: [(i, i + 1) for i in range(len(pts) - 1)]
    return {
        "boundaries_and_nucleus": explicit_case(grid, ring, n_iterations),
        "on_one_line": explicit_case(line, chain(line) + [(0, 10), (3, 18)], n_iterations),
        "on_the_diagonal": explicit_case(diag, chain(diag) + [(0, 11)], n_iterations),
        "neighbours_closer_than_0.01": explicit_case(close, chain(close) + [(0, 2), (0, 6)], n_iterations),
    }


DUPLICATES_SWAP = np.array([0, 2, 1, 3, 4, 5, 6])


def exceptional_cases(n_iterations=2):
    """Geometry whose reference tree depends on the insertion order: exact duplicates in the orders c, c, p and
    c, p, c, two points 1e-13 apart (their paths part below the 32nd subdivision), and a point that no child accepts:
    h = 0.5 + 0.51 / 2 is the nucleus coordinate of the root's first child when the origin and (1, 1) span the box, and
    with q = 0.51 / 4 both (h + q) - q > h and (h - q) + q < h in doubles, so (h, h) falls between that cell's children."""
    h, q = 0.5 + (0.5 + 0.01) / 2, (0.5 + 0.01) / 4
    assert (h + q) - q > h and (h - q) + q < h
    gap = [(0.0, 0.0), (1.0, 1.0), (h, h), (0.9, 0.7), (0.2, 0.3), (0.6, 0.1), (0.3, 0.8)]
    c, p = (0.4, 0.6), (0.7, 0.2)
    rest = [(0.1, 0.1), (0.9, 0.8), (0.2, 0.7), (0.55, 0.35)]
    ccp = explicit_case([c, c, p] + rest, [(i, i + 1) for i in range(6)] + [(0, 4)], n_iterations)
    near = [(0.4, 0.6), (0.4 + 1e-13, 0.6), p] + rest
    edges = [(i, i + 1) for i in range(6)] + [(0, 4)]
    return {
        "duplicates_c_c_p": ccp,
        "duplicates_c_p_c": ccp.permuted(DUPLICATES_SWAP),  # the same graph, the second c listed after p
        "two_points_1e-13_apart": explicit_case(near, edges, n_iterations),
        "point_no_child_accepts": explicit_case(gap, edges, n_iterations),
    }
