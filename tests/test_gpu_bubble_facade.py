"""raven::RemoveBubbles of include/raven_hip/bubbles.hpp (tests/cpp/bubble_facade_test.cpp, g++ against doubles whose node
sequence counts its accesses) against the restatement (tests/host/bubble_reference.cpp) on the same graphs: the return
value, the surviving nodes and edges, the number of similarity tests and of searched junctions equal; the prediction's
hits and misses where a graph was built for them; no node sequence ever read."""
import os
import subprocess

import numpy as np
import pytest

from tests import bubble_util as bu
from tests.graph_util import ROOT, Reader

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bubble_facade")
    exe = str(d / "bubble_facade_test")
    lib = os.path.join(ROOT, "raven_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "bubble_facade_test.cpp"), "-L", lib, "-lraven_hip",
                           "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return bu.build_reference(d), exe, d


def _facade(exe, case, d, tag):
    src, dst = str(d / (tag + ".fin")), str(d / (tag + ".fout"))
    with open(src, "wb") as f:
        f.write(bu.reference_blob(case))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = Reader(open(dst, "rb").read())
    out = dict(popped=int(rd.one(np.uint32)))
    for k in ("n_junctions", "n_checked", "n_predicted", "n_misses"):
        out[k] = int(rd.one(np.uint64))
    out["node_alive"] = rd.take(np.uint8, case.n_nodes)
    out["edge_alive"] = rd.take(np.uint8, len(case.table.tail))
    out["sequence_reads"] = int(rd.one(np.uint64))
    assert rd.done()
    return out


def _same(programs, case, tag):
    ref, exe, d = programs
    want = bu.reference(ref, case, d, tag)
    got = _facade(exe, case, d, tag)
    assert got["popped"] == want["popped"] and got["n_junctions"] == want["n_junctions"]
    assert np.array_equal(got["node_alive"], want["node_alive"]) and np.array_equal(got["edge_alive"], want["edge_alive"])
    assert got["n_checked"] == len(want["tests"]) and got["sequence_reads"] == 0
    return want, got


def test_the_hand_derived_graphs(programs):
    # plain; complex and similar on either count; rejected by length; rejected by score; parallel edges; a wrapped length
    g, (B, a, b, E) = bu.diamond(1)
    g.join(b, E)
    want, got = _same(programs, g.case, "plain")
    assert (want["popped"], got["n_checked"], got["n_predicted"], got["n_misses"]) == (1, 0, 0, 0)
    for count_a in (1, 2):
        g, (B, a, b, E) = bu.diamond(1, b_subs=5, count_a=count_a)
        g.join(b, E)
        g.join(b, g.node(200, 100, unrelated=True))
        want, got = _same(programs, g.case, "complex%d" % count_a)
        # one bubble: its key was predicted, and so was the paired bubble's, which the pop then took away
        assert (want["popped"], got["n_checked"], got["n_predicted"], got["n_misses"]) == (1, 1, 2, 0)
    g, (B, a, b, E) = bu.diamond(1)
    g.join(b, E, 3, 3)
    g.join(b, g.node(200, 100, unrelated=True))
    want, got = _same(programs, g.case, "length")
    assert (want["popped"], got["n_checked"], got["n_misses"]) == (0, 2, 0)
    g, (B, a, b, E) = bu.diamond(1, b_unrelated=True, inner=200, outer=20)
    g.join(b, E)
    g.join(b, g.node(220, 20, unrelated=True))
    want, got = _same(programs, g.case, "score")
    assert (want["popped"], got["n_checked"], got["n_misses"]) == (0, 2, 0)
    g, (B, a, b, E) = bu.diamond(1, b_subs=3)
    g.join(b, E, 60, 100)
    g.join(b, E, 100, 100)
    want, got = _same(programs, g.case, "parallel")
    assert want["popped"] == 2 and want["tests"][0]["rhs_label"].tolist() == [100, 60, 0] and got["n_misses"] == 0
    g, (B, a, b, E) = bu.diamond(1, b_subs=4)
    g.join(b, E, 0xFFFFFFF0, 100)
    g.join(b, g.node(200, 100, unrelated=True))
    want, got = _same(programs, g.case, "wrapped")
    assert want["popped"] == 1 and want["tests"][0]["rhs_label"][1] == 0xFFFFFFF0 and got["n_misses"] == 0


def test_the_reach_the_shared_node_and_the_node_with_its_pair(programs):
    """The facade's own copy of the search and of the checks in front of the similarity test: a sum of exactly 500 000 is
    within reach and 500 001 is not; paths that share a node, or hold a node with its pair, are left alone and ask for
    nothing — the second and third would be complex bubbles otherwise."""
    dead = lambda w, k: np.flatnonzero(w[k] == 0).tolist()
    for tag, g, popped, dead_edges, dead_nodes in (("reach10", bu.at_the_reach(10), 1, [0, 1, 4, 5], [2, 3]),
                                                   ("reach11", bu.at_the_reach(11), 0, [], []),
                                                   ("share", bu.shared_node(), 1, [4, 5, 8, 9], [4, 5]),
                                                   ("pair", bu.node_with_its_pair(), 0, [], [])):
        want, got = _same(programs, g.case, tag)
        assert (got["popped"], dead(got, "edge_alive"), dead(got, "node_alive")) == (popped, dead_edges, dead_nodes), tag
        assert (got["n_checked"], got["n_predicted"], got["n_misses"]) == (0, 0, 0) and want["tests"] == [], tag


def test_a_pop_that_changes_a_later_search_is_a_miss(programs):
    g, n = bu.forced_miss(np.random.default_rng(5))
    want, got = _same(programs, g.case, "miss")
    assert want["popped"] == 2 and got["n_checked"] == 1 and got["n_misses"] == 1


@pytest.mark.parametrize("seed", [1, 2])
def test_chains_with_planted_bubbles_of_every_kind(programs, seed):
    g = bu.chain_with_bubbles(np.random.default_rng(seed), n_bubbles=40)
    want, got = _same(programs, g.case, "chain%d" % seed)
    verdicts = [t["similar"] for t in want["tests"]]
    by_length = [t for t in want["tests"] if t["distance"] == bu.BY_LENGTH]
    assert g.case.n_nodes > 300 and want["popped"] >= 20 and 0 in verdicts and 1 in verdicts and by_length
    assert got["n_predicted"] >= got["n_checked"] - got["n_misses"] > 0
