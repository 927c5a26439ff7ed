"""The two yardsticks of the edge similarity, held to what is known without them (no GPU):
the host build of the slice and edge rules (raven_amd/csrc/unitig_rules.h through tests/host/slice_rules_host.cpp) against
Python strings, and the restatement (tests/host/edge_similarity_reference.cpp) against edges derived by hand and against
the distances of tests/host/bubble_reference.cpp.  Both programs also run under AddressSanitizer and UBSan, as stand-alone
programs."""
import math

import numpy as np
import pytest

from tests import bubble_util as bu
from tests import edge_sim_util as eu
from tests import unitig_util as uu


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("edge_similarity_rules")


@pytest.fixture(scope="module")
def rules(workdir):
    return eu.build_rules_program(workdir)


@pytest.fixture(scope="module")
def ref(workdir):
    return eu.build_reference(workdir)


def _check_slices(exe, case, slices, workdir, tag):
    strings = [eu.slice_string(case, *s) for s in slices]
    lens, woff, words, by_segment = eu.host_slices(exe, case, slices, workdir, tag)
    ew, eo = uu.pack_all(strings)
    assert lens.tolist() == [s.shape[0] for s in strings]
    assert np.array_equal(woff, eo) and np.array_equal(words, ew)
    for got, want in zip(by_segment, strings):  # segment_slice, strand 1 included
        assert np.array_equal(got, want)
    return strings


def test_crafted_slices(rules, workdir):
    case, nodes = eu.crafted_slice_case(np.random.default_rng(1))
    slices = eu.crafted_slices(case, nodes)
    strings = _check_slices(rules, case, slices, workdir, "crafted")
    a = nodes[0]
    by = dict(zip(slices, strings))
    assert by[(a, 0, 40)].shape[0] == 40 and by[(a, 72, 2)].shape[0] == 2 and by[(a, 1, 213)].shape[0] == 213
    assert by[(a, case.length(a), 5)].shape[0] == 0 and by[(a, 33, 0xFFFFFFFF)].shape[0] == case.length(a) - 33
    assert by[(nodes[2], 0, 7)].shape[0] == 0


def test_random_slices_over_tilings_of_one_to_six_segments(rules, workdir):
    rng = np.random.default_rng(2)
    case = eu.slice_case(rng)
    assert sorted(set(len(t) for t in case.tiling)) == [1, 2, 3, 4, 5, 6]
    assert {s[3] for t in case.tiling for s in t} == {0, 1}
    _check_slices(rules, case, eu.random_slices(rng, case, 3000), workdir, "random")


def test_edge_rule(rules, workdir):
    rows = [(100, 30, 200), (100, 30, 50), (100, 100, 50), (100, 101, 50), (100, 0xFFFFFFF0, 50), (100, 0, 0), (0, 0, 7),
            (0xFFFFFFFF, 0, 0xFFFFFFFF), (0xFFFFFFFF, 1, 5), (7, 0, 7)]
    want_l = [70, 70, 0, 0, 0, 100, 0, 0xFFFFFFFF, 0xFFFFFFFE, 7]
    want_r = [70, 50, 0, 0, 0, 0, 0, 0xFFFFFFFF, 5, 7]
    lhs, rhs = eu.host_edges(rules, *zip(*rows), workdir)
    assert lhs.tolist() == want_l and rhs.tolist() == want_r


def test_restatement_on_edges_derived_by_hand(ref, workdir):
    case, want = eu.hand_case()
    got = eu.reference(ref, case, workdir, "hand")
    assert sorted(want) == list(range(len(case.table.tail)))
    for e, (l, r, d, score) in want.items():
        lhs, rhs = eu.edge_strings(case, e)
        assert (lhs.shape[0], rhs.shape[0], eu.dp_distance(lhs, rhs)) == (l, r, d), e  # the derivation itself
        assert (int(got["lhs_length"][e]), int(got["rhs_length"][e]), int(got["distance"][e])) == (l, r, d), e
        if score is None:
            assert math.isnan(got["score"][e]), e
        else:
            assert eu.bits([got["score"][e]])[0] == eu.bits([score])[0], e
    assert got["score"][0] == 1.0 and got["score"][2] == 0.9 and got["score"][10] == 0.0
    assert got["score"][0] != got["score"][1]  # an edge and its pair


def test_restatement_empty_slots_and_empty_graph(ref, workdir):
    case, _ = eu.hand_case()
    case.table.hole()
    case.join(0, 2, 3, 3)
    got = eu.reference(ref, case, workdir, "hole")
    E = len(case.table.tail)
    for e in (E - 4, E - 3):
        assert (got["lhs_length"][e], got["rhs_length"][e], got["distance"][e]) == (0, 0, eu.SLOT_EMPTY) and math.isnan(got["score"][e])
    assert got["distance"][E - 2] != eu.SLOT_EMPTY
    empty = eu.reference(ref, uu.Case([]), workdir, "empty")
    assert all(empty[k].shape[0] == 0 for k in ("lhs_length", "rhs_length", "distance", "score"))


def test_restatement_distances_equal_the_bubble_restatement(ref, workdir):
    rng = np.random.default_rng(3)
    pairs = []
    for n in (0, 1, 63, 64, 65, 200, 1500):
        a = rng.integers(0, 4, size=n).astype(np.uint8)
        pairs += [(a, a), (a, eu.mutate(rng, a, 0.2)), (a, rng.integers(0, 4, size=max(n - 7, 0)).astype(np.uint8)),
                  (a, np.zeros(0, np.uint8)), (np.zeros(0, np.uint8), a)]
    got = eu.distances(ref, pairs, workdir)
    assert np.array_equal(got, bu.distances(bu.build_reference(workdir), pairs, workdir, "bubble"))
    small = [i for i, (a, b) in enumerate(pairs) if a.shape[0] <= 200]
    assert [int(got[i]) for i in small] == [eu.dp_distance(*pairs[i]) for i in small]


def test_both_programs_under_the_sanitizers(workdir):
    rng = np.random.default_rng(4)
    rules_san = eu.build_rules_program(workdir, sanitize=True)
    case, nodes = eu.crafted_slice_case(rng)
    _check_slices(rules_san, case, eu.crafted_slices(case, nodes), workdir, "san_crafted")
    tiled = eu.slice_case(rng)
    _check_slices(rules_san, tiled, eu.random_slices(rng, tiled, 300), workdir, "san_random")
    eu.host_edges(rules_san, [5, 0], [9, 0], [3, 0], workdir, "san_edges")
    ref_san = eu.build_reference(workdir, sanitize=True)
    hand, want = eu.hand_case()
    hand.table.hole()
    got = eu.reference(ref_san, hand, workdir, "san_hand")
    assert [int(got["distance"][e]) for e in sorted(want)] == [want[e][2] for e in sorted(want)]
    multi = eu.overlap_case(rng, (1, 63, 64, 65, 300), 0.15, multi=True)
    eu.reference(ref_san, multi, workdir, "san_multi")
