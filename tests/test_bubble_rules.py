"""RemoveBubbles on the CPU: the restatement (tests/host/bubble_reference.cpp) pinned by results derived by hand, its edit
distance equal to the oracle's textbook DP, and the host build of the path rule and of the similarity threshold
(tests/host/bubble_rules_host.cpp over raven_amd/csrc/unitig_rules.h and overlap_rules.h) equal to the strings — also under
the address and undefined-behaviour sanitizers, the programs having their own main.

The hand-derived graphs lie on a genome: node = 100 bases from its position on, an edge as long as the distance between
the starts (tests/bubble_util.py: GenomeGraph).  Ids in creation order: first node 0, its pair 1, and so on; edge 2j is the
j-th join, 2j + 1 its pair."""
import numpy as np
import pytest

from oracle import oracle
from tests import bubble_util as bu
from tests import unitig_util as uu


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bubble_rules")
    return bu.build_reference(d), bu.build_rules_program(d), d


def _dp(case, t):
    l, r = bu.path_string(case, t["lhs"], t["lhs_label"]), bu.path_string(case, t["rhs"], t["rhs_label"])
    assert (l.shape[0], r.shape[0]) == (t["l"], t["r"])
    return oracle.edit_distance(l.tobytes(), r.tobytes())


def test_a_simple_bubble_needs_no_similarity_test(programs):
    """Both arms plain: the arm with the smaller count goes, the left one (found first) on a tie; its node goes with it.
    After the pop E' (node 7) has one out-edge left: the loop searched from node 0 alone."""
    ref, _, d = programs
    for count_a, dead_edges, dead_nodes in ((1, [0, 1, 4, 5], [2, 3]), (3, [2, 3, 6, 7], [4, 5])):
        g, (B, a, b, E) = bu.diamond(count_a=count_a)
        g.join(b, E)
        w = bu.reference(ref, g.case, d)
        assert w["popped"] == 1 and w["tests"] == [] and w["n_junctions"] == 1
        assert np.flatnonzero(w["edge_alive"] == 0).tolist() == dead_edges and np.flatnonzero(w["node_alive"] == 0).tolist() == dead_nodes


def test_a_complex_bubble_is_popped_on_the_side_with_the_smaller_count(programs):
    """b has a second out-edge to a dead end x: the right path is complex, and of it only b -> E may go.  Five
    substitutions in b: both strings have 300 bases, the distance is 5, the score 1 - 5 / 300.  Counts equal: the left
    path goes whole.  count(a) = 2: the right side loses b -> E and its pair, no node."""
    ref, _, d = programs
    for count_a, dead_edges, junctions in ((1, [0, 1, 4, 5], 2), (2, [6, 7], 1)):
        g, (B, a, b, E) = bu.diamond(b_subs=5, count_a=count_a)
        g.join(b, E)
        g.join(b, g.node(200, 100, unrelated=True))
        w = bu.reference(ref, g.case, d)
        assert w["popped"] == 1 and len(w["tests"]) == 1 and w["n_junctions"] == junctions
        t = w["tests"][0]
        assert t["lhs"].tolist() == [0, 2, 6] and t["rhs"].tolist() == [0, 4, 6]
        assert t["lhs_label"].tolist() == [100, 100, 0] and t["rhs_label"].tolist() == [100, 100, 0]
        assert (t["l"], t["r"], t["distance"], t["similar"]) == (300, 300, 5, 1) and _dp(g.case, t) == 5
        assert np.flatnonzero(w["edge_alive"] == 0).tolist() == dead_edges
        assert np.flatnonzero(w["node_alive"] == 0).tolist() == ([2, 3] if count_a == 1 else [])


def test_rejected_by_length_from_both_sides(programs):
    """b -> E of 3 bases: the right string has 100 + 3 + 100 = 203 bases, fewer than 0.8 x 300 = 240.  The paired bubble
    (from E', node 7: b' has two in-edges) is asked for as well, and rejected the same way.  Nothing is aligned, nothing
    goes; the loop searched from B, b (two out-edges, no bubble) and E'."""
    ref, _, d = programs
    g, (B, a, b, E) = bu.diamond()
    g.join(b, E, 3, 3)
    g.join(b, g.node(200, 100, unrelated=True))
    w = bu.reference(ref, g.case, d)
    assert w["popped"] == 0 and w["node_alive"].all() and w["edge_alive"].all() and w["n_junctions"] == 3
    assert [(t["l"], t["r"], t["distance"], t["similar"]) for t in w["tests"]] == [(300, 203, bu.BY_LENGTH, 0)] * 2
    assert w["tests"][1]["lhs"].tolist() == [7, 3, 1] and w["tests"][1]["rhs"].tolist() == [7, 5, 1]
    assert w["tests"][1]["rhs_label"].tolist() == [3, 100, 0]


def test_rejected_by_score(programs):
    """Arms of 200 unrelated bases between ends of 20: 240 bases each way, and a distance far above 0.2 x 240 = 48."""
    ref, _, d = programs
    g, (B, a, b, E) = bu.diamond(b_unrelated=True, inner=200, outer=20)
    g.join(b, E)
    g.join(b, g.node(220, 20, unrelated=True))
    w = bu.reference(ref, g.case, d)
    assert w["popped"] == 0 and w["edge_alive"].all() and len(w["tests"]) == 2
    for t in w["tests"]:
        assert (t["l"], t["r"], t["similar"]) == (240, 240, 0) and t["distance"] == _dp(g.case, t) and 48 < t["distance"] <= 200


def test_paths_that_share_a_node_or_hold_a_pair_are_left_alone(programs):
    ref, _, d = programs
    # B -> a -> {c, d} -> E and a dead end B -> z: from B both paths run through a; from a the bubble is plain
    g = bu.shared_node()
    w = bu.reference(ref, g.case, d, "share")
    assert w["tests"] == [] and w["popped"] == 1 and np.flatnonzero(w["edge_alive"] == 0).tolist() == [4, 5, 8, 9]
    # B -> a -> E and B -> a' -> E: a (two out-edges: E and B') makes the bubble complex, but a path holds a node's pair
    g = bu.node_with_its_pair()
    w = bu.reference(ref, g.case, d, "pair")
    assert w["tests"] == [] and w["popped"] == 0 and w["edge_alive"].all() and w["node_alive"].all()


def test_the_first_out_edge_to_the_next_node_states_the_label(programs):
    """b -> E twice, 60 bases first, then 100: the search stops at the first of them (it closes the bubble), the string
    takes the first one's 60 bases (100 + 60 + 100 = 260), and b, with its two out-edges, makes the bubble complex.  The
    left path goes (equal counts); then the search from b itself meets E twice, a plain bubble of two one-step paths, and
    the step it removes is again the first of the two edges."""
    ref, _, d = programs
    g, (B, a, b, E) = bu.diamond(b_subs=3)
    first = g.join(b, E, 60, 100)
    g.join(b, E, 100, 100)
    w = bu.reference(ref, g.case, d)
    t = w["tests"][0]
    assert t["rhs"].tolist() == [0, 4, 6] and t["rhs_label"].tolist() == [100, 60, 0] and (t["l"], t["r"]) == (300, 260)
    assert t["distance"] == _dp(g.case, t) and 40 <= t["distance"] <= 43 and t["similar"] == 1
    assert first == 6 and w["popped"] == 2 and np.flatnonzero(w["edge_alive"] == 0).tolist() == [0, 1, 4, 5, 6, 7]


def test_a_wrapped_edge_length_is_within_reach_and_gives_the_whole_node(programs):
    """b -> E with length 2^32 - 16: 100 + (2^32 - 16) wraps to 84, which is within reach; the label is the whole of b."""
    ref, _, d = programs
    g, (B, a, b, E) = bu.diamond(b_subs=4)
    g.join(b, E, 0xFFFFFFF0, 100)
    g.join(b, g.node(200, 100, unrelated=True))
    w = bu.reference(ref, g.case, d)
    t = w["tests"][0]
    assert t["rhs_label"].tolist() == [100, 0xFFFFFFF0, 0] and (t["l"], t["r"], t["distance"], t["similar"]) == (300, 300, 4, 1)
    assert w["popped"] == 1


def test_the_reach_of_500_000_bases(programs):
    """B -> a of 499 990 bases (the label is a's 100 all the same): with a -> E of 10 the end is exactly 500 000 away and
    the plain bubble is popped; with 11 the edge is out of reach and no second way to E is ever seen."""
    ref, _, d = programs
    for last, popped in ((10, 1), (11, 0)):
        g = bu.at_the_reach(last)
        w = bu.reference(ref, g.case, d, "reach%d" % last)
        assert w["popped"] == popped and w["tests"] == [] and int((w["edge_alive"] == 0).sum()) == 4 * popped


def test_a_pop_changes_what_a_later_search_finds(programs):
    """bubble_util.forced_miss: from J (node 2) the untouched graph gives two paths through I (nothing to test); after I's
    bubble is popped the search from J reaches F by two ways, and I's second in-edge makes that bubble complex."""
    ref, _, d = programs
    g, n = bu.forced_miss(np.random.default_rng(5))
    w = bu.reference(ref, g.case, d)
    first = w["tests"][0]
    assert first["lhs"].tolist() == [n["J"], n["z"], n["w"], n["F"]] and first["rhs"].tolist() == [n["J"], n["I"], n["b"], n["E"], n["F"]]
    assert (first["l"], first["r"], first["similar"]) == (500, 500, 1) and first["distance"] == _dp(g.case, first) <= 3
    # I's plain bubble went first (the left arm, through a), then the three steps of J -> z -> w -> F (counts 4 against 6)
    assert w["popped"] == 2 and w["node_alive"][n["a"]] == 0 and w["node_alive"][n["z"]] == 0 and w["node_alive"][n["w"]] == 0
    assert int((w["edge_alive"] == 0).sum()) == 4 + 6


def test_the_restatements_distance_is_the_textbook_dp(programs):
    ref, _, d = programs
    rng = np.random.default_rng(6)
    pairs = []
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 300, 1000):
        a = rng.integers(0, 4, size=n).astype(np.uint8)
        for b in (a, bu.plant(rng, a, min(n, 7)) if n else a, rng.integers(0, 4, size=n + 13).astype(np.uint8), a[:n // 2],
                  np.concatenate([a[n // 3:], a[:n // 3]]), np.zeros(max(1, n - 5), np.uint8)):
            pairs.append((a, b))
            pairs.append((b, a))
    got = bu.distances(ref, pairs, d)
    assert got.tolist() == [oracle.edit_distance(a.tobytes(), b.tobytes()) for a, b in pairs]


def _paths_of(case, tests):
    return [(t[s], t[s + "_label"]) for t in tests for s in ("lhs", "rhs")]


def test_host_path_rule_on_the_hand_derived_paths_and_random_ones(programs):
    ref, host, d = programs
    g, _ = bu.diamond(b_subs=4)
    E = 6
    g.join(4, E, 0xFFFFFFF0, 100)
    g.join(4, g.node(200, 100, unrelated=True))
    w = bu.reference(ref, g.case, d, "hp")
    paths = _paths_of(g.case, w["tests"]) + [([0], [5]), ([0, 2], [0, 9]), ([0, 2, 6], [99, 101, 0]), ([1, 3], [1, 1])]
    _check_paths(host, g.case, paths, d, "hand")
    total = 0
    for seed in range(4):
        rng = np.random.default_rng(200 + seed)
        case = uu.random_tiled_case(rng)
        paths = bu.random_paths(rng, case, 800)
        total += len(paths)
        _check_paths(host, case, paths, d, "r%d" % seed)
    assert total >= 3000


def _check_paths(host, case, paths, d, tag):
    lens, woff, words = bu.host_paths(host, case, paths, d, tag)
    strings = [bu.path_string(case, n, l) for n, l in paths]
    ew, eo = uu.pack_all(strings)
    assert lens.tolist() == [s.shape[0] for s in strings] and np.array_equal(woff, eo) and np.array_equal(words, ew)


def test_host_threshold_is_the_largest_distance_that_passes(programs):
    _, host, d = programs
    mx = np.array([1, 2, 3, 4, 5, 9, 10, 11, 99, 100, 101, 1000, 20_000, 41_000, 500_000, 4_000_000_000], np.uint32)
    for ratio in (0.8, 0.5, 0.93, 0.0, 1.0):
        got = bu.host_kmax(host, mx, ratio, d, "k%g" % ratio)
        assert got.tolist() == [bu.kmax(int(x), ratio) for x in mx]
        for x, k in zip(mx.tolist(), got.tolist()):
            assert not (1.0 - k / x < ratio) or k == 0
            assert k == x or (1.0 - (k + 1) / x < ratio)
    assert bu.host_kmax(host, [5, 10, 100], 0.8, d, "by_hand").tolist() == [1, 2, 20]  # (1 - 1 / 5 = 0.8 is not below 0.8)


def test_host_programs_under_the_sanitizers(programs, tmp_path):
    ref, _, d = programs
    san_ref, san_host = bu.build_reference(tmp_path, sanitize=True), bu.build_rules_program(tmp_path, sanitize=True)
    g, n = bu.forced_miss(np.random.default_rng(5))
    assert bu.reference(san_ref, g.case, tmp_path, "s")["tests"][0]["l"] == 500
    rng = np.random.default_rng(9)
    case = uu.random_tiled_case(rng)
    _check_paths(san_host, case, bu.random_paths(rng, case, 300), tmp_path, "sp")
    assert bu.host_kmax(san_host, [100, 41_000], 0.8, tmp_path, "sk").tolist() == [20, 8200]
