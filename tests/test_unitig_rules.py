"""CreateUnitigs on the CPU: the restatement (tests/host/unitig_reference.cpp) pinned by results derived by hand, and the
host build of raven_amd/csrc/unitig_rules.h (tests/host/unitig_rules_host.cpp) equal to the restatement's strings on seeded
random tilings — also under the address and undefined-behaviour sanitizers, the program having its own main."""
import numpy as np
import pytest

from tests import unitig_util as uu


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("unitig_rules")
    return uu.build_reference(d), uu.build_rules_program(d), d


def _reads(k, n=10, seed=5):
    return uu.random_reads(np.random.default_rng(seed), k, n, n)


def test_chain_of_three_between_two_junctions(programs):
    """J1 -> a -> b -> c -> J2 with a second edge out of J1 and a second into J2; reads of 10 bases.  By hand: node a = 2 is
    the first non-junction that is met, the unitig 14 = a[:3] + b[:2] + c (15 bases), its pair 15 walks 7 -> 5 -> 3 over the
    pair edges of lengths 1 and 4: c'[:1] + b'[:4] + a' (15 bases).  The in-edge J1 -> a (length 5) becomes J1 -> 14 (5), its
    pair (length 6) 15 -> J1' with 6 + 15 - 10 = 11; the out-edge c -> J2 (7) becomes 14 -> J2 with 7 + 15 - 10 = 12, its
    pair J2' -> 15 keeps its 8.  Coverage (10 + 21) / 2 = 15."""
    ref, _, d = programs
    case = uu.Case(_reads(7))
    j1, a, b, c, j2, x, y = uu.simple_nodes(case, 7)
    case.coverage[a] = case.coverage[a + 1] = 10
    case.coverage[c] = case.coverage[c + 1] = 21
    case.join(j1, a, 5, 6)
    case.join(a, b, 3, 4)
    case.join(b, c, 2, 1)
    case.join(c, j2, 7, 8)
    case.join(j1, x, 1, 1)
    case.join(y, j2, 1, 1)
    w = uu.reference(ref, case, 0, d)
    assert w["begin"].tolist() == [2, 7] and w["end"].tolist() == [6, 3] and w["is_circular"].tolist() == [0, 0]
    assert w["member_offsets"].tolist() == [0, 3, 6] and w["members"].tolist() == [2, 4, 6, 7, 5, 3]
    assert w["count"].tolist() == [3, 3] and w["length"].tolist() == [15, 15] and w["coverage"].tolist() == [15, 15]
    assert w["marked"].tolist() == [1] * 8 + [0] * 4
    assert w["edge_tail"].tolist() == [0, 15, 14, 9] and w["edge_head"].tolist() == [14, 1, 8, 15]
    assert w["edge_length"].tolist() == [5, 11, 12, 8]
    s = [case.sequence(u) for u in range(case.n_nodes)]
    assert np.array_equal(w["sequences"][0], np.concatenate([s[2][:3], s[4][:2], s[6]]))
    assert np.array_equal(w["sequences"][1], np.concatenate([s[7][:1], s[5][:4], s[3]]))
    # RemoveEdges(marked, true) takes a .. c and their pairs; nothing here is long enough for GetUnitigs
    assert w["alive"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1] and w["selected"].tolist() == []


@pytest.mark.parametrize("eps", [0, 1, 42])
def test_epsilon_trim_on_each_side_of_the_threshold(programs, eps):
    """A chain between two dead ends with 2 eps + 1 nodes makes nothing, with 2 eps + 2 a unitig of the two nodes in the
    middle, with 2 eps + 3 one of three; with eps > 0 both ends of the unitig have a chain edge to take over (4 new edges,
    2 more marked pairs), with eps = 0 a dead end has none."""
    ref, _, d = programs
    for extra, members in ((1, 0), (2, 2), (3, 3)):
        L = 2 * eps + extra
        case, ids = uu.line_case(np.random.default_rng(eps * 10 + extra), L)
        w = uu.reference(ref, case, eps, d)
        if not members:
            assert w["begin"].shape[0] == 0 and w["marked"].sum() == 0 and w["alive"].all()
            continue
        assert w["begin"].tolist() == [ids[eps], ids[L - 1 - eps] ^ 1] and w["end"].tolist() == [ids[L - 1 - eps], ids[eps] ^ 1]
        assert w["members"].tolist() == ids[eps:L - eps] + [u ^ 1 for u in reversed(ids[eps:L - eps])]
        assert w["edge_tail"].shape[0] == (4 if eps else 0)
        assert int(w["marked"].sum()) == 2 * (members - 1 + (2 if eps else 0))


def test_self_loop_and_cycles(programs):
    ref, _, d = programs
    # u -> u of length 4, the pair's 6: the unitig is u[:4], its pair u'[:6]; nothing connects, both edges go
    case = uu.Case(_reads(1))
    u, = uu.simple_nodes(case, 1, count=7)
    case.join(u, u, 4, 6)
    w = uu.reference(ref, case, 42, d)
    assert w["begin"].tolist() == [0, 1] and w["end"].tolist() == [0, 1] and w["is_circular"].tolist() == [1, 1]
    assert w["members"].tolist() == [0, 1] and w["length"].tolist() == [4, 6] and w["count"].tolist() == [7, 7]
    assert w["edge_tail"].shape[0] == 0 and w["marked"].tolist() == [1, 1] and w["alive"].tolist() == [0, 0, 1, 1]
    assert np.array_equal(w["sequences"][0], case.sequence(0)[:4]) and np.array_equal(w["sequences"][1], case.sequence(1)[:6])
    # 4 -> 0 -> 2 -> 4: node 0 creates and the walk starts there; the pair edges are 1 -> 5, 3 -> 1, 5 -> 3, walked from 1
    case = uu.Case(_reads(3))
    a, b, c = uu.simple_nodes(case, 3)
    case.join(c, a, 1, 2)
    case.join(a, b, 3, 4)
    case.join(b, c, 5, 6)
    w = uu.reference(ref, case, 1, d)  # (no trim and no size rule on a cycle)
    assert w["members"].tolist() == [0, 2, 4, 1, 5, 3] and w["is_circular"].tolist() == [1, 1]
    assert w["length"].tolist() == [3 + 5 + 1, 2 + 6 + 4] and w["marked"].all() and not w["alive"][:6].any()
    # a cycle of two
    case = uu.Case(_reads(2))
    a, b = uu.simple_nodes(case, 2)
    case.join(b, a, 9, 0)
    case.join(a, b, 10, 1)
    w = uu.reference(ref, case, 0, d)
    assert w["members"].tolist() == [0, 2, 1, 3] and w["length"].tolist() == [19, 1]


def test_the_orientation_that_holds_the_smallest_id_creates(programs):
    ref, _, d = programs
    # 1 -> 2 and its pair 3 -> 0: node 0 is met first, so the unitig is 3 -> 0 and its pair 1 -> 2
    case = uu.Case(_reads(2))
    a, b = uu.simple_nodes(case, 2)
    case.join(a ^ 1, b, 4, 5)
    w = uu.reference(ref, case, 0, d)
    assert w["begin"].tolist() == [3, 1] and w["end"].tolist() == [0, 2] and w["members"].tolist() == [3, 0, 1, 2]
    assert w["length"].tolist() == [5 + 10, 4 + 10]
    # all on the reverse strand: 1 -> 3 -> 5 is the PAIR; 4 -> 2 -> 0 creates
    case, ids = uu.line_case(np.random.default_rng(1), 3, flip=[1, 1, 1])
    w = uu.reference(ref, case, 0, d)
    assert w["members"].tolist() == [4, 2, 0, 1, 3, 5]


def test_is_unitig_at_its_thresholds_and_coverage(programs):
    """is_unitig = count > 5 and length > 9999: two reads of 5000 bases joined by an edge of 4999 / 5000 bases give 9999 /
    10000; counts 2 + 3 and 3 + 3.  Coverage is the truncated mean of the two ends."""
    ref, _, d = programs
    for counts, edge, want in (((2, 3), 5000, 0), ((3, 3), 4999, 0), ((3, 3), 5000, 1)):
        case = uu.Case(uu.random_reads(np.random.default_rng(3), 2, 5000, 5000))
        a, b = uu.simple_nodes(case, 2)
        case.count = [counts[0]] * 2 + [counts[1]] * 2
        case.join(a, b, edge, edge)
        w = uu.reference(ref, case, 0, d)
        assert w["is_unitig"].tolist() == [want, want] and w["length"].tolist() == [edge + 5000] * 2
        assert w["selected"].tolist() == ([4] if want else []) and w["count"].tolist() == [sum(counts)] * 2
    for ca, cb, want in ((65535, 65535, 65535), (65535, 0, 32767), (1, 2, 1), (0, 1, 0)):
        case = uu.Case(_reads(2))
        a, b = uu.simple_nodes(case, 2)
        case.coverage = [ca, ca, cb, cb]
        case.join(a, b, 1, 1)
        assert uu.reference(ref, case, 0, d)["coverage"].tolist() == [want, want]


def test_a_chain_edge_longer_than_its_tail_is_refused(programs):
    ref, _, d = programs
    case = uu.Case(_reads(2))
    a, b = uu.simple_nodes(case, 2)
    case.join(a, b, 11, 0)
    assert uu.reference(ref, case, 0, d, ok=(4,)) is None


def _check_host(case, want, host, d, tag):
    keep = uu.member_prefixes(case, want)
    tilings, words, woff = uu.host_words(host, case, want, keep, d, tag)
    assert tilings == uu.expected_tilings(case, want, keep)
    ew, eo = uu.pack_all(want["sequences"])
    assert np.array_equal(woff, eo) and np.array_equal(words, ew)


def test_host_rules_match_the_restatement_on_random_tilings(programs):
    ref, host, d = programs
    total = 0
    for seed in range(6):
        case = uu.random_tiled_case(np.random.default_rng(100 + seed))
        want = uu.reference(ref, case, seed % 2, d, "r%d" % seed)
        total += want["begin"].shape[0]
        assert want["is_circular"].max() == 1 and want["is_circular"].min() == 0
        _check_host(case, want, host, d, "h%d" % seed)
    assert total > 40


def test_host_rules_under_the_sanitizers(programs, tmp_path):
    ref, _, d = programs
    san = uu.build_rules_program(tmp_path, sanitize=True)
    case = uu.random_tiled_case(np.random.default_rng(7))
    want = uu.reference(ref, case, 0, d, "s")
    _check_host(case, want, san, tmp_path, "hs")
