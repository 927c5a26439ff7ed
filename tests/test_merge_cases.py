"""No GPU: the plain reference of the merge stage (tests/merge_cases.py::MergeRef) against the oracle's whole first pass,
every generator against what its cases are named after, and the comparison helper against the mistakes it has to notice.
tests/test_gpu_merge.py runs the same cases on the device."""
import numpy as np
import pytest

from oracle import oracle
from tests import merge_cases as mc

DT = mc.DT


def _family(name):
    return [c for c in mc.cases() if c["family"] == name]


def _pile(state, p):
    off = state["pile_offsets"]
    return state["data"][int(off[p]):int(off[p + 1])]


def _list(state, p):
    off = state["offsets"]
    return state["overlaps"][int(off[p]):int(off[p + 1])]


def _lengths(ovl):
    return np.maximum(ovl["rhs_end"].astype(np.int64) - ovl["rhs_begin"], ovl["lhs_end"].astype(np.int64) - ovl["lhs_begin"])


def _arrival(case, flush, p):
    """Pile p's new entries of one flush in the reference's order, from the flush's list alone."""
    out = []
    for o in case["flushes"][flush].tolist():
        if o[0] == p:
            out.append(o)
        if o[3] == p:
            out.append(mc.reverse(o))
    return out


# ---- the reference against the oracle's whole pass -------------------------------------------------------------------

@pytest.fixture(scope="module")
def lambda_map(lambda_reads):
    """The oracle's Map output of every lambda read, as the pass itself asks for it."""
    rs = lambda_reads
    assert np.array_equal(rs.ids, np.arange(rs.n))
    oe = oracle.Engine(15, 5)
    oe.minimize(rs, 0, rs.n, minhash=False)
    oe.filter(0.001)
    return [oe.map(rs, i, True, True, True)["overlaps"] for i in range(rs.n)]


@pytest.mark.parametrize("quarter", [False, True], ids=["one_flush", "quarter_flushes"])
@pytest.mark.parametrize("kmax", [8, 32])
def test_reference_equals_the_oracle_pass_on_the_lambda_reads(lambda_reads, lambda_map, kmax, quarter):
    rs = lambda_reads
    flush_bases = rs.total_bases // 4 if quarter else 1 << 30
    windows = mc.flush_windows(rs.lengths, flush_bases)
    assert len(windows) == (4 if quarter else 1) or (quarter and len(windows) == 5)
    ref = mc.MergeRef(rs.lengths, kmax)
    for first, last in windows:
        part = [m for m in lambda_map[first:last] if m.shape[0]]
        flush = np.concatenate(part) if part else np.zeros(0, DT)
        mc.assert_defined(rs.lengths, flush)
        ref.flush(flush)
    want = oracle.Engine(15, 5).find_overlaps_and_create_piles(rs, kmax=kmax, flush_bases=flush_bases)
    got = ref.state()
    assert mc.diff_state(got, dict(data=want["pile_data"], pile_offsets=want["pile_offsets"], overlaps=want["overlaps"],
                                   offsets=want["overlap_offsets"])) is None
    assert got["overlaps"].shape[0] > 1000 and int(np.diff(got["offsets"].astype(np.int64)).max()) == kmax


def test_add_layers_equals_the_oracle_on_the_tile_cases():
    """mc.add_layers is pile.cc's sweep in Python; the oracle's is the same sweep in C++, wrap-around included."""
    n_wraps = 0
    for case in _family("tiles"):
        ref = mc.MergeRef(case["lengths"], case["kmax"])
        for f, flush in enumerate(case["flushes"]):
            before = [c.copy() for c in ref.coverage]
            counted = list(ref.counted)
            lists = [list(x) for x in ref.lists]
            ref.flush(flush)
            for p in range(ref.n):
                new = lists[p][counted[p]:] + _arrival(case, f, p)
                if not new:
                    assert np.array_equal(ref.coverage[p], before[p])
                    continue
                want = before[p].copy()
                oracle.pile_add_layers(want, p, np.array(new, dtype=DT))
                assert np.array_equal(ref.coverage[p], want), (case["name"], f, p)
                b, e = mc.events(np.array(new, dtype=DT), p)
                n_wraps += int(np.count_nonzero(e < b))
    assert n_wraps >= 16


# ---- the generators --------------------------------------------------------------------------------------------------

def test_every_family_has_its_cases_and_defined_input():
    assert {c["family"] for c in mc.cases()} == set(mc.FAMILIES)
    assert set(mc.SUBSET) <= set(mc.names()) and {mc.by_name(n)["family"] for n in mc.SUBSET} == set(mc.FAMILIES)
    for case in mc.cases():
        for flush in case["flushes"]:
            mc.assert_defined(case["lengths"], flush)
    # the check itself refuses what the reference does not define
    lengths = np.array([4000, 4000], np.uint32)
    ok = np.array([(0, 16, 200, 1, 32, 300, 7, 0)], dtype=DT)
    mc.assert_defined(lengths, ok)
    for field, value in (("lhs_id", 1), ("rhs_id", 2), ("lhs_end", 4001), ("rhs_end", 15), ("rhs_begin", 300)):
        bad = ok.copy()
        bad[field] = value
        with pytest.raises(AssertionError):
            mc.assert_defined(lengths, bad)
    # 250 cells: a short overlap with its end event on the last cell and its begin event one past it is defined (the
    # reference writes cell 249); with the begin event on cell 251 it is not (the reference writes cell 250)
    mc.assert_defined(np.array([4015, 4000], np.uint32), np.array([(0, 3984, 4007, 1, 32, 300, 7, 0)], dtype=DT))
    with pytest.raises(AssertionError):
        mc.assert_defined(np.array([4015, 4000], np.uint32), np.array([(0, 4000, 4010, 1, 32, 300, 7, 0)], dtype=DT))
    with pytest.raises(IndexError):
        mc.add_layers(np.zeros(250, np.uint16), 0, [(0, 4000, 4010, 1, 32, 300, 7, 0)])


def test_order_cases_place_what_they_say():
    for case in _family("order"):
        ref = mc.reference(case["name"])
        f1, f2 = case["flushes"]
        for flush in (f1, f2):
            for o in flush.tolist():
                assert len(set(o)) == 8  # a missing or doubled reversal shows in every field
        for t, ((in1, own1), (in2, own2)) in case["claims"]["arrived"].items():
            for flush, n_in, n_own in ((f1, in1, own1), (f2, in2, own2)):
                assert int(np.count_nonzero(flush["rhs_id"] == t)) == n_in
                assert int(np.count_nonzero(flush["lhs_id"] == t)) == n_own
            # several earlier queries feed the pile, and their emissions alternate with other piles
            feeders = f2["lhs_id"][f2["rhs_id"] == t]
            assert set(feeders.tolist()) == set(mc.ORDER_Q) and np.all(feeders < t)
            for q in mc.ORDER_Q:
                rhs = f2["rhs_id"][f2["lhs_id"] == q]
                assert np.count_nonzero(np.diff(rhs.astype(np.int64)) != 0) > 40  # (of about 56 emissions)
            kept = min(in1 + own1, case["kmax"])
            assert _list(ref[0], t).shape[0] == kept
            assert _list(ref[1], t).shape[0] == min(kept + in2 + own2, case["kmax"])
        sizes = sorted(_list(ref[0], t).shape[0] for t in mc.ORDER_T)
        if case["kmax"] >= 65:
            assert sizes == [63, 64, 65]
        if case["kmax"] == 200:  # nothing is sorted: kept, then the reversed incoming by query, then the pile's own
            for t in mc.ORDER_T:
                got = _list(ref[1], t).tolist()
                assert got == _arrival(case, 0, t) + _arrival(case, 1, t)
                new = got[len(_arrival(case, 0, t)):]
                assert [o[3] < t for o in new] == [True] * mc.ORDER_COUNTS[t - 6] + [False] * mc.ORDER_COUNTS[t - 6]
    assert mc.boundary_between_feeders(mc.by_name("order:kmax65")["flushes"][1]) is not None


def test_piles_cases_place_what_they_say():
    cases = _family("piles")
    assert [c["lengths"].shape[0] for c in cases] == list(mc.PILE_COUNTS) + [70000]
    for case in cases:
        ref = mc.reference(case["name"])
        n = case["lengths"].shape[0]
        quiet = case["claims"]["quiet"]
        assert (len(quiet) > 0) == (n >= 3)
        for st in ref:
            sizes = np.diff(st["offsets"].astype(np.int64))
            assert not sizes[quiet].any()
            if n >= 3:
                assert np.count_nonzero(sizes) >= (n - len(quiet)) * 3 // 5
            for p in quiet[:50]:
                assert not _pile(st, p).any()
        if n >= 63:  # quiet piles sit among the others
            q = np.array(quiet)
            assert np.all(np.diff(q) > 1) and q[0] > 0
    wide = mc.by_name("piles:70000")
    assert np.all(wide["lengths"] == 64)
    rhs = np.concatenate([f["rhs_id"] for f in wide["flushes"]]).astype(np.int64)
    for bit in range(17):  # every bit of a 17-bit key is 0 somewhere and 1 somewhere; the digits above are all zero
        assert 0 < np.count_nonzero(rhs >> bit & 1) < rhs.shape[0]
    assert int(rhs.max()) >= 65536 and np.count_nonzero(np.diff(wide["flushes"][0]["rhs_id"].astype(np.int64)) < 0) > 5000


def test_kmax_cases_place_what_they_say():
    cases = _family("kmax")
    assert [c["kmax"] for c in cases] == list(mc.KMAX_VALUES)
    for case in cases:
        kmax = case["kmax"]
        ref = mc.reference(case["name"])
        plan = case["claims"]["arrived"]
        assert plan[0][mc.KMAX_GROW] == kmax - 1 and plan[1][mc.KMAX_GROW] == 1 and plan[2][mc.KMAX_GROW] == 1
        assert plan[0][mc.KMAX_FULL] == kmax and plan[1][mc.KMAX_FULL] > 3 * kmax
        assert plan[0][mc.KMAX_SKIP] == kmax + 1
        size = {}
        for f, step in enumerate(plan):
            flush = case["flushes"][f]
            for t in (mc.KMAX_GROW, mc.KMAX_FULL, mc.KMAX_SKIP, mc.KMAX_ONE, mc.KMAX_NEVER):
                arrived = int(np.count_nonzero(flush["lhs_id"] == t) + np.count_nonzero(flush["rhs_id"] == t))
                assert arrived == step.get(t, 0), (case["name"], f, t)
                before = size.get(t, 0)
                got = _list(ref[f], t)
                if arrived == 0:  # untouched: the kept list goes through as it is
                    assert got.tolist() == (_list(ref[f - 1], t).tolist() if f else [])
                    assert np.array_equal(_pile(ref[f], t), _pile(ref[f - 1], t) if f else np.zeros_like(_pile(ref[f], t)))
                    continue
                total = before + arrived
                merged = (_list(ref[f - 1], t).tolist() if f else []) + _arrival(case, f, t)
                assert len(merged) == total
                if total < kmax:  # left in arrival order
                    assert got.tolist() == merged
                else:  # sorted; cut only beyond kmax
                    assert got.shape[0] == kmax and np.all(np.diff(_lengths(got)) <= 0)
                    assert sorted(_lengths(got).tolist(), reverse=True) == sorted(
                        _lengths(np.array(merged, dtype=DT)).tolist(), reverse=True)[:kmax]
                size[t] = min(total, kmax)
                # coverage: every arrival once, the cut ones of this flush included, the kept ones not again
                want = _pile(ref[f - 1], t).copy() if f else np.zeros_like(_pile(ref[f], t))
                mc.add_layers(want, t, _arrival(case, f, t))
                assert np.array_equal(_pile(ref[f], t), want)
        # the sizes before the cut, flush by flush
        assert [kmax - 1, kmax, kmax + 1] == [sum(s.get(mc.KMAX_GROW, 0) for s in plan[:f + 1]) for f in range(3)]
        assert mc.KMAX_SKIP not in plan[1] and mc.KMAX_ONE not in plan[1] and mc.KMAX_SKIP in plan[2]
        assert all(mc.KMAX_NEVER not in s for s in plan) and not _pile(ref[2], mc.KMAX_NEVER).any()
        # total coverage of a pile = sum over ALL arrivals of all flushes, whatever was cut
        for t in (mc.KMAX_FULL, mc.KMAX_SKIP):
            want = np.zeros_like(_pile(ref[2], t))
            for f in range(3):
                mc.add_layers(want, t, _arrival(case, f, t))
            assert np.array_equal(_pile(ref[2], t), want) and want.any()
        if kmax >= 16:  # ties sit on the cut
            got = _lengths(_list(ref[1], mc.KMAX_FULL))
            merged = _lengths(np.array(_list(ref[0], mc.KMAX_FULL).tolist() + _arrival(case, 1, mc.KMAX_FULL), dtype=DT))
            assert np.count_nonzero(merged == got[-1]) > np.count_nonzero(got == got[-1])


def _stable(entries, kmax):
    order = np.argsort(-_lengths(entries), kind="stable")
    return entries[order][:kmax]


def test_sort_cases_place_what_they_say():
    case = mc.by_name("sort:patterns")
    ref = mc.reference("sort:patterns")[0]
    differs = {}
    for (m, pattern), t in case["claims"]["where"].items():
        arrived = np.array(_arrival(case, 0, t), dtype=DT)
        assert arrived.shape[0] == m and sorted(_lengths(arrived).tolist()) == sorted(mc._sort_lengths(pattern, m))
        assert 0 < np.count_nonzero(arrived["rhs_id"] < t) < m  # reversed arrivals and the pile's own
        got = _list(ref, t)
        assert got.shape[0] == mc.SORT_KMAX and np.all(np.diff(_lengths(got)) <= 0)
        differs[(m, pattern)] = got.tolist() != _stable(arrived, mc.SORT_KMAX).tolist()
        ln = _lengths(arrived)
        if pattern == "equal":
            assert len(set(ln.tolist())) == 1
        elif pattern == "two":
            assert len(set(ln.tolist())) == 2
        elif pattern == "cut_ties":
            s = np.sort(ln)[::-1]
            tied = np.flatnonzero(np.diff(s) == 0)
            assert tied.tolist() == list(range(mc.SORT_KMAX - 2, min(mc.SORT_KMAX + 1, m - 1)))
        else:
            lhs_decides = (arrived["lhs_end"].astype(np.int64) - arrived["lhs_begin"]) > (arrived["rhs_end"].astype(np.int64) - arrived["rhs_begin"])
            assert 0.3 * m < np.count_nonzero(lhs_decides) < 0.7 * m
    # libstdc++'s std::sort finishes lists of up to 16 by insertion alone, which is stable; above that its partitioning
    # moves equal lengths: a stable sort on the device cannot pass any of these
    for pattern in ("equal", "two", "sides"):
        for m in (17, 40, 100):
            assert differs[(m, pattern)], (m, pattern)
    assert differs[(40, "cut_ties")] or differs[(100, "cut_ties")] or differs[(17, "cut_ties")]
    assert not differs[(16, "equal")]

    killer = mc.by_name("sort:killer")
    ref = mc.reference("sort:killer")[0]
    assert killer["lengths"].shape[0] == 64  # one wave of truncate_sort_kernel
    want = (np.uint32(mc.KILLER_N + 5) - oracle.antiqsort(mc.KILLER_N)).astype(np.int64)
    for p, ln in zip(mc.KILLER_PILES, (want, want // 7)):
        arrived = np.array(_arrival(killer, 0, p), dtype=DT)
        # the list the sort sees is the adversary's sequence itself (plus a constant): nothing arrives before it
        assert np.array_equal(_lengths(arrived), ln + 48) and np.all(arrived["lhs_id"] == p)
        assert _list(ref, p).tolist() == oracle.truncate(arrived, 32).tolist()
        if p == mc.KILLER_PILES[1]:  # (the lengths of the first are all different: one order only)
            assert _list(ref, p).tolist() != _stable(arrived, 32).tolist()
    sizes = np.diff(ref["offsets"].astype(np.int64))
    arrived_sizes = np.array([len(_arrival(killer, 0, p)) for p in range(64)])
    others = np.delete(arrived_sizes, mc.KILLER_PILES)
    assert others.max() < 200 and np.count_nonzero(others >= 32) > 10 and np.count_nonzero((others > 0) & (others < 32)) > 10
    assert sizes.max() == 32

    deep = mc.by_name("sort:deep")
    ref = mc.reference("sort:deep")[0]
    p, cell = deep["claims"]["cell"]
    b, e = mc.events(deep["flushes"][0], p)
    assert b.shape[0] == mc.DEEP_N > 65535 and np.all(b <= cell) and np.all(e > cell) and len(deep["flushes"]) == 1
    assert int(_pile(ref, p)[cell]) == 65535 and int(_pile(ref, p)[cell - 1]) == 0
    assert _list(ref, p).shape[0] == 32


def test_tile_cases_place_what_they_say():
    case = mc.by_name("tiles:edges")
    f1, f2 = case["flushes"]
    cells = (case["lengths"] >> 4).tolist()[:-1]
    assert cells == list(mc.TILE_CELLS)
    assert {c for c in cells} >= {8191, 8192, 8193, 16384, 16385}
    assert {c % mc.TILE for c in cells} >= {1, 255, 256, 257}
    for p, n_cells in enumerate(cells):
        b, e = mc.events(f1, p)
        if p == mc.TILE_CARRY_PILE:  # tile 0 into tile 2: tile 1 has no event of its own
            assert b.tolist() == [100] and e.tolist() == [16500] and n_cells > 2 * mc.TILE + 116
            continue
        near = {x for x in (1, 8191, 8192, 8193, n_cells - 1) if x <= n_cells - 1}
        assert near <= set(b.tolist()) and near <= set(e.tolist()), p
        assert np.all(e <= n_cells - 1) and np.all(b >= 1)
        if n_cells > 8300:  # inside tile 1 only
            inside = (b // mc.TILE == 1) & (e // mc.TILE == 1) & (b % mc.TILE > 1) & (e - b > 50)
            assert inside.any()
        if n_cells > mc.TILE:  # ending exactly on the first cell of a tile, from the tile before
            assert np.any((e == mc.TILE) & (b < mc.TILE))
    ref = mc.reference("tiles:edges")
    # the carry pile: every cell of tile 1 holds 1 after flush 1 although no event falls into it
    carry = _pile(ref[0], mc.TILE_CARRY_PILE)
    assert np.all(carry[100:16500] == 1) and not carry[:100].any() and not carry[16500:].any()
    # flush 2 lies on top of flush 1
    for p in range(len(cells)):
        assert np.all(_pile(ref[1], p)[1:cells[p] - 1] == _pile(ref[0], p)[1:cells[p] - 1] + 1 +
                      ((np.arange(1, cells[p] - 1) >= mc.TILE - 1) & (np.arange(1, cells[p] - 1) < mc.TILE + 1) & (cells[p] > mc.TILE + 2)))

    wrap = mc.by_name("tiles:wrap")
    ref = mc.reference("tiles:wrap")
    for (f, p, c), v in wrap["claims"]["cells"].items():
        assert int(_pile(ref[f], p)[c]) == v, (f, p, c)
    for (f, p, c), v in wrap["claims"]["prior"].items():
        assert int(_pile(ref[f - 1], p)[c]) == v, (f, p, c)
    assert {v for v in wrap["claims"]["cells"].values()} >= {4, 65535, 65534, 0, 5}
    # the short overlaps really wrap in the reference: end event before begin event, inside a tile and across 8191 / 8192
    f2 = wrap["flushes"][1]
    for p in (mc.WRAP_FIVES, mc.WRAP_ZEROS):
        b, e = mc.events(f2, p)
        assert sorted(zip(e.tolist(), b.tolist())) == [(100, 101), (200, 202), (8191, 8193)]
    for p in (mc.WRAP_FIVES2, mc.WRAP_ZEROS2):
        b, e = mc.events(f2, p)
        assert sorted(zip(e.tolist(), b.tolist())) == [(0, 1), (8189, 8191), (8191, 8192), (mc.WRAP_CELLS - 1, mc.WRAP_CELLS)]
    # a wrap over a cell holding 0 saturates it; over 5 it takes one away
    assert int(_pile(ref[0], mc.WRAP_FIVES)[100]) == 5 and int(_pile(ref[1], mc.WRAP_FIVES)[100]) == 4
    assert int(_pile(ref[0], mc.WRAP_ZEROS)[100]) == 0 and int(_pile(ref[1], mc.WRAP_ZEROS)[100]) == 65535


# ---- the helpers -----------------------------------------------------------------------------------------------------

def test_diff_state_notices_each_kind_of_mistake():
    case = mc.by_name("tiles:edges")
    want = mc.reference("tiles:edges")[1]
    same = {k: v.copy() for k, v in want.items()}
    assert mc.diff_state(same, want) is None
    # two neighbouring entries of a list swapped
    bad = {k: v.copy() for k, v in want.items()}
    lo = int(want["offsets"][case["claims"]["sink"]])
    assert bad["overlaps"][lo] != bad["overlaps"][lo + 1]
    bad["overlaps"][[lo, lo + 1]] = bad["overlaps"][[lo + 1, lo]]
    assert "list of pile %d, entry 0" % case["claims"]["sink"] in mc.diff_state(bad, want)
    # an entry left unreversed
    bad = {k: v.copy() for k, v in want.items()}
    i = lo + 3
    bad["overlaps"][i] = np.array([mc.reverse(bad["overlaps"][i].tolist())], dtype=DT)[0]
    msg = mc.diff_state(bad, want)
    assert "entry 3" in msg and "lhs_id" in msg and "score" not in msg.split("differ:")[0]
    # one cell off at a tile edge
    for cell in (mc.TILE - 1, mc.TILE):
        bad = {k: v.copy() for k, v in want.items()}
        p = 2
        bad["data"][int(want["pile_offsets"][p]) + cell] += 1
        assert "pile 2, cell %d (tile %d, cell %d of it)" % (cell, cell // mc.TILE, cell % mc.TILE) in mc.diff_state(bad, want)
    # kept coverage added a second time
    ref = mc.MergeRef(case["lengths"], case["kmax"])
    ref.flush(case["flushes"][0])
    ref.counted = [0] * ref.n
    ref.flush(case["flushes"][1])
    assert "coverage of pile" in mc.diff_state(ref.state(), want)
    # a list one entry short, a shifted offset
    bad = {k: v.copy() for k, v in want.items()}
    bad["overlaps"] = bad["overlaps"][:-1]
    assert "entries" in mc.diff_state(bad, want)
    bad = {k: v.copy() for k, v in want.items()}
    bad["offsets"][3] += 1
    assert "offsets[3]" in mc.diff_state(bad, want)


def test_parts_and_offsets_helpers():
    flush = mc.by_name("order:kmax65")["flushes"][1]
    n = mc.by_name("order:kmax65")["lengths"].shape[0]
    off = mc.lhs_offsets(flush, n)
    assert off[0] == 0 and off[-1] == flush.shape[0]
    for q in range(n):
        assert np.all(flush["lhs_id"][int(off[q]):int(off[q + 1])] == q)
    for k in (1, 2, 5, 9):
        parts = mc.split_parts(flush, k)
        assert len(parts) == k and np.array_equal(np.concatenate(parts), flush)
        for a, b in zip(parts[:-1], parts[1:]):
            if a.shape[0] and b.shape[0]:
                assert a["lhs_id"][-1] < b["lhs_id"][0]
    assert any(p.shape[0] == 0 for p in mc.split_parts(flush, 9))  # more parts than queries: empty parts
    cut, pile = mc.boundary_between_feeders(flush)
    assert flush["lhs_id"][cut - 1] != flush["lhs_id"][cut]
    assert pile in flush["rhs_id"][:cut][flush["lhs_id"][:cut] == flush["lhs_id"][cut - 1]]
    assert pile in flush["rhs_id"][cut:][flush["lhs_id"][cut:] == flush["lhs_id"][cut]]
