"""TrimAndAnnotatePiles on the device (raven_amd/csrc/pile.hip) on the crafted piles of tests/pile_cases.py, every comparison
for equality with the oracle's restatement of pile.cc (oracle.pile_trim_and_median, oracle.find_chimeric_regions):

  pile_trim_kernel           ballot scan over 64-cell chunks, zeroing, two-pass radix select of the median
  pile_chimeric_wave_kernel  the wave's first sweep of FindSlopes (LDS copy, doubling maxima, runs from ballots with state
                             carried across chunks, ups parked in the output scratch), one lane beyond 4096 cells
  pile_chimeric_kernel       one thread per pile (otherwise only behind RVN_CHIMERIC_PER_THREAD)

The piles reach these through hip.test_piles_annotate (rvn_test_piles_annotate: the functions the C ABI calls, on a CSR
given by the test); the last test builds some of them through the public ABI of libraven_hip.so as well and shows that
the product library computes the same.  tests/test_pile_cases.py (CPU) shows that the piles are what their tags say."""
import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip
from tests import pile_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    data, offsets, tags = pc.generate()
    data.setflags(write=False)
    offsets.setflags(write=False)
    return data, offsets, tags


@pytest.fixture(scope="module")
def trim_reference(cases):
    """threshold -> (begin, end, median, invalid, data after the trim) of EVERY pile, from the oracle."""
    data, offsets, tags = cases
    ref = {}
    for cov in pc.THRESHOLDS:
        after = data.copy()
        rows = [oracle.pile_trim_and_median(after[int(offsets[i]):int(offsets[i + 1])], cov) for i in range(len(tags))]
        after.setflags(write=False)
        ref[cov] = (np.array([r[0] for r in rows], np.uint32), np.array([r[1] for r in rows], np.uint32),
                    np.array([r[2] for r in rows], np.uint16), np.array([r[3] for r in rows], bool), after)
    return ref


def _oracle_regions(data, offsets):
    return [oracle.find_chimeric_regions(pc.pile(data, offsets, i)) if offsets[i + 1] > offsets[i] else np.zeros((0, 2), np.uint32)
            for i in range(offsets.shape[0] - 1)]


@pytest.fixture(scope="module")
def raw_regions(cases):
    """FindChimericRegions of every pile as given (no trim), from the oracle."""
    data, offsets, _ = cases
    return _oracle_regions(data, offsets)


@pytest.fixture(scope="module")
def trimmed_regions(cases, trim_reference):
    """... and of every pile after FindValidRegion(4), raven's order."""
    _, offsets, _ = cases
    return _oracle_regions(trim_reference[4][4], offsets)


def _same_regions(got, want, skip=None):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if skip is not None and skip[i]:
            assert g.shape[0] == 0, i
        else:
            assert g.shape == w.shape and np.array_equal(g, w), (i, g, w)


def _offsets_are_the_running_sum(res):
    counts = np.array([r.shape[0] for r in res["regions"]], dtype=np.int64)
    assert int(res["region_offsets"][0]) == 0 and np.array_equal(res["region_offsets"][1:], np.cumsum(counts))


@pytest.mark.parametrize("coverage", pc.THRESHOLDS)
def test_trim_and_median_match_the_oracle_at_every_threshold(cases, trim_reference, coverage):
    data, offsets, tags = cases
    wb, we, wm, winv, wafter = trim_reference[coverage]
    res = hip.test_piles_annotate(data, offsets, coverage=coverage)
    lens = np.diff(offsets.astype(np.int64))
    for i, t in enumerate(tags):
        got = (int(res["begin"][i]), int(res["end"][i]), int(res["median"][i]), bool(res["invalid"][i]))
        assert got == (int(wb[i]), int(we[i]), int(wm[i]), bool(winv[i])), (t["name"], coverage)
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        assert np.array_equal(res["data"][lo:hi], wafter[lo:hi]), (t["name"], coverage)
        if got[3]:  # an invalid pile is reported as the whole pile and keeps its data
            assert got[:3] == (0, int(lens[i]), 0) and np.array_equal(res["data"][lo:hi], data[lo:hi]), t["name"]
        if t.get("coverage") == coverage:  # what the pile was built for
            if "trim" in t:
                assert (got[0], got[1], got[3]) == t["trim"], t["name"]
            if "median" in t:
                assert got[2] == t["median"], t["name"]
    assert np.count_nonzero(res["invalid"]) > 50 and np.count_nonzero(~res["invalid"]) > (50 if coverage <= 4 else 2)
    # a region that ends before the pile's end is now terminated by a zeroed cell: the trim finds it again
    again = hip.test_piles_annotate(res["data"], offsets, coverage=coverage)
    ok = ~res["invalid"] & (res["end"].astype(np.int64) < lens)
    assert np.count_nonzero(ok) >= 2
    for key in ("begin", "end", "median"):
        assert np.array_equal(again[key][ok], res[key][ok]), key
    assert not again["invalid"][ok].any() and np.array_equal(again["data"], res["data"])


@pytest.mark.parametrize("n", pc.PILE_COUNTS)
def test_pile_counts_that_leave_waves_of_the_last_block_idle(cases, trim_reference, trimmed_regions, n):
    """pile_trim_kernel runs four piles per block: n = 1, 3, 5, 257 leave waves without a pile."""
    data, offsets, tags = cases
    # the piles with something to trim first, so that small n see valid piles too
    first = [i for i, t in enumerate(tags) if t["cls"] in ("run_start", "ties", "median")]
    order = first + [i for i in range(len(tags)) if i not in set(first)]
    idx = order[:n]
    d, off = pc.pick(data, offsets, idx)
    res = hip.test_piles_annotate(d, off, coverage=4)
    wb, we, wm, winv, wafter = trim_reference[4]
    assert np.array_equal(res["begin"], wb[idx]) and np.array_equal(res["end"], we[idx])
    assert np.array_equal(res["median"], wm[idx]) and np.array_equal(res["invalid"], winv[idx])
    assert np.array_equal(res["data"], pc.pick(wafter, offsets, idx)[0])
    assert not res["invalid"][0]
    _same_regions(res["regions"], [trimmed_regions[i] for i in idx], skip=winv[idx])
    _offsets_are_the_running_sum(res)


def test_no_piles_and_piles_without_cells():
    for per_thread in (False, True):
        res = hip.test_piles_annotate(np.zeros(0, np.uint16), np.zeros(1, np.uint64), per_thread=per_thread)
        assert res["regions"] == [] and res["region_offsets"].tolist() == [0] and res["begin"].shape == (0,)
        res = hip.test_piles_annotate(np.zeros(0, np.uint16), np.zeros(4, np.uint64), per_thread=per_thread)
        assert res["begin"].tolist() == [0, 0, 0] and res["end"].tolist() == [0, 0, 0] and res["median"].tolist() == [0, 0, 0]
        assert res["invalid"].all() and res["region_offsets"].tolist() == [0, 0, 0, 0]
        assert all(r.shape == (0, 2) for r in res["regions"])
    # empty piles between others: nothing of theirs is read or written
    d = np.full(400, 40, np.uint16)
    d[200:202] = 3
    res = hip.test_piles_annotate(np.concatenate([d, d]), np.array([0, 0, 400, 400, 800, 800], np.uint64), skip_trim=True)
    assert [r.tolist() for r in res["regions"]] == [[], [[200, 201]], [], [[200, 201]], []]


@pytest.mark.parametrize("per_thread", [False, True], ids=["wave", "one_thread"])
def test_chimeric_regions_of_the_raw_piles_match_the_oracle(cases, raw_regions, per_thread):
    """Every pile as given (skip_trim): both kernels, the host side of slopes.h and the oracle give the same regions."""
    data, offsets, tags = cases
    res = hip.test_piles_annotate(data, offsets, per_thread=per_thread, skip_trim=True)  # (raises on the overflow flag)
    _same_regions(res["regions"], raw_regions)
    _offsets_are_the_running_sum(res)
    for i, t in enumerate(tags):
        if "regions" in t:  # the pits at the ends, at the window's width and at the chunk boundaries
            assert res["regions"][i].tolist() == t["regions"], t["name"]
        if t["kind"] == "chim":
            host = hip.test_find_chimeric_regions(pc.pile(data, offsets, i))
            assert host.shape == res["regions"][i].shape and np.array_equal(host, res["regions"][i]), t["name"]
    assert sum(r.shape[0] for r in res["regions"]) > 3000


@pytest.mark.parametrize("per_thread", [False, True], ids=["wave", "one_thread"])
def test_invalid_piles_get_no_region_and_leave_their_neighbours_alone(cases, raw_regions, per_thread):
    data, offsets, tags = cases
    for phase in (0, 1):
        invalid = (np.arange(len(tags)) % 2 == phase)
        res = hip.test_piles_annotate(data, offsets, per_thread=per_thread, skip_trim=True, invalid=invalid)
        _same_regions(res["regions"], raw_regions, skip=invalid)
        _offsets_are_the_running_sum(res)


@pytest.mark.parametrize("per_thread", [False, True], ids=["wave", "one_thread"])
def test_chimeric_regions_after_the_trim_match_the_oracle(cases, trim_reference, trimmed_regions, per_thread):
    """raven's order: FindValidRegion(4) first, FindChimericRegions of the valid piles on the zeroed data."""
    data, offsets, tags = cases
    res = hip.test_piles_annotate(data, offsets, coverage=4, per_thread=per_thread)
    winv = trim_reference[4][3]
    assert np.array_equal(res["invalid"], winv) and np.array_equal(res["data"], trim_reference[4][4])
    _same_regions(res["regions"], trimmed_regions, skip=winv)
    _offsets_are_the_running_sum(res)
    assert sum(r.shape[0] for r in res["regions"]) > 200 and 50 < np.count_nonzero(winv) < len(tags) - 50


@pytest.mark.parametrize("per_thread", [False, True], ids=["wave", "one_thread"])
def test_a_pile_beyond_the_lds_limit_before_a_pile_of_one_cell(cases, raw_regions, per_thread):
    data, offsets, tags = cases
    at = {t["name"]: i for i, t in enumerate(tags)}
    for names in (("profile_long:4097", "random:1"), ("random:1", "profile_long:4096", "profile_long:4097", "random:2"),
                  ("staircase:4096", "profile_long:4095", "staircase:64")):
        idx = [at[x] for x in names]
        d, off = pc.pick(data, offsets, idx)
        res = hip.test_piles_annotate(d, off, per_thread=per_thread, skip_trim=True)
        _same_regions(res["regions"], [raw_regions[i] for i in idx])
        _offsets_are_the_running_sum(res)


def test_the_product_library_computes_the_same(cases):
    """The same coverage built through the public ABI of libraven_hip.so: every profile whose first and last cell are 0 is
    the sum of intervals of cells [x, y), each realised as an overlap with begin = (x - 1) * 16, end = (y + 1) * 16 on the
    pile under test (Pile::AddLayers covers [(begin >> 4) + 1, (end >> 4) - 1)) and as rhs on one long sink pile.  Then
    Pass1.trim_and_annotate and Pass1.find_chimeric_regions must return what the hook and the oracle return."""
    data, offsets, tags = cases
    idx, budget, n_profiles = [], 60_000, 0
    for i, t in enumerate(tags):
        cells = pc.pile(data, offsets, i)
        if cells.shape[0] < 3 or cells[0] or cells[-1]:
            continue
        rises = int(np.abs(np.diff(cells.astype(np.int64))).sum()) // 2
        if rises == 0 or rises > 4000 or rises > budget or (t["cls"] == "profile" and n_profiles >= 20):
            continue
        n_profiles += t["cls"] == "profile"
        budget -= rises
        idx.append(i)
    names = {tags[i]["name"] for i in idx}
    assert "plateau:300" in names and "run_length:77" in names and "run_length:78" in names and n_profiles == 20
    assert len(idx) >= 40
    d, off = pc.pick(data, offsets, idx)
    sink = len(idx)
    lengths = np.append(np.diff(off.astype(np.int64)) * 16, int(np.diff(off.astype(np.int64)).max()) * 16 + 64).astype(np.uint32)
    layers = [(k, x, y) for k in range(sink) for x, y in pc.layers_of(pc.pile(d, off, k))]
    ovl = np.zeros(len(layers), dtype=hip.OVERLAP_DTYPE)
    lay = np.array(layers, dtype=np.int64)
    ovl["lhs_id"], ovl["rhs_id"] = lay[:, 0], sink
    ovl["lhs_begin"] = ovl["rhs_begin"] = (lay[:, 1] - 1) * 16
    ovl["lhs_end"] = ovl["rhs_end"] = (lay[:, 2] + 1) * 16
    ovl["strand"] = 1
    eng = hip.Engine(15, 5)
    p = eng.shard_piles_create(lengths)
    p.merge(ovl)  # (already in lhs order)
    built, boff = p.piles()
    assert np.array_equal(boff[:sink + 1], off) and np.array_equal(built[:int(off[-1])], d)
    assert int(built.max()) >= 300
    b, e, m, inv = p.trim_and_annotate(4)
    after, _ = p.piles()
    regions = p.find_chimeric_regions(inv)
    p.close()
    eng.close()
    hook = hip.test_piles_annotate(built, boff, coverage=4)
    for key, got in (("begin", b), ("end", e), ("median", m), ("invalid", inv), ("data", after)):
        assert np.array_equal(hook[key], got), key
    _same_regions(regions, hook["regions"])
    want = built.copy()
    for k in range(sink + 1):
        row = oracle.pile_trim_and_median(want[int(boff[k]):int(boff[k + 1])], 4)
        assert (int(b[k]), int(e[k]), int(m[k]), bool(inv[k])) == row, k
        if not row[3]:
            w = oracle.find_chimeric_regions(want[int(boff[k]):int(boff[k + 1])])
            assert regions[k].shape == w.shape and np.array_equal(regions[k], w), k
        else:
            assert regions[k].shape[0] == 0
    assert np.array_equal(after, want)
    assert int(m.max()) >= 300 and 5 < np.count_nonzero(inv) < sink - 5 and sum(r.shape[0] for r in regions) >= 5
