"""The crafted piles of tests/pile_cases.py are what their tags claim — checked with the oracle alone
(oracle.pile_trim_and_median = the restatement of pile.cc:122-174, oracle.find_chimeric_regions = of pile.cc:176-187,
:373-400, :403-600), no GPU — so that tests/test_gpu_pile_annotate.py compares the kernels on inputs that do reach the
branches they were made for.  The thresholds below are conditions on the INPUTS: a generator that misses one is changed,
the threshold is not.  The host side of slopes.h (hip.test_find_chimeric_regions) runs over every chimeric case as well."""
from collections import Counter

import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip
from tests import pile_cases as pc


@pytest.fixture(scope="module")
def cases():
    data, offsets, tags = pc.generate()
    data.setflags(write=False)
    return data, offsets, tags


def _by_name(tags):
    names = [t["name"] for t in tags]
    assert len(set(names)) == len(names)
    return {n: i for i, n in enumerate(names)}


def _trim(cells, coverage):
    d = np.array(cells, dtype=np.uint16)
    return oracle.pile_trim_and_median(d, coverage), d


def test_generator_is_seeded_and_within_its_budget(cases):
    data, offsets, tags = cases
    again = pc.generate()
    assert np.array_equal(again[0], data) and np.array_equal(again[1], offsets) and again[2] == tags
    assert len(tags) == offsets.shape[0] - 1 and int(offsets[-1]) == data.shape[0] and data.dtype == np.uint16
    assert len(tags) <= 800 and data.shape[0] <= 500_000
    count = Counter(t["cls"] for t in tags)
    assert count["profile"] == 400 and count["random"] == 130 and count["pit"] == len(pc.PIT_CELLS) == 19
    assert count["wall"] == 80 and count["staircase"] >= 3 and count["median"] >= 30
    lengths = {int(offsets[i + 1] - offsets[i]) for i, t in enumerate(tags) if t["cls"] == "length"}
    assert lengths == {0, 1, 2, 63, 64, 65, 127, 128, 129, 4096, 8300}
    lengths = [int(offsets[i + 1] - offsets[i]) for i, t in enumerate(tags) if t["cls"] == "profile_long"]
    assert lengths == [4032, 4095, 4096, 4097, 4160, 6000]
    assert sorted(int(offsets[i + 1] - offsets[i]) for i, t in enumerate(tags) if t["cls"] == "random") == list(range(1, 131))


def test_trim_piles_have_the_region_they_were_built_for(cases):
    data, offsets, tags = cases
    n_claims = 0
    for i, t in enumerate(tags):
        if "trim" not in t:
            continue
        cells = pc.pile(data, offsets, i)
        (b, e, m, inv), after = _trim(cells, t["coverage"])
        assert (b, e, inv) == t["trim"], t["name"]
        if inv:
            assert m == 0 and np.array_equal(after, cells), t["name"]
        else:
            want = cells.copy()
            want[:b] = 0
            want[e:] = 0
            assert np.array_equal(after, want), t["name"]
        n_claims += 1
    assert n_claims >= 90  # every trim pile but the random-run ones, and every median pile
    at = _by_name(tags)
    # the issue's own figures for [0] + [5] * n + [0]
    for n, want in ((77, (0, 79, 0, True)), (78, (1, 79, 5, False)), (79, (1, 80, 5, False))):
        got, _ = _trim(pc.pile(data, offsets, at["run_length:%d" % n]), 4)
        assert got == want
        assert np.array_equal(pc.pile(data, offsets, at["run_length:%d" % n]), [0] + [5] * n + [0])
    # ties: the first of the longest runs, which is not the first run of all in two of the three piles
    assert tags[at["ties:two"]]["trim"] == (3, 93, False) and tags[at["ties:three"]]["trim"][0] == 83
    # every threshold occurs, with a valid and an invalid pile each
    for cov in pc.THRESHOLDS:
        got = {t["trim"][2] for t in tags if t["cls"] == "threshold" and t["coverage"] == cov}
        assert got == {False, True}, cov
    # run starts and terminators on the lanes around the chunk boundary
    assert {t["trim"][0] for t in tags if t["cls"] == "run_start"} == {0, 1, 63, 64, 65}
    assert {t["trim"][0] - 1 for t in tags if t["name"].startswith("run_end:then_valid")} == {63, 64, 65, 127, 128}
    assert {t["trim"][1] for t in tags if t["name"].startswith("run_end:valid")} == {127, 128}
    # the many-short-runs pile: 300 runs of 1 - 3 cells, several starts and ends inside every 64-cell chunk
    cells = pc.pile(data, offsets, at["short_runs:alone"]).astype(np.int64)
    ge = cells >= 4
    starts = np.flatnonzero(ge & ~np.concatenate([[False], ge[:-1]]))
    assert starts.shape[0] == 300 and all(np.count_nonzero(starts // 64 == c) >= 4 for c in range(int(starts[-1]) // 64))


def test_median_piles_have_the_stated_median(cases):
    data, offsets, tags = cases
    medians = {}
    for i, t in enumerate(tags):
        if t["kind"] != "median":
            continue
        (b, e, m, inv), _ = _trim(pc.pile(data, offsets, i), 4)
        assert (b, e, inv) == t["trim"] and not inv, t["name"]
        assert m == t["median"], t["name"]
        medians[t["name"][len("median:"):]] = m
    assert [medians["all_%d" % v] for v in (5, 255, 256, 257, 65535)] == [5, 255, 256, 257, 65535]
    assert (medians["255_256_even"], medians["255_256_odd_low"], medians["255_256_odd_high"]) == (256, 255, 256)
    for b in (0, 1, 2, 3, 252, 253, 254, 255):
        assert medians["low_byte_%d" % b] == 0x300 + b and medians["low_byte_%d_top" % b] == 65280 + b
        assert medians["high_byte_%d" % b] >> 8 == b
    # the median's high byte holds a minority of the region, and the region spans three high bytes
    at = _by_name(tags)
    for name in ("three_high_bytes", "minority_high_byte"):
        region = pc.pile(data, offsets, at["median:" + name])[1:-1]
        high = Counter((region >> 8).tolist())
        assert len(high) >= 3 and min(high) < medians[name] >> 8 < max(high)
    assert Counter((pc.pile(data, offsets, at["median:minority_high_byte"])[1:-1] >> 8).tolist())[2] * 4 < 100
    sizes = {int(offsets[at["median:random_%d" % n] + 1] - offsets[at["median:random_%d" % n]]) - 2 for n in (78, 79, 128, 4095)}
    assert sizes == {78, 79, 128, 4095}


def test_chimeric_piles_reach_what_they_were_built_for_and_the_host_hook_agrees(cases):
    data, offsets, tags = cases
    regions = {}
    for i, t in enumerate(tags):
        if t["kind"] != "chim":
            continue
        cells = pc.pile(data, offsets, i)
        want = oracle.find_chimeric_regions(cells)
        got = hip.test_find_chimeric_regions(cells)
        assert got.shape == want.shape and np.array_equal(got, want), t["name"]
        regions[t["name"]] = (want, cells.shape[0])
        if "regions" in t:  # the pit piles: what the issue states
            assert want.tolist() == t["regions"], t["name"]
    assert sum(1 for name, (r, _) in regions.items() if name.startswith("profile:") and r.shape[0]) >= 100
    # a region within 52 cells of each pile end
    assert any(r.shape[0] and int(r[0, 0]) < pc.WINDOW for r, _ in regions.values())
    assert any(r.shape[0] and int(r[-1, 1]) >= n - pc.WINDOW for r, n in regions.values())
    assert regions["pit:5"][0].tolist() == [[5, 6]] and regions["pit:%d" % (pc.PIT_LEN - 3)][0].tolist() == [[397, 398]]
    assert regions["pit:0"][0].shape[0] == 0 and regions["pit:%d" % (pc.PIT_LEN - 2)][0].shape[0] == 0
    # every wall pile has its two pits, the first starting on lane 0, the second ending on lane 63
    for w in range(1, 81):
        r = regions["wall:%d" % w][0]
        if w <= pc.WINDOW:
            assert r.tolist() == [[128, 127 + w], [384 - w, 383]], w
    # the long profiles are not flat
    assert all(regions["profile_long:%d" % n][0].shape[0] for n in (4095, 4096, 4097))
    # saturated cells: a 36008 beside 65535 is flagged, a 36009 is not
    assert regions["saturated:pits_36008"][0].shape[0] == 2 and regions["saturated:pits_36009"][0].shape[0] == 0


def test_staircases_fill_the_scratch_bound(cases):
    """About len / 2 runs of each kind in the first sweep: what the scratch of pile.hip (2 * len slope regions, len ups in
    the output scratch) is argued to hold."""
    data, offsets, tags = cases
    best = 0.0
    for i, t in enumerate(tags):
        if t["cls"] != "staircase":
            continue
        cells = pc.pile(data, offsets, i)
        down, up = pc.first_sweep_runs(cells)
        assert min(down, up) >= cells.shape[0] // 2 - 1, t["name"]
        best = max(best, min(down, up) / cells.shape[0])
    assert best >= 0.25
    assert {int(offsets[i + 1] - offsets[i]) for i, t in enumerate(tags) if t["cls"] == "staircase"} == {64, 128, 4096}


def test_near_integer_products(cases):
    data, offsets, tags = cases
    for i, t in enumerate(tags):
        if t["cls"] != "near_integer":
            continue
        cells = pc.pile(data, offsets, i).astype(np.int64)
        v = int(t["name"].split(":")[1].split("_")[0])
        assert abs(v * 1.82 - round(v * 1.82)) < 0.01 and round(v * 1.82) == v * 91 // 50
        assert set(cells.tolist()) == {v, v * 91 // 50 - 1, v * 91 // 50, v * 91 // 50 + 1}


def test_layers_rebuild_the_profile(cases):
    """pile_cases.layers_of: the intervals the product-library test feeds to AddLayers sum up to the profile."""
    data, offsets, tags = cases
    n = 0
    for i, t in enumerate(tags):
        cells = pc.pile(data, offsets, i)
        if cells.shape[0] < 3 or cells[0] or cells[-1] or int(np.abs(np.diff(cells.astype(np.int64))).sum()) > 8000:
            continue
        diff = np.zeros(cells.shape[0] + 1, dtype=np.int64)
        for x, y in pc.layers_of(cells):
            assert 1 <= x < y <= cells.shape[0] - 1
            diff[x] += 1
            diff[y] -= 1
        assert np.array_equal(np.cumsum(diff)[:-1], cells), t["name"]
        n += 1
    assert n >= 20


def test_device_hook_checks_its_arguments_before_it_needs_a_device():
    """rvn_test_piles_annotate: no piles is RVN_OK with empty outputs, a bad argument RVN_EINVAL — both before the hook
    makes its engine, so they hold on a machine without a GPU."""
    res = hip.test_piles_annotate(np.zeros(0, np.uint16), np.zeros(1, np.uint64))
    assert res["regions"] == [] and res["region_offsets"].tolist() == [0] and res["data"].shape == (0,)
    with pytest.raises(ValueError):
        hip.test_piles_annotate(np.zeros(4, np.uint16), np.array([0, 4, 2], np.uint64))  # descending offsets
    with pytest.raises(ValueError):
        hip.test_piles_annotate(np.zeros(4, np.uint16), np.array([0, 4], np.uint64), coverage=65536)
    with pytest.raises(ValueError):
        hip.test_piles_annotate(np.zeros(4, np.uint16), np.array([0, 4], np.uint64), per_thread=2)
