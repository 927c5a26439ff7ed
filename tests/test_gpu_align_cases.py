"""The alignment-path stage ON THE DEVICE on the crafted pairs of tests/align_cases.py: nw_sweep_kernel<R, G> in its eight
variants and striped, the three walk kernels, nw_path_count / _pack / _expand, and the host schedule around them
(thresholds, the early retry, the repeat passes, the rate handed from call to call), through rvn_test_align_path_batch
(HookEngine.align_paths).  Everything is compared for equality — distances, offsets, run words, op bytes with the DP
reference; the job's final plan, the six counters of NwStats and the launches of the two kernel sites with the prediction.
No tolerance anywhere.  Thresholds are pinned by RVN_NW_RATE, which the test library reads at every call.

Which of the three walk kernels a launch took is not observable from the counts (every walk is one launch of the site
nw_traceback): the walk_size cases hold the RESULTS on both sides of the two sizes where launch_walk_to changes the kernel,
and the nw_group_walk = 1 / 2 / 3 runs of the other families force each kernel in turn."""
import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip
from tests import align_cases as A
from tests import nw_ops_util as U

pytestmark = pytest.mark.gpu

NOT_ALIGNED = 0xFFFFFFFF
GUARD = 64
WALKS = (0, 1, 2, 3)  # engine option nw_group_walk: by size / lane, whole strips / group of lanes / lane, strips of sixteen


@pytest.fixture(scope="module")
def eng():
    e = hip.HookEngine(15)
    yield e
    e.close()


def _align(e, reads, rows, ops=False, guard=0, options=()):
    """one call on a read set of its own, launches counted: (dist, off, words, n_bad, plans, stats, launches)"""
    both = e.upload_codes(reads)
    for name, value in options:
        e.set_option(name, value)
    try:
        e.count_launches()
        got = e.align_paths(both, both, np.array(rows, dtype=hip.ALIGN_PAIR_DTYPE), ops=ops, guard=guard)
        la = e.launches()
    finally:
        e.count_launches(False)
        for name, _ in options:
            e.set_option(name, 0)
        e.reads_destroy(both)
    return got + (la,)


def hold(e, monkeypatch, cases, rate, strands=(1, 0), options=(), what="", both_forms=False):
    """the batch of `cases` equals its references, its plans and counters the prediction; returns the call's stats (and
    under "plans" what the device reported per pair)"""
    monkeypatch.setenv("RVN_NW_RATE", repr(float(rate)))
    reads, rows, items = A.batch(cases, strands)
    dist, off, runs, op_off, ops = A.expected(items)
    stripe_lanes = dict(options).get("nw_stripe_lanes", 0) or A.ALL_LANES
    jobs = [(c.n, c.m, int(d)) for c, d in zip(items, dist)]
    stats = None
    for form in ((False, True) if both_forms else (False,)):
        plans, want_stats, want_launches = A.predict(jobs, rate, stripe_lanes=stripe_lanes, ops=form)
        g_dist, g_off, g_words, n_bad, g_plans, stats, la = _align(e, reads, rows, ops=form, guard=GUARD, options=options)
        n_w = len(ops) if form else len(runs)
        # nothing behind the last offset, run word or op byte
        assert (g_off[len(items) + 1:] == 0xA5A5A5A5A5A5A5A5).all() and len(g_words) == n_w + GUARD, what
        assert (g_words[n_w:] == (0xA5 if form else 0xA5A5A5A5)).all(), what
        A.compare((g_dist, g_off[:len(items) + 1], g_words[:n_w]), (dist, op_off if form else off, ops if form else runs), what)
        assert n_bad == 0
        A.compare_plans(g_plans, plans, what)
        A.compare_counters(stats, la, want_stats, want_launches, what)
        stats["plans"] = g_plans
    return stats


def _walk(gw):
    return (("nw_group_walk", gw),) if gw else ()


STRIPE4 = (("nw_stripe_lanes", 4),)


# ---- threshold -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [_walk(g) for g in WALKS] + [STRIPE4], ids=["walk0", "walk1", "walk2", "walk3", "stripe4"])
def test_threshold(eng, monkeypatch, options):
    """rate 0, k0 = max(16, |n - m|): distance k is accepted, k + 1 repeated; paths on the band's outermost diagonals
    (k == |n - m| included); distance 200 climbs 16 -> 256 (the first repeat in the early retry's compact pass)"""
    cases = A.threshold_cases()
    st = hold(eng, monkeypatch, cases, 0.0, options=options, what="threshold")
    by_dist = {15: 0, 16: 0, 17: 1, 32: 1, 33: 2, 64: 2, 65: 3, 40: 0, 200: 4}
    assert st["n_retries"] == 2 * sum(by_dist[c.meta["dist"]] for c in cases)  # (both strands)
    assert st["n_batches"] == 5 and st["n_unaligned"] == 0
    last = tuple(int(v) for v in st["plans"][-1][[0, 2, 3, 4]])  # (k, R, G, S) of the pair of distance 200
    assert last == ((256, 8, 64, 4) if options == STRIPE4 else (256, 1, 8, 0))  # beyond (1, 4): stripes of four lanes


# ---- ring size and variant -------------------------------------------------------------------------------------------------
def _ring(level, dp):
    return [c for c in A.ring_edge_cases() if c.meta["level"] == level and (c.name not in A.NO_DP_CASES) == dp]


@pytest.mark.parametrize("gw", WALKS)
@pytest.mark.parametrize("level", range(8))
def test_ring_edge(eng, monkeypatch, level, gw):
    """k = n + m: the smallest and the largest pair of each variant (the ring of exactly G lanes), n = m, n > m, n < m; no
    job repeats, so one batch and no early retry"""
    cases = _ring(level, True)
    st = hold(eng, monkeypatch, cases, A.RATE_LARGE, options=_walk(gw), what="ring_edge %d" % level)
    assert st["n_batches"] == 1 and st["n_retries"] == 0
    for c, p in zip(cases, st["plans"][::2]):  # (two strands a case)
        assert (int(p[0]), int(p[2]), int(p[3]), int(p[4])) == (c.n + c.m,) + c.meta["variant"] + (0,), c


@pytest.fixture(scope="module")
def beyond_dp_distances():
    cases = _ring(7, False) + [c for c in A.ring_below_cases() if c.name in A.NO_DP_CASES]
    assert sorted(c.name for c in cases) == sorted(A.NO_DP_CASES) and len(cases) <= 4
    return {c.name: oracle.edit_distance(bytes(c.q), bytes(c.t)) for c in cases}


def _hold_without_dp(e, monkeypatch, c, rate, dist, options):
    monkeypatch.setenv("RVN_NW_RATE", repr(float(rate)))
    reads, rows, items = A.batch([c], (1, 0))
    plans, want_stats, want_launches = A.predict([(c.n, c.m, dist)] * 2, rate)
    g_dist, g_off, g_runs, n_bad, g_plans, stats, la = _align(e, reads, rows, options=options)
    assert n_bad == 0 and g_dist.tolist() == [dist, dist]
    for p in range(2):
        r = g_runs[int(g_off[p]):int(g_off[p + 1])]
        U.check_runs(r, c.q, c.t, dist)
        assert A.replay(r, c.q, c.t) == dist
    A.compare_plans(g_plans, plans, c.name)
    A.compare_counters(stats, la, want_stats, want_launches, c.name)
    return g_plans


@pytest.mark.parametrize("gw", WALKS)
def test_ring_edge_beyond_the_dp(eng, monkeypatch, beyond_dp_distances, gw):
    """The upper edge of (8, 64) — pairs of 16 160 bases, 261 M cells — held to the oracle's distance, check_runs and a
    replay of the runs on the bases: optimal, tie choices unchecked (align_cases.NO_DP_CASES: at most 4 pairs)."""
    for c in _ring(7, False):
        plans = _hold_without_dp(eng, monkeypatch, c, A.RATE_LARGE, beyond_dp_distances[c.name], _walk(gw))
        assert tuple(int(v) for v in plans[0][[0, 2, 3, 4]]) == (c.n + c.m, 8, 64, 0)


@pytest.mark.parametrize("gw", WALKS)
def test_ring_boundary_from_below(eng, monkeypatch, beyond_dp_distances, gw):
    """a related pair and a rate with floor(rate * len) + 16 = kcap (the ring full, the band narrow) and kcap + 1 (the
    next variant)"""
    for c in A.ring_below_cases():
        if c.name in A.NO_DP_CASES:
            plans = _hold_without_dp(eng, monkeypatch, c, c.meta["rate"], beyond_dp_distances[c.name], _walk(gw))
        else:
            plans = hold(eng, monkeypatch, [c], c.meta["rate"], options=_walk(gw), what=c.name)["plans"]
        assert (int(plans[0][0]), int(plans[0][2]), int(plans[0][3])) == (c.meta["k"],) + c.meta["variant"], c


# ---- bundles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [_walk(g) for g in WALKS] + [STRIPE4], ids=["walk0", "walk1", "walk2", "walk3", "stripe4"])
@pytest.mark.parametrize("G", (4, 8, 16, 32))
def test_bundle(eng, monkeypatch, G, options):
    """jobs of one variant, 1 to 2 * 64/G + 1 of them, columns from 1 to the variant's most in ONE bundle: each job's runs
    are those of the job alone (its reference) in any pair order — a neighbour's stores never reach it"""
    for name, cases in A.bundle_batches(G):
        st = hold(eng, monkeypatch, cases, A.RATE_LARGE, strands=(1,), options=options, what=name)
        assert st["n_batches"] == 1
    hold(eng, monkeypatch, A.bundle_pool(G)[:64 // G + 1], A.RATE_LARGE, strands=(0,), options=options, what="G%d strand 0" % G)


# ---- slots ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gw", WALKS)
def test_slots_filled_to_the_first_word(eng, monkeypatch, gw):
    """2k + 1 runs in a slot of 2k + 2 words (k = 16; 32 after one repeat), three such pairs in a row, first and last"""
    for name, cases in A.slot_batches():
        hold(eng, monkeypatch, cases, 0.0, options=_walk(gw), what=name, both_forms=True)


# ---- repeats -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gw", WALKS)
def test_repeats_beyond_the_early_retry(eng, monkeypatch, gw):
    """4 200 pairs of distance 20 at k0 = 16: 4 096 repeat in the early retry's compact pass, 104 in the ordinary one"""
    distinct = A.small_distinct(64, 40, 41, 20, seed=4200)
    cases = [distinct[x % 64] for x in range(4200)]
    st = hold(eng, monkeypatch, cases, 0.0, strands=(1,), options=_walk(gw), what="repeats")
    assert st["n_retries"] == 4200 and st["n_batches"] == 3 and st["n_aligned"] == 4200


@pytest.fixture(scope="module")
def chunked_repeat_distances():
    return [oracle.edit_distance(bytes(c.q), bytes(c.t)) for c in A.chunked_repeat_cases()]


@pytest.mark.parametrize("gw", WALKS)
def test_repeats_handed_back_by_the_early_retry(eng, monkeypatch, chunked_repeat_distances, gw):
    """60 pairs of ~6 000 bases under nw_budget_mb = 64, all beyond their first threshold: the doubled bands exceed buffer
    set 3's twelfth of the budget, the early retry takes what fits and hands the others on, which the pass behind it
    doubles once more (and cuts in two chunks).  3 pairs word for word, the others by distance and a replay of their runs."""
    cases = A.chunked_repeat_cases()
    rate = cases[0].meta["rate"]
    dist = chunked_repeat_distances
    plans, want_stats, want_launches = A.predict([(c.n, c.m, d) for c, d in zip(cases, dist)], rate, budget=64 << 20)
    times = [p[0] // A.threshold(rate, c.n, c.m) for p, c in zip(plans, cases)]
    assert sorted(set(times)) == [2, 4] and want_stats["n_retries"] == 60 and want_stats["n_batches"] == 4
    monkeypatch.setenv("RVN_NW_RATE", repr(rate))
    reads, rows, items = A.batch(cases, (1,))
    g_dist, g_off, g_runs, n_bad, g_plans, stats, la = _align(eng, reads, rows, options=(("nw_budget_mb", 64),) + _walk(gw))
    assert n_bad == 0 and g_dist.tolist() == dist
    A.compare_plans(g_plans, plans, "chunked repeats")
    A.compare_counters(stats, la, want_stats, want_launches, "chunked repeats")
    by_dp = (times.index(2), times.index(4), 59)
    for p, c in enumerate(cases):
        r = g_runs[int(g_off[p]):int(g_off[p + 1])]
        if p in by_dp:
            assert A.reference(c)[0] == dist[p] and np.array_equal(r, A.reference(c)[1]), c
        else:
            U.check_runs(r, c.q, c.t, dist[p])
            assert A.replay(r, c.q, c.t) == dist[p], c


# ---- path kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gw", WALKS)
def test_path_kernels(eng, monkeypatch, gw):
    """runs per pair 0, 1, 3, 63 .. 65, 255 .. 257, 513, one run of 70 000 ops, 256 single ops before one run of 5 000:
    runs, ops, both offset arrays, nothing written behind the last element"""
    hold(eng, monkeypatch, A.path_kernel_cases(), 0.0, options=_walk(gw), what="path", both_forms=True)


def test_path_kernels_around_a_pair_that_is_not_aligned(eng, monkeypatch):
    """nw_stripe_lanes = 1: an unrelated pair of 8 000 bases is beyond eight stripes; no runs, no ops, neighbours whole"""
    rng = np.random.default_rng(8000)
    far = A.Case("path_not_aligned", A.rnd(rng, 8000), A.rnd(rng, 8000))
    d_far = oracle.edit_distance(bytes(far.q), bytes(far.t))
    cases = [c for c in A.path_kernel_cases() if c.n <= 1000]
    cases = cases[:6] + [far] + cases[6:]
    monkeypatch.setenv("RVN_NW_RATE", "0")
    reads, rows, items = A.batch(cases, (1, 0))
    where = [p for p, c in enumerate(items) if c is far]
    near = [c if c is not far else A.Case("path_empty_both", [], []) for c in items]  # (what it leaves: nothing)
    dist, off, runs, op_off, ops = A.expected(near)
    dist[where] = NOT_ALIGNED
    jobs = [(c.n, c.m, d_far if c is far else int(d)) for c, d in zip(items, dist)]
    options = (("nw_stripe_lanes", 1),)
    for form in (False, True):
        plans, want_stats, want_launches = A.predict(jobs, 0.0, stripe_lanes=1, ops=form)
        assert [p for p, f in enumerate(plans) if f is None and items[p].cells] == where
        g_dist, g_off, g_words, n_bad, g_plans, stats, la = _align(eng, reads, rows, ops=form, guard=GUARD, options=options)
        n_w = len(ops) if form else len(runs)
        assert n_bad == 2 and (g_words[n_w:] == (0xA5 if form else 0xA5A5A5A5)).all() and len(g_words) == n_w + GUARD
        A.compare((g_dist, g_off[:len(items) + 1], g_words[:n_w]), (dist, op_off if form else off, ops if form else runs), "stripe 1")
        A.compare_plans(g_plans, plans, "stripe 1")
        A.compare_counters(stats, la, want_stats, want_launches, "stripe 1")


# ---- walk sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pairs", (8192, 8193, 65536, 65537))
def test_walk_size(eng, monkeypatch, n_pairs):
    """one pass of n_pairs small jobs: up to 8 192 the group walk, up to 65 536 the lane walk with whole strips, beyond it
    strips of sixteen columns — one walk launch each; which kernel it was does not show in the counts, the results do"""
    distinct = A.small_distinct(64, 24, 41, None, seed=6464)
    monkeypatch.setenv("RVN_NW_RATE", "1.0")
    reads, rows, items = A.batch(distinct, (1,))
    pick = np.arange(n_pairs) % 64
    dist, off, runs, _, _ = A.expected([items[int(x)] for x in pick])
    plans, want_stats, want_launches = A.predict([(items[int(x)].n, items[int(x)].m, int(d)) for x, d in zip(pick, dist)], 1.0)
    g_dist, g_off, g_runs, n_bad, g_plans, stats, la = _align(eng, reads, [rows[int(x)] for x in pick])
    assert n_bad == 0
    A.compare((g_dist, g_off, g_runs), (dist, off, runs), "walk_size")
    A.compare_counters(stats, la, want_stats, want_launches, "walk_size")
    assert la["nw_traceback"] == 3 and stats["n_batches"] == 1 and stats["n_retries"] == 0


# ---- rate ----------------------------------------------------------------------------------------------------------------
def _hold_at_rate(e, cases, rate):
    reads, rows, items = A.batch(cases, (1,))
    dist, off, runs, _, _ = A.expected(items)
    plans, want_stats, want_launches = A.predict([(c.n, c.m, int(d)) for c, d in zip(items, dist)], rate)
    g_dist, g_off, g_runs, n_bad, g_plans, stats, la = _align(e, reads, rows)
    assert n_bad == 0
    A.compare((g_dist, g_off, g_runs), (dist, off, runs), "rate %r" % rate)
    A.compare_plans(g_plans, plans, "rate %r" % rate)
    A.compare_counters(stats, la, want_stats, want_launches, "rate %r" % rate)


def test_rate_is_handed_from_call_to_call(monkeypatch):
    """0.13 on a fresh engine; after a call that aligned >= 32 pairs the order statistic of nw_next_rate; after one of 31
    pairs the rate stays"""
    monkeypatch.delenv("RVN_NW_RATE", raising=False)
    first, second, few = A.rate_cases(40, 1), A.rate_cases(40, 2), A.rate_cases(31, 3)
    e = hip.HookEngine(15)
    try:
        _hold_at_rate(e, first, 0.13)
        rate1 = A.next_rate(first, 0.13)
        assert rate1 != 0.13
        _hold_at_rate(e, second, rate1)
        rate2 = A.next_rate(second, rate1)
        _hold_at_rate(e, few, rate2)
        assert A.next_rate(few, rate2) == rate2
        _hold_at_rate(e, first, rate2)
    finally:
        e.close()


# ---- the product library ---------------------------------------------------------------------------------------------------
def test_product_library_agrees(monkeypatch):
    """a subset of every family through libraven_hip.so (Engine.align_paths) on a fresh engine at its own rate"""
    monkeypatch.delenv("RVN_NW_RATE", raising=False)
    full, ordinary = A.slot_cases()
    cases = (list(A.threshold_cases()) + [c for c in A.ring_edge_cases() if c.cells <= 5_000_000 and c.meta["edge"] == "high"] +
             list(A.bundle_pool(4)[:17]) + list(A.bundle_pool(32)[:3]) + list(full.values()) + ordinary +
             list(A.path_kernel_cases()) + list(A.small_distinct(64, 40, 41, 20, seed=4200)[:8]) + list(A.small_distinct(64, 24, 41, None, seed=6464)[:8]) +
             list(A.rate_cases(40, 1)[:4]))
    reads, rows, items = A.batch(cases, (1, 0))
    dist, off, runs, op_off, ops = A.expected(items)
    e = hip.Engine(15, 5)
    try:
        both = e.upload_codes(reads)
        pairs = np.array(rows, dtype=hip.ALIGN_PAIR_DTYPE)
        g = e.align_paths(both, both, pairs)
        assert g[3] == 0
        A.compare(g[:3], (dist, off, runs), "product, runs")
        g = e.align_paths(both, both, pairs, ops=True)
        A.compare(g[:3], (dist, op_off, ops), "product, ops")
    finally:
        e.close()
