"""GPU: what lies between the sketch and the chain stage of Map — the device-wide radix sort and scans (radix_sort.hip,
scan.hip), the index's runs, bucket table, direct-address table and Filter (index.hip), and the match stage of map.hip
(match_count_kernel / match_emit_kernel / index_find, join_kernel) — against the numpy reference of tests/match_util.py on
crafted minimizer streams, at the tile, block and bin boundaries of that code.

Index, Filter and join cases go through the C ABI (shard_index_build, index_content, shard_key_counts,
shard_key_histogram, filter, set_occurrence, shard_join); probe, sort and scan cases through the hooks of
libraven_hip_test.so (rvn_test_match_probe, rvn_test_radix_sort_pairs, rvn_test_exclusive_scan).  Everything compares
integers for equality, order included; the one multiset comparison is the order of a read's matches inside its segment
of the join, which map.hip documents as arbitrary.  tests/test_match_reference.py holds the reference to the oracle on
real sketches and checks that the generators build what the cases here are named after.

Left out on purpose: the cap of 26 table bits (index.hip: index_table_impl) needs 2^25 distinct keys.
"""
import numpy as np
import pytest

from raven_amd import hip
from tests import match_util as mu

pytestmark = pytest.mark.gpu

TILE = 4096  # items per block of the radix sort and of the scans
SIZES = [0, 1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 1, 70_000]
KS = [5, 15, 16, 17, 31]  # 10-, 30- and 32-bit keys in 32-bit words, 34- and 62-bit keys in 64-bit words
FLAGS = [(ae, asym) for ae in (False, True) for asym in (False, True)]
_fid = lambda p: "equal%d-symmetric%d" % p


@pytest.fixture(scope="module")
def gpu():
    if hip.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return True


@pytest.fixture(scope="module")
def engines(gpu):
    """k -> engine, made once per module."""
    made = {}

    def get(k):
        if k not in made:
            made[k] = hip.Engine(k, 5)
        return made[k]

    yield get
    for he in made.values():
        he.close()


def _build_and_compare(he, values, origins, all_query=False):
    """The index of a stream == the reference's: sorted values, origins in stable order, distinct keys, member counts.
    (rvn_engine_index_fetch hands the origins back without their two flag bits; what the flags do is seen in the key
    counts, the histogram and the join.)"""
    ref = mu.sort_index(values, origins)
    he.shard_index_build(values, origins, all_query)
    v, o, u = he.index_content()
    errs = mu.diff_index(v, o, u, ref._replace(origins=ref.origins & ~(mu.QUERY_FLAG | mu.FOREIGN_FLAG)))
    errs += mu.diff_arrays("key counts", he.shard_key_counts(), ref.members)
    assert errs == [], errs[:4]
    return ref


# ---- sort and runs ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", mu.SORT_PATTERNS)
@pytest.mark.parametrize("k", KS)
def test_index_is_the_stable_sort(engines, k, pattern):
    """index_content() == stable sort of the stream, for every size around the sort's tile: the origins of a run come out
    in (read, position) order.  The index sorts with skip_constant_digits = false: constant digits are real passes."""
    for n in SIZES:
        _build_and_compare(engines(k), *mu.sort_stream(pattern, n, k, seed=n))


def _sort_reference(keys, values, bits):
    order = np.argsort(keys & np.uint64((1 << bits) - 1), kind="stable")
    return keys[order], values[order]


@pytest.mark.parametrize("skip", [False, True], ids=["all_digits", "skip_constant"])
@pytest.mark.parametrize("variant,bits", [("u32_u64", 10), ("u32_u64", 30), ("u32_u64", 32), ("u32_u32", 10),
                                          ("u32_u32", 30), ("u32_u32", 32), ("u64_u64", 34), ("u64_u64", 62)])
def test_radix_sort_pairs(gpu, variant, bits, skip):
    """The three instantiations on the same sizes and patterns, constant digits skipped and not."""
    errs = []
    for pattern in mu.SORT_PATTERNS:
        for n in SIZES:
            keys = mu.sort_keys(pattern, n, bits, seed=n)
            vals = mu.serial_origins(n) if variant != "u32_u32" else np.arange(n, dtype=np.uint64) * np.uint64(3)
            gk, gv = hip.test_radix_sort_pairs(variant, keys, vals, bits, skip)
            wk, wv = _sort_reference(keys, vals, bits)
            e = mu.diff_arrays("keys", gk, wk) + mu.diff_arrays("values", gv, wv)
            if e:
                errs.append((pattern, n, e))
    assert errs == [], errs[:3]


def test_radix_sort_orders_by_the_low_digits_only(gpu):
    """key_bits below the keys' width: the passes cover the 8-bit digits that hold bits [0, key_bits) — the low
    ceil(key_bits / 8) bytes — and the order by the bytes above stays as it was (the callers' keys have no bits there)."""
    keys = mu.sort_keys("random", 3 * TILE + 1, 32, seed=9)
    vals = mu.serial_origins(keys.shape[0])
    for bits in (0, 1, 8, 9, 17, 24):
        gk, gv = hip.test_radix_sort_pairs("u32_u64", keys, vals, bits, False)
        wk, wv = _sort_reference(keys, vals, (bits + 7) // 8 * 8) if bits else (keys, vals)
        assert mu.diff_arrays("keys", gk, wk) + mu.diff_arrays("values", gv, wv) == [], bits


def test_index_of_4097_tiles(engines):
    """4096 * 4096 + 1 pairs: 4097 tiles = 1 048 832 histogram entries, the second round of the scan of the tile sums
    (scan_block_sums_kernel) inside the sort — and of the heads scan behind it.  The largest input of this file."""
    n = TILE * TILE + 1
    values = mu.sort_keys("random", n, 30, seed=77)
    ref = _build_and_compare(engines(15), values, mu.serial_origins(n))
    assert ref.keys.shape[0] > (1 << 23)


def test_ragged_heads_beyond_one_scan_round(engines):
    """256 * 4096 + 4097 entries whose distinct-key flags are ragged: the heads scan (exclusive_scan_u8_u32) takes its
    second round on the product path; runs, distinct keys and member counts against the reference."""
    n = 256 * TILE + 4097
    rng = np.random.default_rng(5)
    steps = rng.integers(0, 3, n) * (rng.integers(0, 7, n) < 5)  # runs of ragged lengths, keys 1 or 2 apart
    values = np.cumsum(steps).astype(np.uint64)
    perm = rng.permutation(n)
    ref = _build_and_compare(engines(15), values[perm], mu.serial_origins(n))
    assert 300_000 < ref.keys.shape[0] < n and int(ref.members.max()) > 8


# ---- scan ------------------------------------------------------------------------------------------------------------

SCAN_SIZES = [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 256 * TILE - 1, 256 * TILE, 256 * TILE + 4097]


@pytest.mark.parametrize("out_off", [0, 1])
@pytest.mark.parametrize("in_off", [0, 1])
@pytest.mark.parametrize("variant", list(hip.SCAN_VARIANTS))
def test_exclusive_scan(gpu, variant, in_off, out_off):
    """Every size around a thread's 16 items, a tile and the 256 tile sums of one round of scan_block_sums_kernel; the
    offsets shift the device arrays by one element so that load16 / store16 take their element-wise path."""
    rng = np.random.default_rng(31)
    errs = []
    for n in SCAN_SIZES:
        inputs = {"ones": np.ones(n, np.uint64), "small": rng.integers(0, 256 if variant == "u8_u32" else 1000, n).astype(np.uint64)}
        if variant == "u32_u32" and n:  # large values whose total stays below 2^32 by construction
            inputs["large"] = rng.integers(0, ((1 << 32) - 1) // n + 1, n).astype(np.uint64)
        if variant == "u32_u64" and n:  # ... and a total far beyond 2^32 where the output has 64 bits
            inputs["full_range"] = rng.integers(0, 1 << 32, n).astype(np.uint64)
        for name, a in inputs.items():
            want = np.concatenate(([0], np.cumsum(a, dtype=np.uint64)))
            assert variant == "u32_u64" or int(want[-1]) < (1 << 32)
            e = mu.diff_arrays("scan", hip.test_exclusive_scan(variant, a, in_off, out_off), want)
            if e:
                errs.append((n, name, e))
    assert errs == [], errs[:3]


# ---- Filter and histogram --------------------------------------------------------------------------------------------

def _check_histogram(he, members):
    hist, over = he.shard_key_histogram()
    members = np.asarray(members)
    members = members[members > 0]  # a run without members is no key
    want = np.bincount(members[members < 65535], minlength=65536)
    big = np.sort(members[members >= 65535])
    want[65535] = big.shape[0]
    errs = mu.diff_arrays("key histogram", hist, want) + mu.diff_arrays("overflow list (sorted)", np.sort(over), big)
    assert errs == [], errs


@pytest.mark.parametrize("name", list(mu.FILTER_CASES))
def test_filter_quantile_at_the_bin_boundaries(engines, name):
    """Filter's count-of-counts histogram keeps counts below 256 in LDS, up to 65 534 in global bins and from 65 535 in an
    overflow list that index_filter resolves on the host: the quantile just below, on and just above both boundaries."""
    he = engines(15)
    counts, f_named, lands_on = mu.FILTER_CASES[name]
    values, origins, _, _ = mu.counts_stream(counts, 15, seed=5)
    ref = _build_and_compare(he, values, origins)
    assert sorted(ref.members.tolist()) == sorted(counts)
    for f in mu.FILTER_FREQUENCIES:
        he.filter(f)
        assert mu.diff_occurrence(he.occurrence, mu.occurrence(ref.members, f)) == [], f
    he.filter(f_named)
    assert he.occurrence == lands_on + 1
    _check_histogram(he, ref.members)


def test_histogram_counts_members_only(engines):
    """Streams with foreign entries: they are not counted, runs without members do not appear."""
    he = engines(15)
    counts, foreign = [1, 2, 255, 256, 257, 3, 65534, 65535], [0, 5, 1, 300, 0, 3, 2, 7]
    values, origins, _, _ = mu.counts_stream(counts, 15, foreign_counts=foreign, foreign_only=4, seed=6)
    ref = _build_and_compare(he, values, origins)
    assert ref.members.tolist() == counts + [0, 0, 0, 0]
    _check_histogram(he, ref.members)


def test_filter_of_an_empty_index(engines):
    he = engines(15)
    none = np.zeros(0, np.uint64)
    _build_and_compare(he, none, none)
    he.filter(0.5)
    assert he.occurrence == mu.NO_FILTER
    hist, over = he.shard_key_histogram()
    assert int(hist.sum()) == 0 and over.shape[0] == 0
    grp, pos, seg = he.shard_join(7)
    assert grp.shape[0] == 0 and seg.tolist() == [0] * 8


# ---- join ------------------------------------------------------------------------------------------------------------

def _join_and_compare(he, ref, n_reads_total, occ, all_query, flags, q_lo=0, q_hi=None):
    he.set_occurrence(occ)
    got = mu.Join(*he.shard_join(n_reads_total, flags[0], flags[1], q_lo, q_hi))
    want = mu.join_matches(ref, n_reads_total, occ, all_query, flags[0], flags[1], q_lo,
                           n_reads_total if q_hi is None else q_hi)
    errs = mu.diff_join(got, want)
    assert errs == [], (occ, all_query, flags, q_lo, q_hi, errs[:3])
    return want


@pytest.mark.parametrize("flags", FLAGS, ids=_fid)
@pytest.mark.parametrize("all_query", [False, True], ids=["flagged", "all_query"])
def test_join_edge_runs(engines, all_query, flags):
    """Foreign prefixes (the member count decides, not the run length), runs of only foreign entries, runs of one entry,
    one read twice in a run, a flagged and an unflagged entry of one read, both diagonal formulas at positions 0 and
    2^31 - 1, reads without matches between reads with matches (ids 3, 254 .. 258, 298, 299 of 300) — with occurrence
    below, at and above every member count present."""
    he = engines(15)
    R, named = mu.join_edge_runs()
    ref = _build_and_compare(he, *R.build(), all_query=all_query)
    total = 0
    for occ in (1, 2, 3, 4, 5, 6, 7, 8, 9, mu.NO_FILTER):
        total += _join_and_compare(he, ref, R.n_reads_total, occ, all_query, flags).grp.shape[0]
    assert total > 100
    for q_lo, q_hi in ((100, 100), (0, 150), (150, 300), (0, 300), (255, 257), (0, 3)):  # empty, halves, whole, foreign only
        _join_and_compare(he, ref, R.n_reads_total, 9, all_query, flags, q_lo, q_hi)


@pytest.mark.parametrize("all_query", [False, True], ids=["flagged", "all_query"])
@pytest.mark.parametrize("n_runs", [255, 256, 257])
def test_join_run_counts_around_a_block(engines, n_runs, all_query):
    he = engines(15)
    R = mu.join_many_runs(n_runs)
    ref = _build_and_compare(he, *R.build(), all_query=all_query)
    for flags in FLAGS:
        for occ in (1, 3, 4):
            _join_and_compare(he, ref, R.n_reads_total, occ, all_query, flags)
    _join_and_compare(he, ref, R.n_reads_total, 4, all_query, (False, False), 100, 200)


def test_join_one_run_of_1500(engines):
    """1500 all-query entries in one run: 2.25 M matches from one thread, 7500 per read.  The largest join of the file."""
    he = engines(15)
    R = mu.join_big_run()
    ref = _build_and_compare(he, *R.build(), all_query=True)
    want = _join_and_compare(he, ref, R.n_reads_total, 1500, True, (False, False))
    assert want.grp.shape[0] == 1500 * 1500
    assert _join_and_compare(he, ref, R.n_reads_total, 1499, True, (False, False)).grp.shape[0] == 0
    assert _join_and_compare(he, ref, R.n_reads_total, 1500, True, (True, True)).grp.shape[0] > 0


@pytest.mark.parametrize("k", [5, 17, 31])
def test_join_on_other_key_widths(engines, k):
    he = engines(k)
    R = mu.join_many_runs(257, k=k)
    ref = _build_and_compare(he, *R.build())
    for flags in FLAGS:
        _join_and_compare(he, ref, R.n_reads_total, 3, False, flags)


# ---- probe -----------------------------------------------------------------------------------------------------------

PROBE_CASES = [(15, "single_key"), (11, "gaps"), (15, "gaps"), (17, "gaps"), (31, "gaps"), (5, "dense"), (5, "ends"),
               (11, "ends"), (15, "ends"), (17, "ends"), (31, "ends")]


def _probe_case(k, case, direct=False):
    """All four flag combinations at two occurrences on one engine; returns the device outputs."""
    values, origins, _, keys, counts = mu.probe_index(k, case, seed=k)
    ref = mu.sort_index(values, origins)
    qv, qo, off = mu.probe_queries(keys, k, seed=k)
    e = hip.HookEngine(k, direct_index=direct)
    outs = []
    try:
        e.count_launches()
        e.index_build(values, origins)
        for occ in (3, mu.NO_FILTER):
            e.set_occurrence(occ)
            for flags in FLAGS:
                got = mu.Probe(*e.match_probe(qv, qo, off, *flags))
                want = mu.probe_matches(ref, qv, qo, off, occ, *flags)
                errs = mu.diff_probe(got, want)
                assert errs == [], (k, case, direct, occ, flags, errs[:3])
                outs.append(got)
            if occ == 3 and keys.shape[0] > 4:  # a count equal to occurrence is kept, occurrence + 1 is filtered
                hit = np.searchsorted(keys, qv[np.isin(qv, keys)])
                assert 3 in counts[hit] and 4 in counts[hit]
                assert want.filtered.sum() > 0 and want.grp.shape[0] > 0
        launches = e.launches()
    finally:
        e.close()
    # the bucket table is built once, lazily; with the option, the direct-address table beside it
    assert launches["table"] == (2 if direct else 1) and launches["match_count"] == 8
    return outs


@pytest.mark.parametrize("k,case", PROBE_CASES, ids=lambda x: str(x))
def test_probe(gpu, k, case):
    """rvn_test_match_probe == ram's Map up to the chain, in ram's order: keys present and absent, absent between two
    present neighbours in one bucket, below the smallest and above the largest key, 0 and 4^k - 1; bucket gaps of at most
    8 and of more; one key; one bucket per value (k = 5); 64-bit values (k = 17, 31); reads without minimizers."""
    _probe_case(k, case)


@pytest.mark.parametrize("case", ["gaps", "ends"])
def test_probe_direct_table_equals_bucket_table(gpu, case):
    """Every probe case of k = 11 again with index_direct_min_keys = 1 (a 32 MB table): the same bytes."""
    a, b = _probe_case(11, case), _probe_case(11, case, direct=True)
    for x, y in zip(a, b):
        assert mu.diff_probe(y, x) == []


def test_probe_degenerate(gpu):
    values, origins, _, keys, _ = mu.probe_index(15, "gaps")
    qv, qo, off = mu.probe_queries(keys, 15)
    none = np.zeros(0, np.uint64)
    e = hip.HookEngine(15)
    try:
        e.index_build(none, none)  # an empty index
        got = e.match_probe(qv, qo, off, False, False)
        assert got[0].shape[0] == 0 and not got[2].any() and not got[3].any()
        e.index_build(values, origins)  # no query minimizer at all
        got = e.match_probe(none, none, np.zeros(4, np.uint32), False, False)
        assert got[0].shape[0] == 0 and got[2].tolist() == [0, 0, 0, 0]
        absent = np.setdiff1d(qv, keys)  # no match at all
        got = mu.Probe(*e.match_probe(absent, qo[:absent.shape[0]], np.array([0, absent.shape[0]], np.uint32), False, False))
        assert got.grp.shape[0] == 0 and got.seg.tolist() == [0, 0] and not got.filtered.any()
        with pytest.raises(ValueError):  # a value of more than 2k bits would index beyond the table
            e.match_probe(np.array([1 << 30], np.uint64), qo[:1], np.array([0, 1], np.uint32), False, False)
        bad = off.copy()
        bad[-1] += 1  # offsets that do not end at the number of query minimizers
        with pytest.raises(ValueError):
            e.match_probe(qv, qo, bad, False, False)
    finally:
        e.close()
