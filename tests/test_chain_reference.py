"""CPU: the yardstick of tests/test_gpu_chain.py and the claims of its generators.

1. py_chain (tests/chain_util.py: ram's Chain line by line in plain Python) equals oracle.Engine.chain field for field on
   every crafted family — inputs the oracle was never run on before (ties, chain < 4, bandwidth 0).
2. The generators produce what the GPU tests say they feed the device.  These are conditions on the INPUT, evaluated with
   py_chain and its by-products, never with the device.
"""
import numpy as np
import pytest

from oracle import oracle
from tests import chain_util as cu


def _same(oe, lhs_id, g, p, k, params, info=None):
    want = cu.overlaps_as_tuples(oe.chain(lhs_id, g, p))
    got = cu.py_chain(lhs_id, g, p, k, *params, info=info)
    assert got == want, (k, params, len(got), len(want), [x for x in zip(got, want) if x[0] != x[1]][:2])
    return got


@pytest.mark.parametrize("params", cu.PARAM_SETS, ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("k", [5, 15, 31])
def test_py_chain_equals_oracle_on_every_family(k, params):
    oe = oracle.Engine(k, 5, *params)
    for name in cu.FAMILIES:
        for strand in (1, 0):
            for n in (4, 8, 31, 33, 64, 65, 257, 1100):
                if name == "ties" and n < 8:
                    continue
                b = cu.Batch(n * 7 + k + strand)
                g, p = b.interval(name, n, strand, k, params)
                perm = b.rng.permutation(n)
                info = {}
                _same(oe, 77, g[perm], p[perm], k, params, info)
                assert info["intervals"] == [(0, n)], (name, n)  # place(): one band whatever the bandwidth


@pytest.mark.parametrize("params", cu.PARAM_SETS, ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("k", [5, 15, 31])
def test_py_chain_equals_oracle_on_assembled_reads(k, params):
    """Whole reads (several intervals, rhs ids, both strands, the band scenarios), read by read."""
    oe = oracle.Engine(k, 5, *params)
    ids, grp, pos, seg = cu.mixed_batch(100 + k, k, params).build()
    n_ovl = 0
    for i in range(ids.shape[0]):
        s, e = int(seg[i]), int(seg[i + 1])
        n_ovl += len(_same(oe, int(ids[i]), grp[s:e], pos[s:e], k, params))
    assert n_ovl > 0


@pytest.mark.parametrize("strand", [1, 0])
def test_band_scenarios_cut_the_intervals_they_claim(strand):
    bandwidth, chain, matches, gap = params = cu.DEFAULT_PARAMS
    g, p, used = cu.band(np.random.default_rng(1), strand, 50, 15, params)
    m = max(chain, -(-matches // 15), 4) + 2
    by_rhs = {}
    info = {}
    ovl = cu.py_chain(1, g, p, 15, *params, info=info)
    gs = np.sort(g)
    for a, b in info["intervals"]:
        assert int(gs[a]) >> 33 == int(gs[b - 1]) >> 33
        by_rhs.setdefault((int(gs[a]) >> 33) - 50, []).append(b - a)
    assert by_rhs == {0: [2 * m], 1: [m, m], 2: [4 + m, m], 4: [4], 5: [400]}  # (3: windows of 3, no interval)
    # the drift scenario: 400 matches whose diagonals span 9900 come out as ONE overlap
    drift = gs[(gs >> np.uint64(33)) == np.uint64(55)]
    assert int(drift.max() - drift.min()) == 9900
    assert sum(1 for o in ovl if o[3] == 55) == 1
    # bandwidth 0: every four matches of the drift are their own interval
    info = {}
    g0, p0, _ = cu.band(np.random.default_rng(1), strand, 50, 15, cu.PARAM_SETS[1])
    cu.py_chain(1, g0, p0, 15, *cu.PARAM_SETS[1], info=info)
    g0s = np.sort(g0)
    assert [b - a for a, b in info["intervals"] if int(g0s[a]) >> 33 == 55] == [4] * 100


def test_class_batch_has_every_boundary_size():
    b, want = cu.class_batch()
    ids, grp, pos, seg = b.build()
    totals = np.diff(seg.astype(np.int64)).tolist()
    sizes = []
    for i in range(ids.shape[0]):
        gi = np.sort(grp[int(seg[i]):int(seg[i + 1])]).tolist()
        sizes += [e - s for s, e in cu.py_intervals(gi, cu.DEFAULT_PARAMS[0])]
    for cap in (cu.CHAIN_SMALL_CAP,) + cu.CHAIN_CLASS_CAPS:
        for n in (cap - 1, cap, cap + 1):
            assert n in sizes, n
    assert 20000 in sizes and max(sizes) > 65536
    for n in want["intervals"]:
        assert n in sizes, n
    for cap in cu.SEG_CLASS_CAPS:
        for t in (cap - 1, cap, cap + 1):
            assert t in totals, t
    assert max(totals) > 65536 and totals[0] == 0 and totals[-1] == 0 and 1 in totals and 3 in totals
    # every class of the two tables is met (what the launch counts of the GPU test then show the device to have run)
    cls = lambda n, caps: next((c for c, cap in enumerate(caps) if n <= cap), len(caps))
    assert {cls(t, cu.SEG_CLASS_CAPS) for t in totals if t >= 2} == set(range(len(cu.SEG_CLASS_CAPS) + 1))
    assert {cls(n, cu.CHAIN_CLASS_CAPS) for n in sizes if n > cu.CHAIN_SMALL_CAP} == set(range(len(cu.CHAIN_CLASS_CAPS) + 1))
    assert any(4 <= n <= cu.CHAIN_SMALL_CAP for n in sizes)
    # a read above the largest group-sort class made of small intervals only
    assert want["totals"][-1] > 4096 and want["totals"][-1] in totals
    # read ids are not indices, rhs ids reach 2^31 - 1, both strands occur, positions are distinct per (rhs id, strand)
    assert int(ids[-1]) == (1 << 30) - 1 and int((grp >> np.uint64(33)).max()) == (1 << 31) - 1
    assert set(((grp >> np.uint64(32)) & np.uint64(1)).tolist()) == {0, 1}
    for i in range(ids.shape[0]):
        s, e = int(seg[i]), int(seg[i + 1])
        key = np.stack([grp[s:e] >> np.uint64(32), pos[s:e]], axis=1)
        assert np.unique(key, axis=0).shape[0] == e - s, i


@pytest.mark.parametrize("flip", [0, 1])
def test_regime_batch_places_the_chain_lengths(flip):
    b, exact = cu.regime_batch(flip=flip)
    seen = set()
    for read, L, tail, n in exact:
        g, p = [blk for blk in b.reads[read] if blk[0].shape[0] == n][0]
        info = {}
        cu.py_chain(1, g, p, 15, *cu.DEFAULT_PARAMS, info=info)
        assert info["intervals"] == [(0, n)] and info["longest"] == [L], (L, n, info["longest"])
        seen.add((L, n > cu.CHAIN_CLASS_CAPS[-1]))
    for L in cu.REGIME_LENGTHS:
        assert (L, False) in seen
    assert {L for L, glob in seen if glob} >= {64, 513, 5000}  # the global path in each of the three regimes
    assert {blk[0].shape[0] % 64 for r in b.reads for blk in r if blk[0].shape[0] > 64} >= {0, 1, 63}


def test_ties_defeat_a_longest_chain_search():
    """On strand 1 ram sorts equal lhs by ascending rhs, so a later match of the same lhs replaces a tail it does not
    precede: the patience search's chain is SHORTER than the longest chain.  (On strand 0 the same sort order is the
    descending one a patience search wants, and the two agree.)  A device search that finds 'a longest chain' instead of
    ram's fails on these intervals."""
    rng = np.random.default_rng(5)
    shorter = 0
    for _ in range(60):
        lhs, r = cu.ties(rng, 60, 15)
        g, p = cu.place(rng, lhs, r, 1, 9, 500)
        ps = sorted(int(x) for x in p)
        a, c = len(cu.py_longest_subsequence(ps, 1)), cu.longest_chain_n2(ps, 1)
        assert a <= c
        shorter += a < c
    assert shorter >= 30, shorter


@pytest.mark.parametrize("chain,want4096", [(1, 4096), (2, 2048), (3, 1365), (4, 1024), (7, 585)])
def test_slots_fill_the_slot_region(chain, want4096):
    b, listed = cu.slots_batch(3, chain)
    params = (100, chain, 0, 50)
    done_4096 = False
    for read, n in listed:
        if n > 600 and (n != 4096 or done_4096):
            continue
        done_4096 |= n == 4096
        g, p = [blk for blk in b.reads[read] if blk[0].shape[0] == n][0]
        assert len(cu.py_chain(1, g, p, 15, *params)) == n // chain, (n, chain)
    assert done_4096 and 4096 // chain == want4096
    # neighbours: the intervals of a read share rhs id and strand and are cut apart by their diagonals alone
    ids, grp, pos, seg = b.build()
    info = {}
    cu.py_chain(1, grp[:int(seg[1])], pos[:int(seg[1])], 15, *params, info=info)
    assert sorted(e - s for s, e in info["intervals"]) == sorted(n for r, n in listed if r == 0)
