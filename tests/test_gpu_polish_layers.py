"""The window-layer stage of a polishing round on the device (raven_amd/csrc/polish.hip: layer_count_kernel,
layer_fill_kernel, window_finish_kernel, layer_quality_kernel, count_flags_kernel, stitch_kernel, the host planning of
jobs / WinMeta / [W0, W1) / ratio, and best_overlap_kernel through its hook) on the crafted rounds of tests/layer_cases.py.

Engine.polish_set_best dictates every read's overlap, so the alignment span, the breakpoints and the layers are the
test's: the layer table must equal layer_cases.layers_from_best row for row (tests/test_layer_cases.py holds that
reference to oracle.polish_layers on the CPU), the statistics must be the reference's counts, and the consensus is held
to oracle.poa_window over the reference's windows under the tolerance tests/test_gpu_polish.py states (TOL_CPU).

rvn_polish_fetch_layers reports GLOBAL window numbers (first window of the range + index), also for a round over a
range: the rows of a range are compared with the full table's rows of those windows as they are."""
import functools
import math

import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip
from tests import layer_cases as lc
from tests import polish_util as pu2
from tests.test_gpu_polish import TOL_CPU, _ed

pytestmark = pytest.mark.gpu

ALL = 1 << 62


@pytest.fixture(scope="module")
def eng():
    return hip.Engine(15, 5)


@functools.lru_cache(maxsize=None)
def _cases():
    return {c["name"]: c for c in lc.cases()}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(layer table, counts, consensus per target) of a case, computed once and never written to."""
    c = _cases()[name]
    table = lc.layers_from_best(c["targets"], c["reads"], c["best"], c["best_t"], c["quals"], c["q"], c["w"])
    table.setflags(write=False)
    cons, polished = lc.reference_consensus(c, table)
    k = lc.counts(c, table)
    assert polished == k["polished"]
    return table, k, cons


def _words(best):
    return np.ascontiguousarray(best).view(np.uint32).reshape(-1, 8)


def _upload(eng, c):
    td, rd = eng.upload(c["targets"]), eng.upload(c["reads"])
    quals = c["quals"]
    if c["blocks"] is not None:  # the qualities live with the read set, one byte per 64 bases
        rd.attach_quality(c["blocks"], block_shift=6)
        quals = None
    return td, rd, quals


# the rounds at racon's w = 500 first, the w = 50 rounds last
CASE_ORDER = sorted(_cases(), key=lambda n: (_cases()[n]["w"] != 500, n))


@pytest.mark.parametrize("name", CASE_ORDER)
def test_layer_table_counts_and_consensus_of_a_crafted_round(eng, name):
    c = _cases()[name]
    want, k, ref_cons = _reference(name)
    td, rd, quals = _upload(eng, c)
    eng.polish_set_best(_words(c["best"]), c["best_t"])
    cons, ratio, st = eng.polish_round(td, rd, quals=quals, q=c["q"], w=c["w"])
    got = eng.polish_layers()
    print(name, "layers", got.shape[0], "of", want.shape[0], {x: st[x] for x in ("n_layers", "n_reads_used", "n_windows",
          "n_polished_windows", "n_failed_windows", "n_dropped_layers", "n_aligned")}, "ratio", list(ratio))
    assert got.shape == want.shape and np.array_equal(got, want)
    assert st["n_layers"] == k["n_layers"] and st["n_reads_used"] == k["n_reads_used"]
    assert st["n_windows"] == k["n_windows"] and st["n_dropped_layers"] == 0 and st["n_failed_windows"] == 0
    assert st["n_polished_windows"] == sum(k["polished"])
    for t in range(c["targets"].n):
        assert ratio[t] == k["polished"][t] / k["windows"][t]
        d = _ed(cons[t], ref_cons[t])
        print(name, "target", t, "ED(gpu, reference)", d, "of", len(ref_cons[t]))
        assert d <= math.ceil(TOL_CPU * len(ref_cons[t])), (d, len(ref_cons[t]))


def _cuts(name):
    """(lo, hi) window ranges of a case: a cut inside a target, at a target boundary, inside the span of one read's
    overlap, and an empty range."""
    c = _cases()[name]
    w = c["w"]
    fw = [int(x) for x in lc.first_windows(c["targets"], w)]
    n = fw[-1]
    inside_target = next(k for k in range(1, n) if k not in fw)
    boundary = fw[1] if len(fw) > 2 else n  # (one target: the only boundaries are the ends)
    spanned = None
    for o, bt in zip(c["best"], c["best_t"]):
        a, b = int(o["rhs_begin"]) // w, (int(o["rhs_end"]) - 1) // w
        if b > a:
            spanned = fw[int(bt)] + a + 1
            break
    assert spanned is not None
    return n, sorted({inside_target, boundary, spanned}), inside_target


@pytest.mark.parametrize("name", ["multi_target", "ties_130"])
def test_window_ranges_give_exactly_their_rows_and_add_up(eng, name):
    c = _cases()[name]
    want, k, _ = _reference(name)
    td, rd, quals = _upload(eng, c)
    n, cuts, inside = _cuts(name)

    def run(lo, hi):
        eng.polish_set_best(_words(c["best"]), c["best_t"])
        cons, nw, npol, st = eng.polish_round_range(td, rd, lo, hi, quals=quals, q=c["q"], w=c["w"])
        return cons, [int(x) for x in nw], [int(x) for x in npol], st, eng.polish_layers()

    cons_f, nw_f, npol_f, st_f, lay_f = run(0, ALL)
    assert np.array_equal(lay_f, want) and nw_f == k["windows"] and npol_f == k["polished"]
    for cut in cuts:
        parts = [run(0, cut), run(cut, n)]
        for (lo, hi), (cons, nw, npol, st, lay) in zip(((0, cut), (cut, n)), parts):
            rows = want[(want[:, 0] >= lo) & (want[:, 0] < hi)]
            assert lay.shape == rows.shape and np.array_equal(lay, rows), (cut, lo, hi)
            assert st["n_windows"] == hi - lo and st["n_layers"] == rows.shape[0] and sum(nw) == hi - lo
        for t in range(c["targets"].n):
            assert parts[0][1][t] + parts[1][1][t] == nw_f[t] and parts[0][2][t] + parts[1][2][t] == npol_f[t]
            # windows are stitched in order: the two halves of a target are the target's consensus
            assert np.array_equal(np.concatenate([parts[0][0][t], parts[1][0][t]]), cons_f[t])
    cons, nw, npol, st, lay = run(inside, inside)  # lo == hi: no window, no layer, nothing written
    assert lay.shape[0] == 0 and st["n_windows"] == 0 and sum(nw) == 0 and sum(npol) == 0 and all(len(x) == 0 for x in cons)
    cons, nw, npol, st, lay = run(n, ALL)          # a range behind the last window
    assert lay.shape[0] == 0 and st["n_windows"] == 0 and all(len(x) == 0 for x in cons)


@functools.lru_cache(maxsize=None)
def _synthetic():
    _, _, targets, reads, _ = pu2.make_case(genome_len=12_000, coverage=12, read_len=2000, seed=7)
    want = oracle.polish_layers(targets, reads)
    want.setflags(write=False)
    return targets, reads, want


def test_supplied_table_is_validated_and_consumed_by_one_round(eng):
    targets, reads, want = _synthetic()
    td, rd = eng.upload(targets), eng.upload(reads)
    best, best_t = lc.best_from_oracle(targets, reads)
    # a table of another length than the read set
    eng.polish_set_best(_words(best[:-1]), best_t[:-1])
    with pytest.raises(ValueError, match="does not match the read set"):
        eng.polish_round(td, rd)
    eng.polish_round(td, rd)  # the refused table is gone with the round that refused it: this one maps by itself
    assert np.array_equal(eng.polish_layers(), want)
    # a target index of at least the number of targets
    bad = best_t.copy()
    bad[int(np.flatnonzero(best_t != lc.UNUSED)[3])] = targets.n
    eng.polish_set_best(_words(best), bad)
    with pytest.raises(ValueError, match="names a target that does not exist"):
        eng.polish_round(td, rd)
    eng.polish_round(td, rd)
    assert np.array_equal(eng.polish_layers(), want)
    # a table that leaves out every second read is used by ONE round
    half = best_t.copy()
    half[1::2] = lc.UNUSED
    ref_half = lc.layers_from_best(targets, reads, best, half)
    assert 0 < ref_half.shape[0] < want.shape[0]
    eng.polish_set_best(_words(best), half)
    _, _, st = eng.polish_round(td, rd)
    assert np.array_equal(eng.polish_layers(), ref_half) and st["n_reads_used"] == int((half != lc.UNUSED).sum())
    _, _, st = eng.polish_round(td, rd)
    assert np.array_equal(eng.polish_layers(), want) and st["n_reads_used"] == int((best_t != lc.UNUSED).sum())


def test_map_path_and_supplied_path_agree(eng):
    targets, reads, want = _synthetic()
    td, rd = eng.upload(targets), eng.upload(reads)
    cons_a, ratio_a, st_a = eng.polish_round(td, rd)
    lay_a = eng.polish_layers()
    assert np.array_equal(lay_a, want)
    best, best_t, n_ovl = eng.polish_map_best(td, rd)
    assert n_ovl == st_a["n_overlaps"]
    ref_best, ref_best_t = lc.best_from_oracle(targets, reads)
    assert np.array_equal(best_t, ref_best_t) and np.array_equal(best, _words(ref_best))
    eng.polish_set_best(best, best_t)
    cons_b, ratio_b, st_b = eng.polish_round(td, rd)
    assert np.array_equal(eng.polish_layers(), lay_a) and st_b["n_overlaps"] == 0  # (no mapping in that round)
    assert len(cons_a) == len(cons_b) and all(np.array_equal(x, y) for x, y in zip(cons_a, cons_b))
    assert list(ratio_a) == list(ratio_b) and st_a["n_layers"] == st_b["n_layers"]
    assert st_a["n_reads_used"] == st_b["n_reads_used"]


# ---- best_overlap_kernel on crafted lists (rvn_test_best_overlap) ----------------------------------------------------

def _ovl(lhs_begin, lhs_end, rhs_id, rhs_begin, rhs_end, strand=1, score=0, lhs_id=0):
    o = np.zeros(1, dtype=hip.OVERLAP_DTYPE)[0]
    for f, v in (("lhs_id", lhs_id), ("lhs_begin", lhs_begin), ("lhs_end", lhs_end), ("rhs_id", rhs_id),
                 ("rhs_begin", rhs_begin), ("rhs_end", rhs_end), ("score", score), ("strand", strand)):
        o[f] = v
    return o


def _best_reference(lists, first, err_thr, id_to_t, best, best_t):
    """racon's choice in numpy, doubles for the error ratio: the first of the longest overlaps; unused when
    1 - min(span) / max(span) > err_thr or the target id has no index."""
    best, best_t = best.copy(), best_t.copy()
    for r, lst in enumerate(lists):
        b, t = np.zeros(1, dtype=hip.OVERLAP_DTYPE)[0], lc.UNUSED
        if len(lst):
            a = lst["lhs_end"].astype(np.int64) - lst["lhs_begin"]
            c = lst["rhs_end"].astype(np.int64) - lst["rhs_begin"]
            b = lst[int(np.argmax(np.maximum(a, c)))]  # argmax: the first of the maxima
            x, y = np.float64(int(b["lhs_end"]) - int(b["lhs_begin"])), np.float64(int(b["rhs_end"]) - int(b["rhs_begin"]))
            with np.errstate(invalid="ignore", divide="ignore"):
                err = np.float64(1.0) - np.minimum(x, y) / np.maximum(x, y)
            if not (err > err_thr) and int(b["rhs_id"]) < len(id_to_t):
                t = int(id_to_t[int(b["rhs_id"])])
        best[first + r], best_t[first + r] = b, t
    return best, best_t


def _run_best(lists, first, err_thr, id_to_t, extra_rows=3):
    lists = [np.asarray(x, dtype=hip.OVERLAP_DTYPE).reshape(-1) for x in lists]
    off = np.zeros(len(lists) + 1, dtype=np.uint32)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate(lists) if lists else np.zeros(0, dtype=hip.OVERLAP_DTYPE)
    rows = first + len(lists) + extra_rows
    best0 = np.zeros(rows, dtype=hip.OVERLAP_DTYPE)
    best0.view(np.uint32)[:] = 0xABABABAB  # the caller's sentinel
    bt0 = np.full(rows, 0x12345678, dtype=np.uint32)
    id_to_t = np.asarray(id_to_t, dtype=np.uint32)
    got = hip.test_best_overlap(flat, off, first, err_thr, id_to_t, best0, bt0)
    want = _best_reference(lists, first, err_thr, id_to_t, best0, bt0)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    outside = np.ones(rows, dtype=bool)
    outside[first:first + len(lists)] = False
    assert (got[1][outside] == 0x12345678).all() and (got[0].view(np.uint32).reshape(-1, 8)[outside] == 0xABABABAB).all()
    return got


def _stack(*ovls):
    out = np.zeros(len(ovls), dtype=hip.OVERLAP_DTYPE)
    for i, o in enumerate(ovls):
        out[i] = o
    return out


def test_best_overlap_kernel_on_crafted_lists():
    idmap = [2, lc.UNUSED, 0, 1, 3]  # not the identity; id 1 is no target
    rng = np.random.default_rng(3)
    many = np.zeros(1000, dtype=hip.OVERLAP_DTYPE)
    many["lhs_begin"] = rng.integers(0, 100, size=1000)
    many["lhs_end"] = many["lhs_begin"] + rng.integers(1000, 5000, size=1000)
    many["rhs_begin"] = rng.integers(0, 100, size=1000)
    many["rhs_end"] = many["rhs_begin"] + (many["lhs_end"] - many["lhs_begin"]) - rng.integers(0, 50, size=1000).astype(np.uint32)
    many["rhs_id"] = rng.integers(2, 5, size=1000)
    many["score"] = np.arange(1000)
    top = int((many["lhs_end"] - many["lhs_begin"]).max()) + 1
    for i in (411, 412, 977):  # the longest span three times: the first of them wins
        many["lhs_end"][i] = many["lhs_begin"][i] + top
    lists = [
        _stack(),                                                                          # no overlap
        _stack(_ovl(0, 900, 0, 100, 1000, score=1), _ovl(5, 905, 2, 0, 900, score=2), _ovl(9, 909, 3, 7, 907, score=3)),  # ties
        _stack(_ovl(0, 900, 0, 0, 900, score=1), _ovl(0, 901, 2, 0, 900, score=2)),         # a later, strictly longer one
        _stack(_ovl(0, 900, 0, 0, 800, score=1), _ovl(0, 700, 2, 0, 850, score=2)),         # decided by an lhs span
        _stack(_ovl(0, 800, 0, 0, 950, score=1), _ovl(0, 900, 2, 0, 900, score=2)),         # decided by an rhs span
        _stack(_ovl(0, 7001, 0, 0, 10000)), _stack(_ovl(0, 7000, 0, 0, 10000)), _stack(_ovl(0, 6999, 0, 0, 10000)),
        _stack(_ovl(0, 10000, 0, 0, 7001)), _stack(_ovl(0, 10000, 0, 0, 7000)), _stack(_ovl(0, 10000, 0, 0, 6999)),
        _stack(_ovl(50, 50, 3, 70, 70)),                                                   # zero length: NaN ratio, kept
        _stack(_ovl(0, 500, 5, 0, 500)), _stack(_ovl(0, 500, 0xFFFFFFFF, 0, 500)),          # rhs_id beyond the map
        _stack(_ovl(0, 500, 1, 0, 500)),                                                   # mapped to no target
        _stack(_ovl(0, 500, 4, 0, 500, strand=0)),
        many,
        _stack(),
    ]
    best, bt = _run_best(lists, 7, 0.3, idmap)
    kept = [int(x) != lc.UNUSED for x in bt[7:7 + len(lists)]]
    assert kept[1] and kept[2] and kept[11] and not kept[0] and not kept[12] and not kept[13] and not kept[14]
    assert [int(best[7 + i]["score"]) for i in (1, 2, 3, 4)] == [1, 2, 1, 1] and int(best[7 + 16]["score"]) == 411
    assert len(set(kept[5:8])) == 2 and kept[5:8] == kept[8:11]  # the threshold falls between the three ratios
    # err_thr = 0: only equal spans are kept (and the NaN of a zero-length overlap)
    _, bt0 = _run_best(lists, 0, 0.0, idmap, extra_rows=1)
    assert [int(x) != lc.UNUSED for x in bt0[:len(lists)]][1:5] == [True, False, False, False]
    assert int(bt0[11]) == 1 and int(bt0[15]) == 3
    _run_best([], 4, 0.3, idmap)  # no read at all: nothing is launched, nothing is written


@pytest.mark.parametrize("n", [1, 256, 257])
def test_best_overlap_kernel_writes_rows_first_to_first_plus_n(n):
    rng = np.random.default_rng(n)
    lists = []
    for _ in range(n):
        m = int(rng.integers(0, 5))
        o = np.zeros(m, dtype=hip.OVERLAP_DTYPE)
        o["lhs_end"] = rng.integers(1, 4, size=m) * 1000
        o["rhs_end"] = rng.integers(1, 4, size=m) * 1000 + rng.integers(0, 2, size=m) * 600
        o["rhs_id"] = rng.integers(0, 6, size=m)
        o["score"] = rng.integers(0, 1 << 20, size=m)
        lists.append(o)
    _, bt = _run_best(lists, 5, 0.3, [1, 0, lc.UNUSED, 2])
    used = bt[5:5 + n] != lc.UNUSED
    assert n == 1 or (used.any() and not used.all())
