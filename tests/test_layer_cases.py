"""tests/layer_cases.py held to the oracle on the CPU: its reference restates oracle.polish_layers on whole synthetic
rounds, and every crafted case is what its tags say it is — by the reference's own output, never by what the device
returns (tests/test_gpu_polish_layers.py runs the rounds on the device)."""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import layer_cases as lc
from tests import polish_util as pu2


@functools.lru_cache(maxsize=None)
def _cases():
    return {c["name"]: c for c in lc.cases()}


@functools.lru_cache(maxsize=None)
def _table(name):
    c = _cases()[name]
    t = lc.layers_from_best(c["targets"], c["reads"], c["best"], c["best_t"], c["quals"], c["q"], c["w"])
    t.setflags(write=False)
    return t


def _rows(table):
    return {tuple(int(x) for x in r) for r in table}


def _pieces(table):
    return {(int(r[0]), int(r[1])) for r in table}


# ---- the reference against oracle.polish_layers ----------------------------------------------------------------------

@pytest.mark.parametrize("n_targets,with_qual,w", [(1, False, 500), (2, True, 500), (1, False, 200)])
def test_reference_reproduces_the_oracles_layer_table(n_targets, with_qual, w):
    _, _, targets, reads, _ = pu2.make_case(genome_len=12_000, coverage=12, read_len=2000, seed=7, n_targets=n_targets)
    quals, q = None, 0.0
    if with_qual:  # per-base qualities 3 .. 19: q = 11 drops some layers and keeps others
        rng = np.random.default_rng(5)
        quals = [(rng.integers(3, 20, size=int(n)) + 33).astype(np.uint8) for n in reads.lengths]
        q = 11.0
    want = oracle.polish_layers(targets, reads, quals=quals, q=q, w=w)
    best, best_t = lc.best_from_oracle(targets, reads, 0.3)
    got = lc.layers_from_best(targets, reads, best, best_t, quals, q, w)
    assert want.shape[0] > 100 and got.shape == want.shape and np.array_equal(got, want)
    assert (got[:, 6] == 0).any() and (got[:, 6] == 1).any()
    if with_qual:
        assert got.shape[0] < lc.layers_from_best(targets, reads, best, best_t, None, 0.0, w).shape[0]


# ---- the cases are what they are named after -------------------------------------------------------------------------

def _wrong_quals(c, how):
    """The table the reference gives when the qualities are read the wrong way round."""
    quals = [np.asarray(x)[::-1] for x in c["quals"]] if how == "reversed" else None
    if how == "blocks_reversed":
        quals = [np.repeat(b[::-1], 64)[:len(x)] for b, x in zip(c["blocks"], c["quals"])]
    return lc.layers_from_best(c["targets"], c["reads"], c["best"], c["best_t"], quals, c["q"], c["w"])


def _check_len_9(c, t):
    assert c["w"] == 500 and t.shape[0] == c["reads"].n and set(t[:, 0]) == {1}
    for o in c["best"]:  # 9 bases in the first and in the last window
        assert 500 - int(o["rhs_begin"]) == 9 and int(o["rhs_end"]) - 1000 == 9


def _check_len_10(c, t):
    assert c["w"] == 500 and t.shape[0] == 3 * c["reads"].n
    assert sorted(int(x) for x in t[t[:, 0] != 1][:, 3]) == [10] * (2 * c["reads"].n)


def _check_empty_window(c, t):
    w = c["w"]
    for r in range(c["reads"].n):  # windows 1 and 2 lie inside the overlap's span and have no row
        assert int(c["best"][r]["rhs_begin"]) < w and int(c["best"][r]["rhs_end"]) > 3 * w
        assert {int(x) for x in t[t[:, 1] == r][:, 0]} == {0, 3}


def _check_one_pair(c, t):
    assert c["w"] == 50 and 1 >= 0.02 * c["w"]  # the length rule lets one base through: begin < end decides
    ends = sorted(int(o["rhs_end"]) for o in c["best"])
    assert ends == [101, 101, 102, 102]
    last = t[t[:, 0] == 2]
    assert last.shape[0] == 2 and (last[:, 3] == 2).all() and (last[:, 4] == 0).all() and (last[:, 5] == 1).all()


def _check_short_tail(c, t):
    lens = [int(x) for x in c["targets"].lengths]
    w = c["w"]
    assert 2003 in lens and any(n % w == 0 for n in lens) and any(n % w == 1 for n in lens)
    fw = lc.first_windows(c["targets"], w)
    for ti, n in enumerate(lens):  # a read reaches the last base of every target
        assert any(int(bt) == ti and int(o["rhs_end"]) == n for o, bt in zip(c["best"], c["best_t"]))
        tail = n - (n - 1) // w * w
        rows = t[t[:, 0] == fw[ti + 1] - 1]
        assert (rows[:, 5] <= tail - 1).all()
        if tail == 1 or tail < 0.02 * w:
            assert rows.shape[0] == 0
        else:
            assert rows.shape[0] > 0
            if tail < w:
                assert (rows[:, 5] == tail - 1).any()


def _check_q_exact(c, t):
    assert c["q"] == 10.0 and all((np.asarray(x) >= 42).all() for x in c["quals"])
    lowered = [r for r, x in enumerate(c["quals"]) if (np.asarray(x) == 42).sum() == 1]
    pristine = [r for r, x in enumerate(c["quals"]) if (np.asarray(x) == 43).all()]
    assert len(lowered) == 2 and len(pristine) == 2
    for r in pristine:
        assert (t[:, 1] == r).sum() == 3
    for r in lowered:
        assert [int(x) for x in t[t[:, 1] == r][:, 0]] == [1, 2]
    # without the filter all twelve pieces are layers
    assert lc.layers_from_best(c["targets"], c["reads"], c["best"], c["best_t"], None, 0.0, c["w"]).shape[0] == 12


def _check_q_oriented(c, t):
    assert (c["best"]["strand"] == 0).any()
    wrong = _wrong_quals(c, "reversed")
    assert not np.array_equal(wrong, t)
    rc_read = int(np.flatnonzero(c["best"]["strand"] == 0)[0])
    assert [int(x) for x in t[t[:, 1] == rc_read][:, 0]] == [0]
    assert [int(x) for x in wrong[wrong[:, 1] == rc_read][:, 0]] == [2]


def _check_q_blocks(c, t):
    assert c["blocks"] is not None and (c["best"]["strand"] == 0).any() and (c["best"]["strand"] == 1).any()
    for b, x, n in zip(c["blocks"], c["quals"], c["reads"].lengths):
        assert len(b) == (int(n) + 63) // 64 and int(n) % 64 != 0 and np.array_equal(np.repeat(b, 64)[:int(n)], x)
    unfiltered = lc.layers_from_best(c["targets"], c["reads"], c["best"], c["best_t"], None, 0.0, c["w"])
    assert 0 < t.shape[0] < unfiltered.shape[0]
    assert (unfiltered[:, 2] % 64 != 0).any() and ((unfiltered[:, 2] + unfiltered[:, 3]) % 64 != 0).any()
    for strand in (0, 1):  # the filter decides on both strands, both ways
        reads = set(np.flatnonzero(c["best"]["strand"] == strand))
        kept = sum(int(r[1]) in reads for r in t)
        assert 0 < kept < sum(int(r[1]) in reads for r in unfiltered)
    assert not np.array_equal(_wrong_quals(c, "blocks_reversed"), t)


def _check_ties_130(c, t):
    assert c["reads"].n == 130 > 2 * 64
    for wdw in (0, 1):
        rows = t[t[:, 0] == wdw]
        assert rows.shape[0] == 130 and len(set(rows[:, 4])) == 1 and [int(x) for x in rows[:, 1]] == list(range(130))


def _check_ties_interleaved(c, t):
    rows = t[t[:, 0] == 0]
    assert rows.shape[0] == 130 and len(set(rows[:, 4])) == 5
    order = [int(x) for x in rows[:, 1]]
    assert order != sorted(order)                                        # not by job alone
    assert (np.diff(rows[:, 4].astype(np.int64)) >= 0).all()             # by begin ...
    same = np.diff(rows[:, 4].astype(np.int64)) == 0
    assert same.sum() > 100 and (np.diff(rows[:, 1].astype(np.int64))[same] > 0).all()  # ... then by read
    assert (rows[:, 6] == 0).any() and (rows[:, 6] == 1).any()


def _check_unused_and_degenerate(c, t):
    bt, b = c["best_t"], c["best"]
    unused = np.flatnonzero(bt == lc.UNUSED)
    assert len(unused) >= 2 and 0 < unused.min() and unused.max() < len(bt) - 1
    assert any(int(o["rhs_end"]) == int(o["rhs_begin"]) and int(x) != lc.UNUSED for o, x in zip(b, bt))
    assert any(int(o["lhs_end"]) == int(o["lhs_begin"]) and int(x) != lc.UNUSED for o, x in zip(b, bt))
    assert lc.counts(c, t)["n_reads_used"] > len(set(t[:, 1]))  # used reads without a layer
    assert sorted(set(int(x) for x in t[:, 0])) == [0, 2, 4] and lc.counts(c, t)["n_windows"] == 5


def _check_multi_target(c, t):
    ids = [int(x) for x in c["targets"].ids]
    assert c["targets"].n == 3 and sorted(ids) != list(range(3)) and len(set(int(x) for x in c["targets"].lengths)) == 3
    fw = lc.first_windows(c["targets"], c["w"])
    for ti in range(3):
        assert (c["best_t"] == ti).sum() >= 5
        rows = t[(t[:, 0] >= fw[ti]) & (t[:, 0] < fw[ti + 1])]
        assert rows.shape[0] > 0 and all(int(c["best_t"][int(r)]) == ti for r in rows[:, 1])
    for o, bt in zip(c["best"], c["best_t"]):
        assert int(o["rhs_id"]) == ids[int(bt)]
    assert (np.diff(c["best_t"].astype(np.int64)) < 0).any()  # reads are not grouped by target


TAG_CHECKS = {"len_9": _check_len_9, "len_10": _check_len_10, "empty_window": _check_empty_window,
              "one_pair": _check_one_pair, "short_tail": _check_short_tail, "q_exact": _check_q_exact,
              "q_oriented": _check_q_oriented, "q_blocks": _check_q_blocks, "ties_130": _check_ties_130,
              "ties_interleaved": _check_ties_interleaved, "unused_and_degenerate": _check_unused_and_degenerate,
              "multi_target": _check_multi_target}


def test_every_tag_has_a_check_and_a_case():
    assert set(TAG_CHECKS) == set(lc.TAGS)
    carried = set().union(*(c["tags"] for c in _cases().values()))
    assert carried == set(lc.TAGS), set(lc.TAGS) ^ carried


@pytest.mark.parametrize("name", sorted(_cases()))
def test_case_is_what_its_tags_say(name):
    c, t = _cases()[name], _table(name)
    assert c["tags"] and c["tags"] <= set(lc.TAGS)
    assert c["best"].shape[0] == c["best_t"].shape[0] == c["reads"].n
    assert c["targets"].n >= 1 and max(int(x) for x in c["targets"].lengths) <= 2500
    rows, pieces = _rows(t), _pieces(t)
    assert c["present"] or c["absent"] or "multi_target" in c["tags"] or "q_blocks" in c["tags"]
    for row in c["present"]:
        assert tuple(row) in rows, row
    for piece in c["absent"]:
        assert tuple(piece) not in pieces, piece
    for tag in sorted(c["tags"]):
        TAG_CHECKS[tag](c, t)
    # every used read with a non-empty span lies inside its read and its target
    for r, (o, bt) in enumerate(zip(c["best"], c["best_t"])):
        if int(bt) != lc.UNUSED:
            assert int(o["lhs_begin"]) <= int(o["lhs_end"]) <= int(c["reads"].lengths[r])
            assert int(o["rhs_begin"]) <= int(o["rhs_end"]) <= int(c["targets"].lengths[int(bt)])


def test_polished_rule_of_the_counts_is_the_oracles():
    """counts() calls a window polished iff at least two layers beside the backbone survive (racon: a window of fewer than
    three sequences returns its backbone): the oracle's Window::GenerateConsensus says the same of every window of every
    case, windows of exactly one and of exactly two layers among them."""
    seen = set()
    for name, c in sorted(_cases().items()):
        t = _table(name)
        cons, polished = lc.reference_consensus(c, t)
        k = lc.counts(c, t)
        assert polished == k["polished"], name
        assert len(cons) == c["targets"].n and all(len(x) > 0 for x in cons)
        seen |= set(np.bincount(t[:, 0].astype(np.int64), minlength=k["n_windows"]).tolist())
    assert {0, 1, 2} <= seen
