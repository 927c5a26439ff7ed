"""edit_distance_dev (raven_amd/csrc/edit_distance.hip) on the device over the cases of tests/ed_ring_cases.py, through
rvn_test_edit_distance_dev — the function the identity filters and RemoveBubbles' similarity test call, with the pairs,
the thresholds and the route chosen here: the wave ring at its thresholds, capacity and wraps, the workgroup ring at
L = 64 / 128 / 512 lanes, the striped sweep at one, two and three stripes.  One call per class (per L for the workgroup
ring): every stored value equals the model's (the exact DP distance, or "above"), and the launches per kernel site equal
the model's prediction.  Three classes also go through the product's own doors (rvn_edit_distance_batch,
rvn_path_similarity_batch) and give what the hook gave.  tests/test_ed_ring_cases.py holds the cases to the DP and to
what their classes promise, without a GPU."""
import ctypes as C

import numpy as np
import pytest

from raven_amd import hip
from tests import ed_ring_cases as ec

pytestmark = pytest.mark.gpu

SITES = ("edit_lane", "edit_banded", "edit_wide", "edit_full")


@pytest.fixture(scope="module")
def D():
    return ec.distances()


@pytest.fixture(scope="module")
def hook():
    e = hip.HookEngine(15)
    yield e
    e.close()


@pytest.fixture(scope="module")
def engine():
    e = hip.Engine(15, 5)
    e.set_kernel_timing(True)
    return e


def _records(pairs):
    return np.ascontiguousarray(pairs, dtype=np.uint32).view(hip.ED_PAIR_DTYPE).reshape(-1)


def _run(hook, some, D, L=0, placed=None):
    """One call on the cases `some` by route L: values and launches against the model.  Returns (values, read set, pairs)."""
    rs, pairs, kmax = placed if placed is not None else ec.place(some)
    shapes = [ec.shape(c, D[c["seq"]]) for c in some]
    want = np.array([ec.expected(*s, int(L != 0), L) for s in shapes], dtype=np.uint32)
    h = hook.upload(rs)
    try:
        if L:
            hook.set_option("ed_wide_lanes", L)
        hook.count_launches()
        got = hook.edit_distance_dev(h, _records(pairs), kmax, wide_sweep=L != 0)
        la = {k: v for k, v in hook.launches().items() if k.startswith("edit_")}
    finally:
        hook.count_launches(False)
        hook.set_option("ed_wide_lanes", -1)
        hook.reads_destroy(h)
    bad = [(c["name"], s, int(g), int(w)) for c, s, g, w in zip(some, shapes, got, want) if g != w]
    assert np.array_equal(got, want), (len(bad), bad[:8])
    assert set(la) == set(SITES) and la == ec.launches(shapes, int(L != 0), L), (la, ec.launches(shapes, int(L != 0), L))
    return got, rs, pairs


def _same_through_edit_distance_batch(engine, some, got, rs, pairs):
    """rvn_edit_distance_batch on the same read set and records (the cases have no threshold): the hook's values."""
    assert all(c["km"] is None and c["L"] == 0 for c in some)
    engine.reset_stats()
    out, _, cells = engine.edit_distance_batch(engine.upload(rs), _records(pairs))
    assert np.array_equal(out, got) and cells == sum(int(p[2]) * int(p[5]) for p in pairs)


@pytest.mark.parametrize("tag", ["thr_edge", "cap_edge", "ring_reuse", "full"])
def test_class_through_the_hook_and_through_edit_distance_batch(hook, engine, D, tag):
    some = ec.by_tag(tag)
    got, rs, pairs = _run(hook, some, D)
    _same_through_edit_distance_batch(engine, some, got, rs, pairs)
    if tag == "full":  # every pair ended in the striped sweep, in one launch (its boundary rows at offsets of different m)
        assert all(int(g) == D[c["seq"]] > ec.CAP for g, c in zip(got, some))


@pytest.mark.parametrize("tag", ["geometry", "retire", "text_side", "bounded"])
def test_class_through_the_hook(hook, D, tag):
    some = ec.by_tag(tag)
    got, _, _ = _run(hook, some, D)
    if tag == "bounded":
        assert {int(g) == ec.ABOVE for g in got} == {True, False}


@pytest.mark.parametrize("L", [64, 128, 512, 1])
def test_wide(hook, engine, D, L):
    """wide_sweep = 1 with ed_wide_lanes = L; the whole-read forward members also through rvn_path_similarity_batch, which
    derives the same thresholds from its ratio and reports what lies above them uniformly as "above"."""
    some = [c for c in ec.by_tag("wide") if c["L"] == L]
    got, rs, pairs = _run(hook, some, D, L)
    whole = [i for i, c in enumerate(some) if c["ratio"] is not None]
    assert bool(whole) == (L != 1)
    rd = engine.upload(rs)
    for ratio in sorted({some[i]["ratio"] for i in whole}):
        idx = [i for i in whole if some[i]["ratio"] == ratio]
        engine.set_option("ed_wide_lanes", L)
        try:
            engine.reset_stats()
            similar, distance = engine.path_similarity(rd, [(int(pairs[i][0]), int(pairs[i][3])) for i in idx], ratio)
            la = {k: v[1] for k, v in engine.kernel_ms().items() if k.startswith("edit_")}
        finally:
            engine.set_option("ed_wide_lanes", -1)
        want = [int(got[i]) if int(got[i]) <= some[i]["km"] else ec.ABOVE for i in idx]
        assert distance.tolist() == want and similar.tolist() == [int(w != ec.ABOVE) for w in want]
        assert la == ec.launches([ec.shape(some[i], D[some[i]["seq"]]) for i in idx], 1, L), la


def test_batch_shares_of_the_wave_ring(hook, D):
    """Calls that leave exactly 1, 3, 4 and 5 pairs to the wave ring (four pairs share a workgroup), scattered among pairs
    the lane stage decides: every answer at its own index."""
    pool = ec.by_tag("batch")
    for share, idx in ec.batch_calls().items():
        some = [pool[i] for i in idx]
        got, _, _ = _run(hook, some, D)
        assert sum(ec.leaves_lane(*ec.shape(c, D[c["seq"]])) for c in some) == share


def test_every_case_in_one_call_and_the_same_call_permuted(hook, D):
    """Every case of every class on the usual route in one call (the members of the workgroup ring's class included: their
    thresholds and spans, swept by the wave ring), then the same records in another order: the lists of the wave ring and of
    the striped sweep are collected with atomics, and every answer lands at its own index."""
    some = list(ec.cases())
    placed = ec.place(some)
    got, rs, pairs = _run(hook, some, D, placed=placed)
    order = np.random.default_rng(8300).permutation(len(some))
    assert not np.array_equal(order, np.arange(len(some)))
    kmax = placed[2]
    again, _, _ = _run(hook, [some[i] for i in order], D, placed=(rs, pairs[order], kmax[order]))
    assert np.array_equal(again, got[order])


def test_the_hook_refuses_before_anything_is_launched(hook):
    some = ec.by_tag("geometry")[:2]
    rs, pairs, _ = ec.place(some)
    h = hook.upload(rs)
    try:
        hook.count_launches()
        rec = _records(pairs)
        for field, value in (("lhs_read", rs.n), ("rhs_read", rs.n), ("lhs_len", int(rs.lengths[2]) - int(rec[1]["lhs_begin"]) + 1),
                             ("rhs_begin", int(rs.lengths[3])), ("rhs_len", 0xFFFFFFFF)):
            bad = rec.copy()
            bad[1][field] = value
            with pytest.raises(ValueError, match="rvn_test_edit_distance_dev: span outside its read"):
                hook.edit_distance_dev(h, bad)
        with pytest.raises(ValueError, match="wide_sweep is 0 or 1"):
            hook.edit_distance_dev(h, rec, wide_sweep=2)
        with pytest.raises(ValueError, match="wide_sweep is 0 or 1"):
            hook.edit_distance_dev(h, rec, wide_sweep=-1)
        T = hip.test_lib()
        out = np.zeros(2, np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        for args in ((None, h, p(rec), 2, None, 0, p(out)), (hook._h, None, p(rec), 2, None, 0, p(out)),
                     (hook._h, h, None, 2, None, 0, p(out)), (hook._h, h, p(rec), 2, None, 0, None)):
            assert T.rvn_test_edit_distance_dev(*args) == hip.RVN_EINVAL
            assert b"rvn_test_edit_distance_dev: NULL argument" in T.rvn_last_error()
        assert sum(v for k, v in hook.launches().items()) == 0      # nothing ran for any of them
        assert hook.edit_distance_dev(h, rec[:0]).shape == (0,)     # an empty call: nothing to do
        assert hook.edit_distance_dev(h, rec).tolist() == [400, 400]
    finally:
        hook.count_launches(False)
        hook.reads_destroy(h)
