"""The merge stage of a flush of FindOverlapsAndCreatePiles on the device (raven_amd/csrc/pile.hip: piles_merge —
rhs_keys_kernel and the stable sort by rhs, pile_counts_kernel, pile_build_kernel, add_layers_kernel,
truncate_sort_kernel, kept_write_kernel, the kept lists from flush to flush) on the crafted lists of tests/merge_cases.py.
After EVERY flush the coverage of every pile and every list (offsets, all eight fields, the order) must equal the plain
reference of construct.cc:72-107 there (MergeRef; held to the oracle's whole pass by tests/test_merge_cases.py, which
also shows that the cases are what their names say).  Integers, no tolerance.

Every case goes through rvn_shard_piles_create + one rvn_shard_piles_merge per flush; a subset of every family also
through rvn_shard_piles (one shot), rvn_shard_piles_merge_dev / rvn_shard_piles_dev (device pointers of torch tensors)
and rvn_shard_piles_merge_parts_dev (the list cut at lhs boundaries)."""
import numpy as np
import pytest

from raven_amd import hip
from tests import merge_cases as mc

pytestmark = pytest.mark.gpu

MERGE_SITES = ("pile_keys", "pile_counts", "pile_build")
LAYER_SITES = ("add_layers",)
TRUNCATE_SITES = ("truncate_sort", "kept_write")


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(15, 5)
    yield e
    e.close()


def _state(p):
    data, poff = p.piles()
    ovl, ooff = p.overlaps()
    return dict(data=data, pile_offsets=poff, overlaps=ovl, offsets=ooff)


def _host(p, flush, kmax):
    p.merge(flush, kmax)


def _check(eng, name, merge=_host, flushes=None):
    """The case flush by flush through `merge`; the state after every flush against the reference."""
    case, ref = mc.by_name(name), mc.reference(name)
    p = eng.shard_piles_create(case["lengths"])
    try:
        for f, flush in enumerate(case["flushes"][:flushes]):
            merge(p, flush, case["kmax"])
            d = mc.diff_state(_state(p), ref[f])
            assert d is None, "%s after flush %d: %s" % (name, f + 1, d)
    finally:
        p.close()


def _device_overlaps(flush):
    """The overlaps as a torch tensor in HBM (four 64-bit words each); its data_ptr() is what the _dev entries take."""
    import torch
    words = np.ascontiguousarray(flush).view(np.int64).copy() if flush.shape[0] else np.zeros(0, np.int64)
    t = torch.from_numpy(words).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _device(flush, n):
    """(tensor of the overlaps, tensor of Map's per-read offsets) on the device."""
    import torch
    t_off = torch.from_numpy(mc.lhs_offsets(flush, n).view(np.int32).copy()).to(torch.device("cuda", 0))
    t_ovl = _device_overlaps(flush)
    return t_ovl, t_off


@pytest.mark.parametrize("name", mc.names())
def test_every_flush_equals_the_reference(eng, name):
    _check(eng, name)


@pytest.mark.parametrize("name", mc.SUBSET)
def test_one_shot_entries_give_the_same_bytes(eng, name):
    """rvn_shard_piles and rvn_shard_piles_dev: a pass created and its first flush merged in one call."""
    case, want = mc.by_name(name), mc.reference(name)[0]
    flush, n = case["flushes"][0], case["lengths"].shape[0]
    p = eng.shard_piles(case["lengths"], flush, case["kmax"])
    try:
        assert mc.diff_state(_state(p), want) is None, name
    finally:
        p.close()
    t_ovl, t_off = _device(flush, n)
    p = eng.shard_piles_dev(case["lengths"], t_ovl.data_ptr(), t_off.data_ptr(), flush.shape[0], case["kmax"])
    try:
        assert mc.diff_state(_state(p), want) is None, name
    finally:
        p.close()


@pytest.mark.parametrize("name", mc.SUBSET)
def test_device_pointers_give_the_same_bytes(eng, name):
    """rvn_shard_piles_merge_dev: the overlaps and Map's per-read offsets are torch tensors in HBM."""
    n = mc.by_name(name)["lengths"].shape[0]
    keep = []

    def merge(p, flush, kmax):
        t_ovl, t_off = _device(flush, n)
        keep.append((t_ovl, t_off))
        p.merge_dev(t_ovl.data_ptr(), t_off.data_ptr(), flush.shape[0], kmax)

    _check(eng, name, merge)


def _parts_merge(cut):
    """merge through rvn_shard_piles_merge_parts_dev; cut(flush) -> the parts, in ascending lhs order."""
    keep = []

    def merge(p, flush, kmax):
        parts = cut(flush)
        assert sum(x.shape[0] for x in parts) == flush.shape[0]
        tensors = [_device_overlaps(x) for x in parts]
        keep.append(tensors)
        p.merge_parts_dev([(t.data_ptr(), x.shape[0]) for t, x in zip(tensors, parts)], kmax)

    return merge


@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("name", mc.SUBSET)
def test_parts_give_the_same_bytes(eng, name, k):
    _check(eng, name, _parts_merge(lambda flush: mc.split_parts(flush, k)))


@pytest.mark.parametrize("name", mc.SUBSET)
def test_empty_parts_change_nothing(eng, name):
    empty = np.zeros(0, dtype=mc.DT)

    def cut(flush):
        a, b = mc.split_parts(flush, 2)
        return [empty, a, empty, empty, b, empty]

    _check(eng, name, _parts_merge(cut))


def test_a_part_boundary_between_two_queries_of_one_rhs_pile(eng):
    """The reversed entries of a pile keep the queries' order across the boundary of two parts."""
    name = "order:kmax65"
    for flush in mc.by_name(name)["flushes"]:
        assert mc.boundary_between_feeders(flush) is not None

    def cut(flush):
        c, _ = mc.boundary_between_feeders(flush)
        return [flush[:c], flush[c:]]

    _check(eng, name, _parts_merge(cut))


def test_every_site_runs_once_per_flush_that_has_overlaps(eng):
    """Launch counters of the merge, AddLayers and truncation sites: one launch of each per non-empty flush, none for an
    empty one (and the empty flush leaves the state alone)."""
    name = "kmax:17"
    case, ref = mc.by_name(name), mc.reference(name)
    sites = MERGE_SITES + LAYER_SITES + TRUNCATE_SITES
    empty = np.zeros(0, dtype=mc.DT)
    eng.set_kernel_timing(True)
    eng.reset_stats()
    p = eng.shard_piles_create(case["lengths"])
    try:
        launches = lambda: {k: v[1] for k, v in eng.kernel_ms().items() if k in sites}
        assert set(launches()) == set(sites) and not any(launches().values())
        p.merge(empty, case["kmax"])
        assert not any(launches().values())
        done = 0
        for f, flush in enumerate(case["flushes"]):
            assert flush.shape[0] > 0
            p.merge(flush, case["kmax"])
            done += 1
            assert launches() == {k: done for k in sites}, f
            p.merge(empty, case["kmax"])
            assert launches() == {k: done for k in sites}, f
            assert mc.diff_state(_state(p), ref[f]) is None, f
    finally:
        p.close()
        eng.set_kernel_timing(False)
        eng.reset_stats()


def test_refused_lists_leave_the_pass_as_it_was(eng):
    """RVN_EINVAL for a list that is not ordered by lhs, for an id >= n and for lhs_id >= rhs_id (pile_build_kernel's
    order — every reversed entry before the pile's own — is the reference's only for lhs_id < rhs_id); the next valid
    flush gives what it gives in a pass that never saw the bad calls."""
    name = "kmax:16"
    case, ref = mc.by_name(name), mc.reference(name)
    n, kmax = case["lengths"].shape[0], case["kmax"]
    f1, f2 = case["flushes"][0], case["flushes"][1]

    def spoilt(base, i, **fields):
        bad = base.copy()
        for k, v in fields.items():
            bad[k][i] = v
        return bad

    mid = f2.shape[0] // 2
    assert f2["lhs_id"][0] < f2["lhs_id"][-1]
    bad_lists = [
        f2[::-1].copy(),                                                   # descending lhs
        spoilt(f2, mid, rhs_id=n),                                         # rhs id == n
        spoilt(f2, f2.shape[0] - 1, lhs_id=n, rhs_id=n + 1),               # lhs id == n (still ordered)
        spoilt(f2, mid, rhs_id=0xFFFFFFFF),
        spoilt(f2, mid, rhs_id=int(f2["lhs_id"][mid])),                    # lhs_id == rhs_id
        spoilt(f2, f2.shape[0] - 1, rhs_id=int(f2["lhs_id"][-1]) - 1),     # lhs_id > rhs_id
    ]
    p = eng.shard_piles_create(case["lengths"])
    try:
        p.merge(f1, kmax)
        for bad in bad_lists:
            with pytest.raises(ValueError):
                p.merge(bad, kmax)
            assert mc.diff_state(_state(p), ref[0]) is None
        p.merge(f2, kmax)
        assert mc.diff_state(_state(p), ref[1]) is None
    finally:
        p.close()
    for bad in bad_lists:  # the one-shot entry refuses the same lists (and hands out no pass)
        with pytest.raises(ValueError):
            eng.shard_piles(case["lengths"], bad, kmax)
    _check(eng, name)
