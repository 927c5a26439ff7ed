"""GPU: the chain stage of Map (raven_amd/csrc/chain.hip: chain_matches — group sort, diagonal bands, position sort,
chain_small_kernel / chain_wave, emission, overlap slots) against ram's Chain on crafted match lists.

Every test feeds host match lists to Engine.shard_chain (rvn_shard_chain runs exactly chain_matches; the reads give only
ids and lengths) and compares, read by read, ovl[off[i]:off[i + 1]] with oracle.Engine.chain(ids[i], grp_i, pos_i) of an
oracle engine built with the same parameters: all eight fields, in order, no tolerance, no case left out.  The oracle is
held to a second statement of ram's Chain on the same inputs in tests/test_chain_reference.py, which also checks that the
generators (tests/chain_util.py) build the sizes and chain lengths named here.
"""
import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip, seqio
from tests import chain_util as cu
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

W = 5
NON_DEFAULT = cu.PARAM_SETS[1:]
_pid = lambda p: "-".join(map(str, p))


@pytest.fixture(scope="module")
def gpu():
    if hip.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return True


@pytest.fixture(scope="module")
def engines(gpu):
    """(k, params) -> (hip engine, oracle engine), made once per module."""
    made = {}

    def get(k, params):
        if (k, params) not in made:
            made[(k, params)] = (hip.Engine(k, W, *params), oracle.Engine(k, W, *params))
        return made[(k, params)]

    yield get
    for he, _ in made.values():
        he.close()


def _upload(he, ids):
    """Reads that carry the ids (the chain stage reads nothing else of them)."""
    return he.upload(seqio.pack_reads([np.zeros(7, np.uint8)] * int(ids.shape[0]), ids=ids))


def _mismatches(oe, ids, grp, pos, seg, ovl, off):
    errs = []
    total = 0
    assert off.shape[0] == ids.shape[0] + 1 and int(off[0]) == 0 and int(off[-1]) == ovl.shape[0]
    for i in range(ids.shape[0]):
        s, e = int(seg[i]), int(seg[i + 1])
        want = oe.chain(int(ids[i]), grp[s:e], pos[s:e])
        got = ovl[int(off[i]):int(off[i + 1])]
        total += want.shape[0]
        if got.shape[0] != want.shape[0] or not np.array_equal(got, want):
            d = pu.first_diff(got, want)
            errs.append("read %d (id %d, %d matches): device %d overlaps, ram %d; first difference at %s: device %s ram %s" % (
                i, ids[i], e - s, got.shape[0], want.shape[0], d, got[d:d + 1], want[d:d + 1]))
    return errs, total


def _check(engines, k, params, built):
    he, oe = engines(k, params)
    ids, grp, pos, seg = built
    rd = _upload(he, ids)
    ovl, off = he.shard_chain(rd, grp, pos, seg)
    errs, total = _mismatches(oe, ids, grp, pos, seg, ovl, off)
    rd.close()
    assert errs == [], errs[:4]
    return ovl, off, total


def test_every_size_class_in_one_call(engines):
    """One batch, one call, and the launch counts say that every class ran: the class tables of sizeclass.h restated —
    group sort of a read (kSegClassTable): LDS for <= 256 / 512 / 1024 / 2048 / 4096 matches + the wave sort beyond = 6;
    position sort and chain of an interval above 32 matches (kChainClassTable): LDS for <= 128 / 256 / 512 / 768 / 1024 /
    2048 / 4096 / 8192 + global scratch beyond = 9 each; chain_small (<= kChainSmallCap = 32): one launch."""
    he, _ = engines(15, cu.DEFAULT_PARAMS)
    b, _ = cu.class_batch()
    he.set_kernel_timing(True)
    he.reset_stats()
    try:
        _, _, total = _check(engines, 15, cu.DEFAULT_PARAMS, b.build())
        launches = {name: n for name, (ms, n) in he.kernel_ms().items()}
    finally:
        he.set_kernel_timing(False)
    assert total > 100
    assert launches["seg_sort_group"] == len(cu.SEG_CLASS_CAPS) + 1
    assert launches["seg_sort_pos"] == len(cu.CHAIN_CLASS_CAPS) + 1
    assert launches["chain"] == len(cu.CHAIN_CLASS_CAPS) + 1
    assert launches["chain_small"] == 1
    assert launches["intervals"] == 1


@pytest.mark.parametrize("flip", [0, 1])
def test_every_search_regime(engines, flip):
    """Colinear prefixes of 63 / 64 / 65, 511 / 512 / 513, 4095 / 4096 / 4097 and 5000 matches followed by descending
    noise, a sawtooth and a tie grid, in LDS classes and on the global path; ties, saw, anti and late on their own; n = 0,
    1 and 63 mod 64.  flip swaps the strands."""
    b, _ = cu.regime_batch(flip=flip)
    _, _, total = _check(engines, 15, cu.DEFAULT_PARAMS, b.build())
    assert total >= 40


@pytest.mark.parametrize("params", cu.PARAM_SETS, ids=_pid)
@pytest.mark.parametrize("k", [5, 15, 31])
def test_scores_gaps_bands_on_every_engine(engines, k, params):
    """Every family — steps (spacings of k - 1 / k / k + 1), gaps (differences of gap / gap + 1, pieces around `chain`,
    scores of exactly `matches` and one below), band (diagonals bandwidth / bandwidth + 1 apart, windows of 3 and 4, the
    extend rule, a drifting diagonal) among them — on both strands, for the default and five other engines."""
    _, _, total = _check(engines, k, params, cu.mixed_batch(100 + k, k, params).build())
    assert total > 0


@pytest.mark.parametrize("chain", [1, 2, 3, 4, 7])
def test_slot_capacity(engines, chain):
    """Every `chain` matches one overlap: each interval fills its slot region ceil(b / min(4, chain)) ... to the last slot,
    neighbours back to back, in the small kernel, in LDS classes and on the global path."""
    params = (100, chain, 0, 50)
    b, listed = cu.slots_batch(3, chain)
    ovl, off, total = _check(engines, 15, params, b.build())
    for read in range(len(b.reads)):
        assert int(off[read + 1]) - int(off[read]) == sum(n // chain for r, n in listed if r == read)
    assert total == sum(n // chain for _, n in listed)


@pytest.mark.parametrize("chain", [33, 40])
def test_chain_above_the_small_kernel(engines, chain):
    """Nothing for the small kernel; intervals between 32 and `chain` matches are skipped by both kernels."""
    _, _, total = _check(engines, 15, (100, chain, 0, 50), cu.above_small_batch(4, chain).build())
    assert total > 0


@pytest.mark.parametrize("minhash", [False, True])
@pytest.mark.parametrize("params", NON_DEFAULT, ids=_pid)
def test_map_lambda_on_non_default_engines(gpu, lambda_reads, params, minhash):
    """The whole Map, end to end, with non-default bandwidth / chain / matches / gap."""
    rs = lambda_reads
    he, oe = hip.Engine(15, W, *params), oracle.Engine(15, W, *params)
    rd = he.upload(rs)
    he.minimize(rd, 0, rs.n, minhash)
    oe.minimize(rs, 0, rs.n, minhash)
    he.filter(0.001)
    oe.filter(0.001)
    errs, n = pu.compare_map(he, oe, rd, rs, 0, rs.n if minhash else 96, minhash)
    he.close()
    assert errs == [] and n > 0


@pytest.mark.parametrize("params", [NON_DEFAULT[1], NON_DEFAULT[2], NON_DEFAULT[3]], ids=_pid)
def test_pass1_lambda_on_non_default_engines(gpu, lambda_reads, params):
    he, oe = hip.Engine(15, W, *params), oracle.Engine(15, W, *params)
    rd = he.upload(lambda_reads)
    errs, _ = pu.compare_pass1(he, oe, rd, lambda_reads)
    he.close()
    assert errs == []


def test_order_inside_a_segment_does_not_matter(engines):
    he, _ = engines(15, cu.DEFAULT_PARAMS)
    out = []
    for shuffle in (0, 1):
        b = cu.mixed_batch(6, 15, cu.DEFAULT_PARAMS)
        b.add_read([b.interval("ties", 8192 + 127, 1), b.interval("saw", 5000, 0), b.interval("late", 700, 1)])
        ids, grp, pos, seg = b.build(shuffle_seed=shuffle)
        rd = _upload(he, ids)
        out.append((grp, he.shard_chain(rd, grp, pos, seg)))
        rd.close()
    assert not np.array_equal(out[0][0], out[1][0])  # the two inputs do differ in order
    assert out[0][1][0].shape[0] > 0
    assert out[0][1][0].tobytes() == out[1][1][0].tobytes() and out[0][1][1].tobytes() == out[1][1][1].tobytes()


def test_device_pointer_form_gives_the_same_bytes(engines):
    import torch
    he, _ = engines(15, cu.DEFAULT_PARAMS)
    ids, grp, pos, seg = cu.mixed_batch(9, 15, cu.DEFAULT_PARAMS).build()
    rd = _upload(he, ids)
    ovl, off = he.shard_chain(rd, grp, pos, seg)
    dev = torch.device("cuda", 0)
    # (torch has no uint64: the same bits as int64)
    d_grp, d_pos, d_seg = (torch.from_numpy(x.view(np.int64)).to(dev) for x in (grp, pos, seg))
    torch.cuda.synchronize()
    n = he.shard_chain_dev(rd, d_grp.data_ptr(), d_pos.data_ptr(), d_seg.data_ptr(), grp.shape[0])
    d_ovl = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    d_off = torch.zeros(rd.n + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (the engine copies on its own stream: torch's fills must be done first)
    he.map_fetch_dev(d_ovl.data_ptr(), d_off.data_ptr())
    ovl2, off2 = d_ovl.cpu().numpy(), d_off.cpu().numpy()
    rd.close()
    assert n == ovl.shape[0] and n > 0
    assert ovl2.tobytes() == ovl.tobytes() and off2.tobytes() == off.tobytes()


def test_degenerate_batches(engines):
    he, oe = engines(15, cu.DEFAULT_PARAMS)
    none = np.zeros(0, np.uint64)
    # all reads empty (H = 0), with and without match arrays
    ids = np.array([5, 9, 12], np.uint32)
    rd = _upload(he, ids)
    ovl, off = he.shard_chain(rd, none, none, np.zeros(4, np.uint64))
    assert ovl.shape[0] == 0 and off.tolist() == [0, 0, 0, 0]
    # matches, but no read has an interval
    b = cu.Batch(1)
    for n in (3, 0, 2):
        b.add_read([b.loose(n)] if n else [])
    _, grp, pos, seg = b.build()
    ovl, off = he.shard_chain(rd, grp, pos, seg)
    assert ovl.shape[0] == 0 and off.tolist() == [0, 0, 0, 0]
    rd.close()
    # a single read with exactly four matches (k = 31 so that four matches can score 100)
    b = cu.Batch(2)
    b.add_read([b.interval("steps", 4, 0, 31, cu.DEFAULT_PARAMS)])
    ovl, off, total = _check(engines, 31, cu.DEFAULT_PARAMS, b.build())
    assert total == 1 and off.tolist() == [0, 1]
