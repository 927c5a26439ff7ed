"""rvn_align_path_batch (Engine.align_paths) on the device: the alignment paths of the polishing front end as a result.
Reference = a numpy DP with traceback under the stated tie rule (tests/nw_ops_util.py): runs equal word for word, distances
equal, no tolerance.  Second, independent check: racon's window breakpoints derived from the device's runs equal
oracle.nw_breakpoints.  Every walk form, the striped sweeps and a chunked pass give the default's runs."""
import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip
from tests import nw_ops_util as U

pytestmark = pytest.mark.gpu

NOT_ALIGNED = 0xFFFFFFFF


def _rnd(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def _mutate(rng, s, sub, ins, dele):
    s = np.asarray(s, dtype=np.uint8)
    r = rng.random(len(s))
    out = s.copy()
    is_sub = r < sub
    out[is_sub] = (out[is_sub] + rng.integers(1, 4, size=int(is_sub.sum()))) % 4
    is_ins = (r >= sub) & (r < sub + ins)
    is_del = (r >= sub + ins) & (r < sub + ins + dele)
    cnt = np.ones(len(s), dtype=np.int64)
    cnt[is_ins] = 2
    cnt[is_del] = 0
    out = np.repeat(out, cnt)
    pos = np.cumsum(cnt)[is_ins] - 1
    out[pos] = rng.integers(0, 4, size=len(pos))
    return out.astype(np.uint8)


def _revcomp(c):
    return (3 - np.asarray(c, dtype=np.uint8)[::-1]).astype(np.uint8)


def _families():
    """[(name, query, target)]: the alignment is query (columns) against target (rows)"""
    rng = np.random.default_rng(355)
    fam = []
    ont = lambda t: _mutate(rng, t, 0.04, 0.03, 0.03)
    for n, reps in ((500, 3), (2000, 2), (5000, 3)):
        for x in range(reps):
            t = _rnd(rng, n)
            fam.append(("ont_%d_%d" % (n, x), ont(t), t))
    for x in range(2):
        t = _rnd(rng, 2000)
        fam.append(("hifi_2000_%d" % x, _mutate(rng, t, 0.002, 0.0015, 0.0015), t))
    for rows in (1, 63, 64, 65, 127, 128, 129):  # rows = target span
        t = _rnd(rng, rows)
        fam.append(("rows_%d" % rows, ont(np.concatenate((t, _rnd(rng, 3)))) if rows > 1 else _rnd(rng, 2), t))
    for cols in (16, 17, 32, 33, 64, 65):  # columns = query span: the hs word, the checkpoint interval, a block
        t = _rnd(rng, cols + 4)
        q = ont(t)
        q = np.concatenate((q, _rnd(rng, cols)))[:cols]
        fam.append(("cols_%d" % cols, q, t))
    t = _rnd(rng, 700)
    fam.append(("identical_700", t.copy(), t))
    t = _rnd(rng, 1)
    fam.append(("identical_1", t.copy(), t))
    t = _rnd(rng, 900)
    fam.append(("burst_ins", np.concatenate((t[:300], _rnd(rng, 80), t[300:700], _rnd(rng, 33), t[700:])), t))
    fam.append(("burst_del", np.concatenate((t[:200], t[290:600], t[664:])), t))
    hp = np.concatenate((_rnd(rng, 150), np.full(90, 1, np.uint8), _rnd(rng, 150)))
    fam.append(("homopolymer", np.concatenate((hp[:180], hp[191:])), hp))
    fam.append(("homopolymer_all", np.zeros(140, np.uint8), np.zeros(100, np.uint8)))
    tr = np.concatenate((_rnd(rng, 100), np.tile(np.array([2, 3], np.uint8), 70), _rnd(rng, 100)))
    fam.append(("tandem", ont(np.concatenate((tr[:150], tr[164:]))), tr))
    fam.append(("unrelated_300_2000", _rnd(rng, 300), _rnd(rng, 2000)))
    fam.append(("unrelated_2000_300", _rnd(rng, 2000), _rnd(rng, 300)))
    fam.append(("unrelated_600_600", _rnd(rng, 600), _rnd(rng, 600)))
    fam.append(("empty_query", np.zeros(0, np.uint8), _rnd(rng, 40)))
    fam.append(("empty_target", _rnd(rng, 70), np.zeros(0, np.uint8)))
    fam.append(("empty_both", np.zeros(0, np.uint8), np.zeros(0, np.uint8)))
    return fam


class Batch:
    """Every family on both strands, the spans in the middle of their reads (pads of different lengths on the two
    sides: on the reverse strand query_begin counts in the read as stored).  One read set holds queries and targets
    (reads 2p, 2p + 1); `split` addresses the same reads in a query set and a target set of their own."""

    def __init__(self):
        rng = np.random.default_rng(950)
        self.fam = _families()
        self.ref = {name: U.dp_runs(q, t) for name, q, t in self.fam}  # computed once, shared, left unchanged
        self.reads, self.items = [], []
        pairs = []
        for name, q, t in self.fam:
            for strand in (1, 0):
                qa, qb = _rnd(rng, int(rng.integers(0, 40))), _rnd(rng, int(rng.integers(41, 90)))
                ta, tb = _rnd(rng, int(rng.integers(0, 700))), _rnd(rng, int(rng.integers(0, 30)))
                p = len(self.items)
                self.reads.append(np.concatenate((qa, q if strand else _revcomp(q), qb)))
                self.reads.append(np.concatenate((ta, t, tb)))
                pairs.append((2 * p, len(qa), len(q), 2 * p + 1, len(ta), len(t), strand, 0))
                self.items.append((name, strand))
        self.pairs = np.array(pairs, dtype=hip.ALIGN_PAIR_DTYPE)
        self.split = self.pairs.copy()
        self.split["query_read"] //= 2
        self.split["target_read"] //= 2

    def check(self, dist, off, runs):
        assert off[0] == 0 and off[-1] == len(runs)
        for p, (name, strand) in enumerate(self.items):
            want_d, want = self.ref[name]
            got = runs[int(off[p]):int(off[p + 1])]
            assert dist[p] == want_d, (name, strand)
            assert np.array_equal(got, want), (name, strand, got[:6], want[:6])


@pytest.fixture(scope="module")
def batch():
    return Batch()


@pytest.fixture(scope="module")
def eng():
    return hip.Engine(15, 5)


@pytest.fixture(scope="module")
def default_result(batch, eng):
    both = eng.upload_codes(batch.reads)
    return eng.align_paths(both, both, batch.pairs)


def test_runs_equal_dp_traceback(batch, default_result):
    dist, off, runs, n_bad = default_result
    assert n_bad == 0
    batch.check(dist, off, runs)
    for p, (name, _) in enumerate(batch.items):
        _, q, t = next(f for f in batch.fam if f[0] == name)
        U.check_runs(runs[int(off[p]):int(off[p + 1])], q, t, int(dist[p]))


def test_empty_spans(batch, default_result):
    dist, off, runs, _ = default_result
    for p, (name, _) in enumerate(batch.items):
        got = runs[int(off[p]):int(off[p + 1])].tolist()
        if name == "empty_query":
            assert (int(dist[p]), got) == (40, [(40 << 2) | U.OP_D])
        elif name == "empty_target":
            assert (int(dist[p]), got) == (70, [(70 << 2) | U.OP_I])
        elif name == "empty_both":
            assert (int(dist[p]), got) == (0, [])
        elif name.startswith("identical"):
            assert int(dist[p]) == 0 and len(got) == 1 and got[0] & 3 == U.OP_EQ


def test_two_read_sets_give_the_same(batch, eng, default_result):
    queries = eng.upload_codes(batch.reads[0::2])
    targets = eng.upload_codes(batch.reads[1::2])
    got = eng.align_paths(queries, targets, batch.split)
    for a, b in zip(got, default_result):
        assert np.array_equal(a, b)


def test_breakpoints_from_runs_equal_oracle(batch, default_result):
    """racon's find_breaking_points over the device's runs = the oracle's, windows of 500 (positions in the stored
    target read, query positions in the orientation the span is aligned in)"""
    _, off, runs, _ = default_result
    seen = 0
    for p, (name, strand) in enumerate(batch.items):
        _, q, t = next(f for f in batch.fam if f[0] == name)
        if len(q) == 0 or len(t) == 0:
            continue
        pr = batch.pairs[p]
        qlen = len(batch.reads[2 * p])
        q_begin = int(pr["query_begin"]) if strand else qlen - int(pr["query_begin"]) - int(pr["query_len"])
        t_begin = int(pr["target_begin"])
        want, _ = oracle.nw_breakpoints(q, t, q_begin, t_begin, 500)
        got = U.breakpoints_from_runs(runs[int(off[p]):int(off[p + 1])], q_begin, t_begin, t_begin + len(t), 500)
        assert np.array_equal(got, want), (name, strand)
        seen += 1
    assert seen > 40


@pytest.mark.parametrize("option,value", [("nw_group_walk", 1), ("nw_group_walk", 2), ("nw_group_walk", 3),
                                          ("nw_stripe_lanes", 1), ("nw_stripe_lanes", 2), ("nw_stripe_lanes", 4),
                                          ("nw_budget_mb", 64)])
def test_every_walk_form_and_stripes(batch, eng, default_result, option, value):
    both = eng.upload_codes(batch.reads)
    eng.set_option(option, value)
    try:
        got = eng.align_paths(both, both, batch.pairs)
    finally:
        eng.set_option(option, 0)
    for a, b in zip(got, default_result):
        assert np.array_equal(a, b)


def test_several_chunks(eng):
    """a batch whose stored band words exceed the smallest budget several times over: chunks on rotating buffer sets, a
    block of slots per pass; same runs as in one chunk"""
    rng = np.random.default_rng(64)
    g = _rnd(rng, 120_000)
    reads, pairs = [], []
    for p in range(600):
        n = int(rng.integers(3000, 6000))
        b = int(rng.integers(0, len(g) - n))
        t = g[b:b + n]
        q = _mutate(rng, t, 0.04, 0.03, 0.03)
        strand = p & 1
        reads += [q if strand else _revcomp(q), t]
        pairs.append((2 * p, 0, len(q), 2 * p + 1, 0, n, strand, 0))
    pairs = np.array(pairs, dtype=hip.ALIGN_PAIR_DTYPE)
    both = eng.upload_codes(reads)
    one = eng.align_paths(both, both, pairs)
    eng.set_option("nw_budget_mb", 64)
    try:
        many = eng.align_paths(both, both, pairs)
    finally:
        eng.set_option("nw_budget_mb", 0)
    assert one[3] == 0
    for a, b in zip(one, many):
        assert np.array_equal(a, b)
    # (same layout; strand 0 turns the rhs there and the query here: the distance is the same)
    d2, _, _ = eng.edit_distance_batch(both, pairs.view(hip.ED_PAIR_DTYPE))
    assert np.array_equal(one[0], d2)


def test_batch_large_enough_for_pilot_and_head(eng):
    """4 096 jobs and more take the stage's full schedule: a pilot swept for its distances only (no slots), the longest
    alignments as a pass of their own with compact job arrays, the rest behind them — every pass with its own block of slots"""
    rng = np.random.default_rng(4500)
    g = _rnd(rng, 100_000)
    reads, pairs, qs, ts = [], [], [], []
    for p in range(4500):
        n = int(rng.integers(100, 700))
        b = int(rng.integers(0, len(g) - n))
        t = g[b:b + n]
        q = _mutate(rng, t, 0.04, 0.03, 0.03) if p % 50 else _rnd(rng, n)  # (unrelated ones: beyond the threshold, repeated)
        strand = p & 1
        reads += [q if strand else _revcomp(q), t]
        pairs.append((2 * p, 0, len(q), 2 * p + 1, 0, n, strand, 0))
        qs.append(q)
        ts.append(t)
    pairs = np.array(pairs, dtype=hip.ALIGN_PAIR_DTYPE)
    both = eng.upload_codes(reads)
    dist, off, runs, n_bad = eng.align_paths(both, both, pairs)
    assert n_bad == 0
    d2, _, _ = eng.edit_distance_batch(both, pairs.view(hip.ED_PAIR_DTYPE))
    assert np.array_equal(dist, d2)
    for p in range(4500):
        U.check_runs(runs[int(off[p]):int(off[p + 1])], qs[p], ts[p], int(dist[p]))
    for p in range(0, 4500, 450):
        want_d, want = U.dp_runs(qs[p], ts[p])
        assert dist[p] == want_d and np.array_equal(runs[int(off[p]):int(off[p + 1])], want)


def test_mixed_batch_order_offsets_ops(eng):
    rng = np.random.default_rng(3000)
    g = _rnd(rng, 300_000)
    n_pairs = 3000
    lens = rng.integers(0, 3001, size=n_pairs)
    lens[:6] = (0, 0, 1, 3000, 64, 0)
    rng.shuffle(lens)
    reads, pairs, qs, ts = [], [], [], []
    for p, n in enumerate(lens):
        b = int(rng.integers(0, len(g) - 3000))
        t = g[b:b + int(n)]
        q = _mutate(rng, t, 0.04, 0.03, 0.03) if p % 7 else _rnd(rng, int(rng.integers(0, 200)))
        strand = int(rng.integers(0, 2))
        reads += [q if strand else _revcomp(q), t]
        pairs.append((2 * p, 0, len(q), 2 * p + 1, 0, len(t), strand, 0))
        qs.append(q)
        ts.append(t)
    pairs = np.array(pairs, dtype=hip.ALIGN_PAIR_DTYPE)
    both = eng.upload_codes(reads)
    dist, off, runs, n_bad = eng.align_paths(both, both, pairs)
    assert n_bad == 0 and len(dist) == n_pairs and len(off) == n_pairs + 1
    assert off[0] == 0 and off[-1] == len(runs) and (np.diff(off.astype(np.int64)) >= 0).all()
    for p in range(n_pairs):  # pair order: every pair's runs consume exactly ITS spans
        U.check_runs(runs[int(off[p]):int(off[p + 1])], qs[p], ts[p], int(dist[p]))
    for p in range(0, n_pairs, 97):  # and '=' / 'X' agree with the bases
        ops = U.expand_runs(runs[int(off[p]):int(off[p + 1])])
        qi = np.cumsum((ops != U.OP_D)) - 1
        ti = np.cumsum((ops != U.OP_I)) - 1
        eq, x = ops == U.OP_EQ, ops == U.OP_X
        assert (qs[p][qi[eq]] == ts[p][ti[eq]]).all() and (qs[p][qi[x]] != ts[p][ti[x]]).all()
    d2, _, _ = eng.edit_distance_batch(both, pairs.view(hip.ED_PAIR_DTYPE))
    assert np.array_equal(dist, d2)
    # the ops form: edlib's bytes, expanded on the device
    dist_o, op_off, ops, _ = eng.align_paths(both, both, pairs, ops=True)
    assert np.array_equal(dist_o, dist)
    assert np.array_equal(ops, U.expand_runs(runs))
    per_pair = [int((runs[int(off[p]):int(off[p + 1])] >> 2).sum()) for p in range(n_pairs)]
    assert np.array_equal(op_off, np.concatenate(([0], np.cumsum(per_pair))).astype(np.uint64))
    # the same call again on the same engine: the same bytes
    again = eng.align_paths(both, both, pairs)
    assert np.array_equal(again[0], dist) and np.array_equal(again[1], off) and again[2].tobytes() == runs.tobytes()


def test_pair_beyond_the_band_limit_is_not_aligned():
    """The rule of nwpath.hip (plan): a band that no variant's ring holds is swept in stripes of nw_stripe_lanes
    super-blocks, at most eight of them; with nw_stripe_lanes = 1 that is a band of 3 592 diagonals, and an unrelated pair
    of 8 000 bases (distance about 0.53 x 8 000) is beyond it.  It is reported, not an error, and its neighbours are
    untouched."""
    rng = np.random.default_rng(8000)
    t = _rnd(rng, 400)
    small = [(_mutate(rng, t, 0.04, 0.03, 0.03), t), (_rnd(rng, 90), _rnd(rng, 60))]
    reads = [small[0][0], small[0][1], _rnd(rng, 8000), _rnd(rng, 8000), small[1][0], small[1][1]]
    pairs = np.array([(0, 0, len(reads[0]), 1, 0, 400, 1, 0), (2, 0, 8000, 3, 0, 8000, 1, 0),
                      (4, 0, 90, 5, 0, 60, 1, 0)], dtype=hip.ALIGN_PAIR_DTYPE)
    eng = hip.Engine(15, 5)
    eng.set_option("nw_stripe_lanes", 1)
    both = eng.upload_codes(reads)
    dist, off, runs, n_bad = eng.align_paths(both, both, pairs)
    assert n_bad == 1 and dist[1] == NOT_ALIGNED and off[1] == off[2]
    for p, (q, tt) in ((0, small[0]), (2, small[1])):
        want_d, want = U.dp_runs(q, tt)
        assert dist[p] == want_d and np.array_equal(runs[int(off[p]):int(off[p + 1])], want)
    _, op_off, ops, _ = eng.align_paths(both, both, pairs, ops=True)
    assert op_off[1] == op_off[2] and np.array_equal(ops, U.expand_runs(runs))


def test_bad_indices_and_spans_are_einval(eng):
    both = eng.upload_codes([np.zeros(50, np.uint8), np.ones(60, np.uint8)])
    ok = (0, 0, 50, 1, 0, 60, 1, 0)
    eng.align_paths(both, both, np.array([ok], dtype=hip.ALIGN_PAIR_DTYPE))
    for bad in ((2, 0, 50, 1, 0, 60, 1, 0), (0, 0, 50, 2, 0, 60, 1, 0), (0, 1, 50, 1, 0, 60, 1, 0),
                (0, 0, 50, 1, 30, 31, 0, 0)):
        with pytest.raises(ValueError):
            eng.align_paths(both, both, np.array([ok, bad], dtype=hip.ALIGN_PAIR_DTYPE))
