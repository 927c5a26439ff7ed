"""Crafted pairs for the alignment-path stage (nwpath.hip with nwplan.h / nwsweep.h / nwtrace.h), their plain reference and
the bookkeeping the stage must show for them.  Shared by tests/test_align_cases.py (CPU: the generators are what their names
say, the prediction equals nwplan.h, the comparison helper notices defects) and tests/test_gpu_align_cases.py (device).

Reference of a pair: tests/nw_ops_util.dp_runs — the full matrix, tie rule diagonal > I > D; nothing here restates the walk.
Pairs of more than DP_MAX_CELLS cells (NO_DP_CASES names them, at most 4) are held to oracle.edit_distance, check_runs and a
replay of the runs on the bases instead: optimal, tie choices unchecked.

Prediction: the restatement tests/test_nw_plan.py already holds against nwplan.h (band, ring_lanes, largest_threshold,
store, plan) + the threshold rule of a batch without a model, k = min(max(floor(rate * max(n, m)) + 16, |n - m|, 16),
n + m), + the schedule of a call whose passes are one chunk each: all jobs; the early retry (a compact pass of at most
4 096 of the jobs beyond their thresholds, doubled); then passes of everything still beyond its threshold, doubled, until
none is left.

A pair is (query, target) as uint8 code arrays: the query's bases are the columns (m), the target's the rows (n)."""
import functools

import numpy as np

from tests import nw_ops_util as U
from tests import test_nw_plan as P

DP_MAX_CELLS = 70_000_000
RATE_LARGE = 4.0  # floor(4 * max(n, m)) + 16 > n + m: every threshold is n + m
HEAD_MAX = P.HEAD_MAX
ALL_LANES, NO_BUDGET = 64, 1 << 62


# ---- bases ---------------------------------------------------------------------------------------------------------------
def rnd(rng, n, letters=4):
    return rng.integers(0, letters, size=n, dtype=np.uint8)


def revcomp(c):
    return (3 - np.asarray(c, dtype=np.uint8)[::-1]).astype(np.uint8)


def mutate(rng, s, sub, ins, dele):
    """ONT-like: every base substituted / followed by an inserted base / deleted with the given probabilities"""
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


def related(rng, n, m):
    """a target of n bases and an ONT-like copy of it cut or padded to m bases"""
    t = rnd(rng, n)
    q = mutate(rng, t, 0.04, 0.03, 0.03)
    q = np.concatenate((q, rnd(rng, max(m - len(q), 0))))[:m]
    return q, t


def mismatches_at(rng, length, positions):
    """(q, t): t over {A, C, G}, q = t with T at `positions`.  T matches no target base, so every such column costs one;
    the all-diagonal path is optimal and, by the tie rule (diagonal wherever optimal), the path: '=' runs cut by 'X'."""
    t = rnd(rng, length, 3)
    q = t.copy()
    q[np.asarray(positions, dtype=np.int64)] = 3
    return q, t


def spread(length, count, first=None):
    """count isolated positions in [1, length - 1): no two adjacent, none at either end (first: the first one, e.g. 0)"""
    assert 2 * count + 2 <= length
    step = (length - 2) // count
    assert step >= 2
    pos = 1 + step * np.arange(count)
    if first is not None:
        pos[0] = first
    return pos


class Case:
    def __init__(self, name, q, t, **meta):
        self.name, self.q, self.t = name, np.asarray(q, np.uint8), np.asarray(t, np.uint8)
        self.n, self.m = len(self.t), len(self.q)
        self.meta = meta

    @property
    def cells(self):
        return self.n * self.m

    def __repr__(self):
        return "Case(%s, n=%d, m=%d)" % (self.name, self.n, self.m)


_REF = {}


def reference(case):
    """(distance, runs) by the DP, once per case name"""
    key = case.meta.get("same_pair_as", case.name)
    if "identical" in case.meta:  # the one path of cost 0; too long for the matrix
        assert np.array_equal(case.q, case.t)
        return 0, np.array([(case.n << 2) | U.OP_EQ], dtype=np.uint32)
    if key not in _REF:
        assert case.cells <= DP_MAX_CELLS, case
        d, runs = U.dp_runs(case.q, case.t)
        runs.setflags(write=False)
        _REF[key] = (d, runs)
    return _REF[key]


def replay(runs, q, t):
    """cost of the runs replayed on the bases: '=' columns equal, 'X' columns differ, both spans consumed"""
    ops = U.expand_runs(runs)
    qi = np.cumsum(ops != U.OP_D) - 1
    ti = np.cumsum(ops != U.OP_I) - 1
    eq, x = ops == U.OP_EQ, ops == U.OP_X
    assert (q[qi[eq]] == t[ti[eq]]).all() and (q[qi[x]] != t[ti[x]]).all()
    assert int((ops != U.OP_D).sum()) == len(q) and int((ops != U.OP_I).sum()) == len(t)
    return int((ops != U.OP_EQ).sum())


def diagonals(runs):
    """(min, max) of row - column over the cells the path visits, the origin included"""
    ops = U.expand_runs(runs).astype(np.int64)
    off = np.concatenate(([0], np.cumsum((ops == U.OP_D).astype(np.int64) - (ops == U.OP_I))))
    return int(off.min()), int(off.max())


# ---- prediction ----------------------------------------------------------------------------------------------------------
def threshold(rate, n, m):
    return min(max(int(rate * max(n, m)) + 16, abs(n - m), 16), n + m)


@functools.lru_cache(None)
def plan_of(n, m, k, stripe_lanes, budget):
    return P.plan(n, m, k, stripe_lanes, budget)


def attempts(n, m, dist, rate, stripe_lanes=ALL_LANES, budget=NO_BUDGET):
    """[(R, G, S, k, kcap)] of every attempt of a job, the last one holds the distance; None at the end: refused there"""
    out, k = [], threshold(rate, n, m)
    while True:
        p = P.plan(n, m, k, stripe_lanes, budget)
        out.append(p)
        if p is None or dist <= p[3]:
            return out
        assert p[3] < n + m
        k = 2 * p[3]


def predict(jobs, rate, stripe_lanes=ALL_LANES, budget=None, ops=False):
    """jobs: [(n, m, distance)].  The call's final plans [(k, kcap, R, G, S) or None: not aligned], its six counters and
    its launches {"nw_forward", "nw_traceback"}.  budget None: the default budget (a share of the free memory), under which
    every pass of a small batch is one chunk; a number: engine option nw_budget_mb in bytes — the passes are cut by the
    restatement of nw_chunks, and what the early retry's one chunk does not hold is doubled once more by the pass behind
    it."""
    plan_budget = NO_BUDGET if budget is None else budget
    st = dict(n_aligned=0, n_retries=0, n_unaligned=0, n_batches=0, band_cells=0, store_bytes=0)
    launches = dict(nw_forward=0, nw_traceback=0)
    plan, final = {}, [None] * len(jobs)

    def replan(i, k):
        n, m, _ = jobs[i]
        p = plan_of(n, m, k, stripe_lanes, plan_budget)
        if p is not None:
            plan[i] = p
        return p is not None

    def sweep_and_walk(todo, layout=P.OWN_FIRST):
        """one pass: counters, launches; (the jobs beyond their thresholds in pass order, the jobs handed back)"""
        if not todo:
            return [], []
        order = sorted(todo, key=lambda i: tuple(-v for v in P.order_key(jobs[i][:2] + (plan[i][3],) + plan[i][:3])))
        bounds, left = [(0, len(order))], []
        if budget is not None:
            lines, _ = P.chunks([jobs[i][:2] + (plan[i][3],) + plan[i][:3] for i in order], budget, layout, 1)
            bounds = [tuple(int(v) for v in ln.split()[1:3]) for ln in lines if ln.startswith("chunk ")]
            left = [order[int(x)] for ln in lines if ln.startswith("left") for x in ln.split()[1:]]
        for c0, c1 in bounds:
            stored, stripes, classes = 0, 0, set()
            for i in order[c0:c1]:
                n, m, _ = jobs[i]
                R, G, S, k, _ = plan[i]
                lo, hi = P.band(n, m, k)
                st["band_cells"] += m * (lo + hi + 1)
                hs, ck = P.store(n, m, k, R, S)
                stored += hs * 4 + ck * 16
                if S:
                    stripes = max(stripes, P.n_stripes_of(n, R, S))
                else:
                    classes.add((R, G))
            st["store_bytes"] = max(st["store_bytes"], stored)
            st["n_batches"] += 1
            launches["nw_forward"] += len(classes) + stripes  # one per non-empty class, one per stripe
            launches["nw_traceback"] += 1                       # one walk per chunk
        handed_back = set(left)
        return [i for i in order if i not in handed_back and jobs[i][2] > plan[i][3]], left

    def settle(todo, beyond):
        for i in todo:
            if i not in beyond:
                st["n_aligned"] += 1
                final[i] = (plan[i][3], plan[i][4]) + plan[i][:3]

    first = []
    for i, (n, m, _) in enumerate(jobs):
        if n == 0 or m == 0 or not replan(i, threshold(rate, n, m)):
            st["n_unaligned"] += 1
        else:
            first.append(i)
    beyond, _ = sweep_and_walk(first)
    settle(first, set(beyond))
    early = []
    for i in beyond:  # the early retry: at most 4 096, a job that cannot be doubled stays where it is
        if len(early) >= HEAD_MAX:
            break
        if replan(i, 2 * plan[i][3]):
            early.append(i)
    beyond_early, left = sweep_and_walk(early, P.HEAD_ONLY)
    early = set(early) - set(left)  # (beyond the set's share: doubled, not swept; the next pass doubles again)
    st["n_retries"] += len(early)
    settle(early, set(beyond_early))
    again = [i for i in beyond if i not in early] + beyond_early
    while again:
        todo = []
        for i in sorted(again):
            st["n_retries"] += 1
            if replan(i, 2 * plan[i][3]):
                todo.append(i)
            else:
                st["n_unaligned"] += 1
        again, _ = sweep_and_walk(todo)
        settle(todo, set(again))
    # the path form: count, pack and — where the ops are asked for and there are any — expand
    any_ops = any(f is not None for f in final) or any((n == 0) != (m == 0) for n, m, _ in jobs)
    launches["nw_traceback"] += 2 + (1 if ops and any_ops else 0)
    return final, st, launches


def expected(cases):
    """the result of a batch from the references: (distances, run offsets, runs, op offsets, ops)"""
    refs = [reference(c) for c in cases]
    dist = np.array([d for d, _ in refs], dtype=np.uint32)
    runs = np.concatenate([np.zeros(0, np.uint32)] + [r for _, r in refs]).astype(np.uint32)
    off = np.concatenate(([0], np.cumsum([len(r) for _, r in refs]))).astype(np.uint64)
    op_off = np.concatenate(([0], np.cumsum([int((r >> 2).sum()) for _, r in refs]))).astype(np.uint64)
    return dist, off, runs, op_off, U.expand_runs(runs)


def compare(got, want, what=""):
    """Equality of a device result (distances, offsets, run words or op bytes) with the expected one, element for element;
    the message names the first pair that differs."""
    g_dist, g_off, g_words = got
    w_dist, w_off, w_words = want
    assert len(g_dist) == len(w_dist) and len(g_off) == len(w_off), what
    bad = np.flatnonzero(g_dist != w_dist)
    assert bad.size == 0, "%s: distance of pair %d: %d, reference %d" % (what, bad[0], g_dist[bad[0]], w_dist[bad[0]])
    bad = np.flatnonzero(g_off != w_off)
    assert bad.size == 0, "%s: offset %d: %d, reference %d" % (what, bad[0], g_off[bad[0]], w_off[bad[0]])
    assert len(g_words) == len(w_words), what
    bad = np.flatnonzero(g_words != w_words)
    if bad.size:
        p = int(np.searchsorted(w_off, bad[0], side="right")) - 1
        raise AssertionError("%s: word %d (pair %d): %#x, reference %#x" % (what, bad[0], p, g_words[bad[0]], w_words[bad[0]]))


def compare_counters(got_stats, got_launches, want_stats, want_launches, what=""):
    for name, v in want_stats.items():
        assert got_stats[name] == v, "%s: %s %d, predicted %d" % (what, name, got_stats[name], v)
    for name, v in want_launches.items():
        assert got_launches[name] == v, "%s: %s launches %d, predicted %d" % (what, name, got_launches[name], v)


def compare_plans(got_plans, want_plans, what=""):
    assert len(got_plans) == len(want_plans), what
    for p, (g, w) in enumerate(zip(got_plans, want_plans)):
        if w is not None:
            assert tuple(int(v) for v in g) == tuple(w), "%s: plan of pair %d: %r, predicted %r" % (what, p, tuple(g), w)


def batch(cases, strands=(1, 0)):
    """(reads, pairs rows, cases in pair order): every case on the given strands (1: as is, 0: the query stored
    reverse-complemented), spans in the middle of their reads with pads of different lengths"""
    rng = np.random.default_rng(len(cases))
    reads, rows, items = [], [], []
    for c in cases:
        for strand in strands:
            qa, qb = rnd(rng, int(rng.integers(0, 40))), rnd(rng, int(rng.integers(41, 90)))
            ta, tb = rnd(rng, int(rng.integers(0, 70))), rnd(rng, int(rng.integers(0, 30)))
            p = len(items)
            reads.append(np.concatenate((qa, c.q if strand else revcomp(c.q), qb)))
            reads.append(np.concatenate((ta, c.t, tb)))
            rows.append((2 * p, len(qa), c.m, 2 * p + 1, len(ta), c.n, strand, 0))
            items.append(c)
    return reads, rows, items


# ---- families ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def threshold_cases():
    """rate 0: k0 = max(16, |n - m|).  meta: dist, and `touch` = -1 / +1 where the path must run on diagonal -lo / +hi"""
    rng = np.random.default_rng(1601)
    out = []
    for dist, length in ((15, 120), (16, 160), (17, 200), (32, 240), (33, 280), (64, 340), (65, 400)):
        q, t = mismatches_at(rng, length, spread(length, dist))
        out.append(Case("thr_mismatch_%d" % dist, q, t, dist=dist))
    t = rnd(rng, 200)
    out.append(Case("thr_on_minus_lo", np.concatenate((3 - t[:8], t[:-8])), t, dist=16, touch=-1))
    out.append(Case("thr_on_plus_hi", np.concatenate((t[8:], 3 - t[-8:])), t, dist=16, touch=+1))
    t = rnd(rng, 216)
    out.append(Case("thr_rows_16_more", np.concatenate((t[:90], t[106:])), t, dist=16, touch=+1))   # k == d: lo = 0
    out.append(Case("thr_cols_16_more", t, np.concatenate((t[:90], t[106:])), dist=16, touch=-1))   # k == d: hi = 0
    t = rnd(rng, 300)
    out.append(Case("thr_rows_40_more", np.concatenate((t[:100], t[140:])), t, dist=40, touch=+1))  # k0 = d = 40
    out.append(Case("thr_all_mismatch_200", rnd(rng, 200, 2) + 2, rnd(rng, 200, 2), dist=200))     # 16 -> ... -> 256
    return tuple(out)


def _sizes_of_variant(lvl, d):
    """(smallest, largest) n + m of pairs with n - m = d whose threshold n + m takes variant lvl"""
    R, G = P.VARIANTS[lvl]
    sums = []
    for edge in ("low", "high"):
        if edge == "low":
            s = 2 + abs(d) if lvl == 0 else P.largest_threshold(*_split(1 << 20, d), *P.VARIANTS[lvl - 1]) + 1
            step = 1
        else:
            s = P.largest_threshold(*_split(1 << 20, d), R, G)
            step = -1
        while (s - d) % 2 or min(_split(s, d)) < 1 or P.plan(*_split(s, d), s, ALL_LANES, NO_BUDGET)[:2] != (R, G):
            s += step
        sums.append(s)
    return tuple(sums)


def _split(s, d):
    return (s + d) // 2, (s - d) // 2  # (n, m) with n + m = s, n - m = d


NO_DP_CASES = ("ring_8x64_high_d0", "ring_8x64_high_d37", "ring_8x64_high_d-37", "below_8x64_at_kcap")


@functools.lru_cache(None)
def ring_edge_cases():
    """large rate, k = n + m: per variant the smallest and the largest n + m it takes, with n = m, n > m, n < m.
    meta: variant (R, G), lanes of the ring, rate"""
    rng = np.random.default_rng(6401)
    out = []
    for lvl, (R, G) in enumerate(P.VARIANTS):
        for d in (0, 37, -37):
            low, high = _sizes_of_variant(lvl, d)
            for edge, s in (("low", low), ("high", high)):
                n, m = _split(s, d)
                q, t = related(rng, n, m)
                lanes = P.ring_lanes(*P.band(n, m, s), R)
                out.append(Case("ring_%dx%d_%s_d%d" % (R, G, edge, d), q, t, variant=(R, G), lanes=lanes, edge=edge,
                                rate=RATE_LARGE, level=lvl))
    return tuple(out)


@functools.lru_cache(None)
def ring_below_cases():
    """the same boundaries from below: a related pair with a few edits and a rate r with floor(r * len) + 16 = kcap (the
    ring full, the band narrow) and kcap + 1 (the next variant).  One case per (variant, side): meta rate, variant."""
    rng = np.random.default_rng(6402)
    out = []
    for lvl, (R, G) in enumerate(P.VARIANTS):
        kcap = P.largest_threshold(1 << 20, 1 << 20, R, G)
        length = (kcap + 1) // 2 + 40  # n = m = length: n + m > kcap + 1
        q0, t = related(rng, length, length)
        for k, tag in ((kcap, "at_kcap"), (kcap + 1, "above_kcap")):
            if lvl == len(P.VARIANTS) - 1 and tag == "above_kcap":
                continue  # (stripes of 64 lanes: not in this family)
            rate = next(r for r in ((k - 16 + f) / length for f in (0.5, 0.25, 0.75)) if int(r * length) + 16 == k)
            want = P.plan(length, length, k, ALL_LANES, NO_BUDGET)
            assert want[:2] == (P.VARIANTS[lvl] if tag == "at_kcap" else P.VARIANTS[lvl + 1]) and want[3] == k
            out.append(Case("below_%dx%d_%s" % (R, G, tag), q0, t, rate=rate, variant=want[:2], k=k, same_pair_as="below_%dx%d" % (R, G)))
    return tuple(out)


def _is_variant(n, m, R, G):
    p = P.plan(n, m, n + m, ALL_LANES, NO_BUDGET)
    return p is not None and p[:3] == (R, G, 0)


@functools.lru_cache(None)
def bundle_pool(G):
    """jobs of variant (1, G) under k = n + m, most different first: columns from 1 to the variant's largest, n_steps = m +
    ceil(n / 64) of every residue 0, 1, 15, 16, 17, 31 mod 32 (and so 32, 33), n = 1, m = 1, a homopolymer pair"""
    rng = np.random.default_rng(3200 + G)
    hi = P.largest_threshold(1 << 20, 1 << 20, 1, G) - 1
    sizes = []  # (n, m)
    m_max = max(m for m in range(1, hi) if _is_variant(1, m, 1, G))
    sizes.append((1, m_max))                                    # n = 1 < m, the most columns of the variant
    sizes.append((max(n for n in range(1, hi) if _is_variant(n, 1, 1, G)), 1))  # m = 1
    for res in (0, 1, 15, 16, 17, 31):
        for m0 in (hi // 2, hi // 5, 40):
            found = next(((n, m) for m in range(m0, m0 + 64) for n in (hi - m - 1, hi - m - 2)
                          if n >= 1 and _is_variant(n, m, 1, G) and (m + (n + 63) // 64) % 32 == res), None)
            if found and found not in sizes:
                sizes.append(found)
                break
    assert {(m + (n + 63) // 64) % 32 for n, m in sizes} >= {0, 1, 15, 16, 17, 31}, G
    if G == 4:
        sizes += [(1, 1), (1, 9), (7, 1)]
    while len(sizes) < 2 * (64 // G) + 1:
        m = int(rng.integers(2, hi - 2))
        n = hi - m - int(rng.integers(1, 3))
        if _is_variant(n, m, 1, G):
            sizes.append((n, m))
    out = []
    for x, (n, m) in enumerate(sizes):
        q, t = related(rng, n, m)
        if x == 2:  # a homopolymer pair: every cell a tie
            q, t = np.full(m, 2, np.uint8), np.full(n, 2, np.uint8)
        out.append(Case("bundle_G%d_%d_n%d_m%d" % (G, x, n, m), q, t, variant=(1, G), rate=RATE_LARGE))
    return tuple(out)


def bundle_batches(G):
    """[(name, cases)]: n_idx = 1, 64/G - 1, 64/G, 64/G + 1, 2 * 64/G + 1 jobs; the largest also reversed and shuffled"""
    pool, NG = bundle_pool(G), 64 // G
    out = []
    for n_idx in sorted({1, NG - 1, NG, NG + 1, 2 * NG + 1} - {0}):
        out.append(("G%d_n%d" % (G, n_idx), pool[:n_idx]))
    full = pool[:2 * NG + 1]
    out.append(("G%d_reversed" % G, full[::-1]))
    perm = np.random.default_rng(G).permutation(len(full))
    out.append(("G%d_shuffled" % G, tuple(full[int(i)] for i in perm)))
    return out


def _indel_singles(rng, count):
    """count isolated edits, alternately one inserted and one deleted base, '=' at both ends: 2 * count + 1 runs"""
    gap = 9
    t = rnd(rng, gap * (count + 1) + count // 2 + 3)
    q, at = [], 0
    for e in range(count):
        q.append(t[at:at + gap])
        at += gap
        if e % 2 == 0:
            q.append(np.array([min(set(range(4)) - {int(t[at - 1]), int(t[at])})], np.uint8))  # unlike both neighbours
        else:
            at += 1  # t[at - 1] is deleted
    q.append(t[at:])
    return np.concatenate(q), t


@functools.lru_cache(None)
def slot_cases():
    """rate 0: paths that fill their slot of 2k + 2 words to the first word — k edits, each isolated, '=' at both ends:
    2k + 1 runs + the count word — for k = 16 and, after one repeat, 32; between ordinary pairs.  meta: runs"""
    rng = np.random.default_rng(3301)
    full = {}
    for k in (16, 32):
        q, t = mismatches_at(rng, 40 + 5 * k, spread(40 + 5 * k, k))
        full["x%d" % k] = Case("slot_mismatch_%d" % k, q, t, runs=2 * k + 1, dist=k)
        for seed in range(50):  # (isolated indels of a random sequence: the DP decides whether each stayed a single)
            q, t = _indel_singles(np.random.default_rng(3302 + 97 * seed + k), k)
            d, r = U.dp_runs(q, t)
            if d == k and len(r) == 2 * k + 1:
                break
        full["id%d" % k] = Case("slot_indel_%d" % k, q, t, runs=2 * k + 1, dist=k)
    ordinary = [Case("slot_ordinary_%d" % x, *related(rng, 150 + 30 * x, 150 + 29 * x)) for x in range(4)]
    return full, ordinary


def slot_batches():
    full, o = slot_cases()
    out = []
    for kind in ("x", "id"):
        f16, f32 = full[kind + "16"], full[kind + "32"]
        out.append((kind + "_three_in_a_row", (o[0], f16, f32, f16, o[1])))
        out.append((kind + "_first_and_last", (f32, o[2], o[3], f16)))
    return out


def _with_runs(rng, runs):
    """a pair of exactly `runs` runs (>= 1): '=' runs cut by isolated 'X', the first column an 'X' for an even count"""
    e = runs // 2
    length = 3 * e + 4
    if runs == 1:
        return mismatches_at(rng, length, [])
    if runs % 2:
        return mismatches_at(rng, length, spread(length, e))
    return mismatches_at(rng, length, spread(length, e, first=0))


@functools.lru_cache(None)
def path_kernel_cases():
    """rate 0.  Runs per pair 0, 1, 3, 63, 64, 65, 255, 256, 257, 513; one run of 70 000; 256 runs of one op then one of
    5 000; empty spans; meta: runs.  (The pair that is not aligned is made by the GPU test: it needs an engine option.)"""
    rng = np.random.default_rng(2560)
    out = [Case("path_empty_both", [], [], runs=0), Case("path_empty_query", [], rnd(rng, 40), runs=1),
           Case("path_empty_target", rnd(rng, 70), [], runs=1)]
    for runs in (1, 3, 63, 64, 65, 255, 256, 257, 513):
        q, t = _with_runs(rng, runs)
        out.append(Case("path_runs_%d" % runs, q, t, runs=runs))
    t = rnd(rng, 70_000)
    out.append(Case("path_one_run_70000", t.copy(), t, runs=1, identical=True))
    t = rnd(rng, 256 + 5000, 3)
    q = t.copy()
    q[1:256:2] = 3  # '=' X '=' X ... X: 256 runs of one op each, then 5 000 '='
    out.append(Case("path_256_singles_then_5000", q, t, runs=257))
    return tuple(out)


@functools.lru_cache(None)
def small_distinct(count=64, lo=24, hi=41, dist=None, seed=64):
    """`count` distinct pairs of lo .. hi - 1 bases; dist: exactly that distance (T against {A, C, G}: see mismatches_at)"""
    rng = np.random.default_rng(seed)
    out = []
    for x in range(count):
        n = int(rng.integers(lo, hi))
        if dist is None:
            q, t = related(rng, n, int(rng.integers(lo, hi)))
        else:
            q, t = mismatches_at(rng, n, rng.choice(n, size=dist, replace=False))
        out.append(Case("small_%d_%s_%d" % (seed, dist, x), q, t, dist=dist))
    return tuple(out)


@functools.lru_cache(None)
def rate_cases(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for x in range(count):
        n = int(rng.integers(200, 900))
        t = rnd(rng, n)
        out.append(Case("rate_%d_%d" % (seed, x), mutate(rng, t, 0.04, 0.03, 0.03), t))
    return tuple(out)


@functools.lru_cache(None)
def chunked_repeat_cases():
    """60 pairs of about 6 000 bases, a quarter of them edits, and a rate whose first threshold (about 1 000) none of them
    meets and whose double all do: under nw_budget_mb = 64 the doubled bands exceed the early retry's twelfth of the budget"""
    rng = np.random.default_rng(6000)
    out = []
    for x in range(60):
        t = rnd(rng, 5800 + 7 * x)
        out.append(Case("chunked_repeat_%d" % x, mutate(rng, t, 0.10, 0.08, 0.08), t, rate=0.164))
    return tuple(out)


def next_rate(cases, previous):
    """nw_next_rate: from the distances of a call that aligned every case"""
    if len(cases) < 32:
        return previous
    r = sorted(reference(c)[0] / max(c.n, c.m) for c in cases)
    return r[min(len(r) - 1, int(len(r) * 0.9))] * 1.05 + 0.002
