"""Crafted match lists for the chain stage of Map (raven_amd/csrc/chain.hip: chain_matches) and a second, plain-Python
statement of ram's MinimizerEngine::Chain to hold the C++ oracle to on the same lists.

Encoding (ram's Match):  group = (rhs_id << 1 | strand) << 32 | diagonal,  positions = lhs_pos << 32 | rhs_pos.
Within one (rhs_id, strand) every position pair is distinct (real data has this property and chain_small_kernel's
insertion sort relies on it), and the order inside a read's segment is shuffled.

The interval families work in "forward space": arrays (lhs, r) in which a chain ascends in both.  place() turns r into
rhs positions (strand 1: rhs = r, strand 0: rhs = R0 - r, so the chain descends in rhs as ram's std::greater wants) and
gives every match of the interval a diagonal word inside one band, so that the band loop cuts exactly the intervals that
were built whatever the bandwidth.  (Nothing behind the group sort reads the diagonal of a group word; the `band` family
sets it on purpose.)
"""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
U = np.uint64

# The size classes of raven_amd/csrc/sizeclass.h, restated (kSegClassTable, kChainSmallCap, kChainClassTable;
# tests/test_size_class.py holds the two to each other): a read's group sort runs in LDS up to 4096 matches and
# as a wave sort beyond ("big"); an interval of <= 32 matches is chained by one lane, larger ones by one wave
# out of LDS up to 8192 matches and out of global scratch beyond ("global").
SEG_CLASS_CAPS = (256, 512, 1024, 2048, 4096)
CHAIN_SMALL_CAP = 32
CHAIN_CLASS_CAPS = (128, 256, 512, 768, 1024, 2048, 4096, 8192)

DEFAULT_PARAMS = (500, 4, 100, 10000)  # (bandwidth, chain, matches, gap) as in ram
PARAM_SETS = (DEFAULT_PARAMS, (0, 4, 100, 10000), (100, 1, 0, 50), (500, 2, 30, 200), (2000, 7, 100, 10000),
              (500, 40, 100, 10000))


# ---- ram's Chain, line by line, in plain Python -----------------------------------------------------------------------
def py_intervals(g, bandwidth):
    """ram Chain's first loop over the group words g (sorted; WITHOUT the stop dummy, which is appended here)."""
    g = list(g) + [0xFFFFFFFFFFFFFFFF]
    intervals = []
    j = 0
    for i in range(1, len(g)):
        if g[i] - g[j] > bandwidth:
            if i - j >= 4:
                if intervals and intervals[-1][1] > j:
                    intervals[-1][1] = i
                else:
                    intervals.append([j, i])
            j += 1
            while j < i and g[i] - g[j] > bandwidth:
                j += 1
    return intervals


def py_longest_subsequence(pos, strand):
    """ram LongestSubsequence on position words (already sorted): patience search with ram's exact lo / hi / mid."""
    n = len(pos)
    if n == 0:
        return []
    minimal = [0] * (n + 1)
    predecessor = [0] * n
    longest = 0
    lhs = [p >> 32 for p in pos]
    rhs = [p & M32 for p in pos]
    for it in range(n):
        lo, hi = 1, longest
        while lo <= hi:
            mid = lo + (hi - lo) // 2
            q = minimal[mid]
            if lhs[q] < lhs[it] and (rhs[q] < rhs[it] if strand else rhs[q] > rhs[it]):
                lo = mid + 1
            else:
                hi = mid - 1
        predecessor[it] = minimal[lo - 1]
        minimal[lo] = it
        longest = max(longest, lo)
    dst = []
    j = minimal[longest]
    for _ in range(longest):
        dst.append(j)
        j = predecessor[j]
    dst.reverse()
    return dst


def py_chain(lhs_id, groups, positions, k=15, bandwidth=500, chain=4, matches=100, gap=10000, info=None):
    """ram MinimizerEngine::Chain: list of (lhs_id, lhs_begin, lhs_end, rhs_id, rhs_begin, rhs_end, score, strand).
    info (a dict) receives the by-products: "intervals" [(begin, end)] and "longest" [chain length per interval
    (None where the interval is shorter than `chain` and never reaches the LIS)]."""
    k = min(max(int(k), 1), 31)
    order = sorted(range(len(groups)), key=lambda x: int(groups[x]))  # (stable, as ram's radix sort)
    g = [int(groups[x]) for x in order]
    p = [int(positions[x]) for x in order]
    intervals = py_intervals(g, bandwidth)
    g.append(0xFFFFFFFFFFFFFFFF)
    p.append(0xFFFFFFFFFFFFFFFF)  # stop dummy
    if info is not None:
        info["intervals"] = [tuple(x) for x in intervals]
        info["longest"] = []
    dst = []
    for j, i in intervals:
        if i - j < chain:
            if info is not None:
                info["longest"].append(None)
            continue
        p[j:i] = sorted(p[j:i])
        strand = (g[j] >> 32) & 1
        indices = py_longest_subsequence(p[j:i], strand)
        if info is not None:
            info["longest"].append(len(indices))
        if len(indices) < chain:
            continue
        indices.append(len(p) - 1 - j)
        l = 0
        for kk in range(1, len(indices)):
            if (((p[j + indices[kk]] >> 32) - (p[j + indices[kk - 1]] >> 32)) & M32) > gap:
                if kk - l < chain:
                    l = kk
                    continue
                lhs_matches = lhs_begin = lhs_end = 0
                rhs_matches = rhs_begin = rhs_end = 0
                for m in range(l, kk):
                    lhs_pos = p[j + indices[m]] >> 32
                    if lhs_pos > lhs_end:
                        lhs_matches = (lhs_matches + lhs_end - lhs_begin) & M32
                        lhs_begin = lhs_pos
                    lhs_end = (lhs_pos + k) & M32
                    rhs_pos = p[j + indices[m]] & M32
                    if not strand:
                        rhs_pos = ((1 << 31) - (rhs_pos + k - 1)) & M32
                    if rhs_pos > rhs_end:
                        rhs_matches = (rhs_matches + rhs_end - rhs_begin) & M32
                        rhs_begin = rhs_pos
                    rhs_end = (rhs_pos + k) & M32
                lhs_matches = (lhs_matches + lhs_end - lhs_begin) & M32
                rhs_matches = (rhs_matches + rhs_end - rhs_begin) & M32
                score = min(lhs_matches, rhs_matches)
                if score < matches:
                    l = kk
                    continue
                first, last = p[j + indices[l]], p[j + indices[kk - 1]]
                dst.append((int(lhs_id) & M32, first >> 32, (k + (last >> 32)) & M32, g[j] >> 33,
                            (first & M32) if strand else (last & M32),
                            (k + ((last & M32) if strand else (first & M32))) & M32, score, strand))
                l = kk
    return dst


def overlaps_as_tuples(ovl):
    """A structured overlap array (oracle / hip OVERLAP_DTYPE) as the tuples py_chain returns."""
    return [tuple(int(x) for x in o) for o in ovl.tolist()]


def longest_chain_n2(pos_sorted, strand):
    """Textbook O(n^2) length of the longest chain (lhs ascending and rhs ascending / descending, both strictly)."""
    lhs = [int(p) >> 32 for p in pos_sorted]
    rhs = [int(p) & M32 for p in pos_sorted]
    best = [1] * len(lhs)
    for i in range(len(lhs)):
        for j in range(i):
            if lhs[j] < lhs[i] and (rhs[j] < rhs[i] if strand else rhs[j] > rhs[i]) and best[j] + 1 > best[i]:
                best[i] = best[j] + 1
    return max(best) if best else 0


# ---- interval families (forward space: a chain ascends in lhs and in r) -------------------------------------------------
def _asc(rng, n, lo, hi):
    return np.cumsum(rng.integers(lo, hi + 1, size=n)).astype(np.int64)


def colinear(rng, n, k=15):
    """Both coordinates strictly ascending: the chain is the whole interval."""
    return _asc(rng, n, 1, 2 * k), _asc(rng, n, 1, 2 * k)


def ties(rng, n, k=15):
    """Tandem-repeat-like: a few distinct lhs values each met by many r values and the reverse, drawn without replacement
    from a grid of ~sqrt(2 n) x sqrt(2 n) cells.  ram's predicate is not monotone over the tails here."""
    side = max(2, int(np.ceil(np.sqrt(2.0 * n))))
    cells = rng.choice(side * side, size=n, replace=False)
    return (cells // side).astype(np.int64) * k + 1, (cells % side).astype(np.int64) * k + 1


def saw(rng, n, k=15):
    """lhs strictly ascending, r a rising sawtooth with teeth of 2 - 7 elements: a speculated colinear run turns every few
    elements, and elements alternately extend and do not extend the chain."""
    lhs = _asc(rng, n, 1, k)
    r = np.zeros(n, dtype=np.int64)
    i, floor = 0, 0
    while i < n:
        t = int(rng.integers(2, 8))
        m = min(t, n - i)
        r[i:i + m] = floor + np.arange(m) * 5
        floor += int(rng.integers(3, 12))  # the next tooth starts inside this one's span: some of it extends, some does not
        i += m
    # distinct pairs: lhs is strictly ascending already
    return lhs, r + 1


def anti(rng, n, k=15):
    """lhs ascending, r strictly descending: no two matches chain, the longest chain is 1."""
    return _asc(rng, n, 1, k), (np.cumsum(rng.integers(1, k + 1, size=n))[::-1]).astype(np.int64)


def prefix(rng, n, L, k=15, tail="anti"):
    """A colinear prefix of L matches, then n - L matches of larger lhs:
       tail="anti": r strictly descending inside the prefix's r range — each one replaces a tail somewhere below, none can
                    follow the prefix's last element or an earlier tail match, so the chain length stays exactly L;
       tail="saw" / "ties": that family behind (lhs) and across (r) the prefix's upper end — the chain grows from L on,
                    with the search at work at lengths around L."""
    assert 2 <= L <= n
    m = n - L
    scale = max(4, -(-(m + 2) // (2 * L)) + 1)  # the prefix's r range has room for m distinct values below its end
    lhs, r = _asc(rng, L, 1, k), _asc(rng, L, 2, k) * scale
    if m == 0:
        return lhs, r
    if tail == "anti":
        tr = np.sort(rng.choice(np.arange(1, int(r[-1])), size=m, replace=False))[::-1]
        tl = lhs[-1] + _asc(rng, m, 1, k)
    else:
        tl, tr = (saw if tail == "saw" else ties)(rng, m, k)
        tl = tl + lhs[-1]
        tr = tr + int(r[max(0, L - 1 - min(L - 1, 8))])  # starts a few elements below the prefix's end
    return np.concatenate([lhs, tl]), np.concatenate([r, tr.astype(np.int64)])


def steps(rng, n, k=15):
    """Colinear with spacings of exactly k - 1, k and k + 1 on both sides, mixed: the covered-bases score at its kink."""
    d = np.array([max(1, k - 1), k, k + 1])
    return np.cumsum(d[rng.integers(0, 3, size=n)]).astype(np.int64), np.cumsum(d[rng.integers(0, 3, size=n)]).astype(np.int64)


def gaps(rng, n, k=15, chain=4, matches=100, gap=10000):
    """Colinear pieces separated by lhs differences of exactly gap (no split) and gap + 1 (split): pieces one shorter than
    `chain`, of `chain` and longer ones, and — where a piece of unit spacing can score it — pieces whose covered bases
    are exactly `matches` and `matches` - 1.  About n matches (the last piece is cut to fit)."""
    lens = []
    if matches > k and matches - k + 1 >= chain:
        lens += [("unit", matches - k + 1), ("unit", matches - k), ("unit2", matches - k + 1), ("unit2", matches - k)]
    lens += [("k", max(1, chain - 1)), ("k", chain), ("k", chain + 1), ("k", max(chain, -(-matches // k))),
             ("k", max(chain, -(-matches // k)) + 1), ("k", max(chain, -(-matches // k) - 1))]
    lhs, r = [], []
    x = y = 1
    at = 0
    while len(lhs) < n:
        kind, m = lens[at % len(lens)] if at < 2 * len(lens) else ("k", int(rng.integers(1, 3 * max(chain, 4))))
        m = min(m, n - len(lhs))
        for e in range(m):
            lhs.append(x)
            r.append(y)
            if e + 1 < m:
                x += 1 if kind == "unit" else 2 if kind == "unit2" else int(rng.integers(1, min(gap, 2 * k) + 1))
                y += 1 if kind in ("unit", "unit2") else int(rng.integers(1, 2 * k + 1))
        # every third joint does not split (a difference of exactly gap), the others do (gap + 1)
        x += gap if at % 3 == 2 else gap + 1
        y += int(rng.integers(1, 2 * k + 1))
        at += 1
    return np.array(lhs, dtype=np.int64), np.array(r, dtype=np.int64)


def slots(rng, n, chain=4, gap=50, k=15):
    """Every `chain` consecutive matches form one piece (unit spacing inside, gap + 1 between): with matches <= k an
    interval of n matches emits floor(n / chain) overlaps, the capacity of its slot region."""
    i = np.arange(n, dtype=np.int64)
    lhs = (i // chain) * (gap + chain) + (i % chain) + 1
    return lhs, i * 2 + 1


def late(rng, n, k=15):
    """Colinear, but the match of the lowest lhs lies above every other r: the chain starts at the SECOND sorted element,
    whose predecessor word is ram's minimal[0] == 0 — an index that is not part of the chain (the backtrack must stop
    after `longest` elements and not follow it)."""
    lhs, r = colinear(rng, n, k)
    r = r.copy()
    r[0] = r[-1] + 1 + int(rng.integers(0, k))
    return lhs, r


FAMILIES = ("colinear", "ties", "saw", "anti", "prefix", "steps", "gaps", "slots", "late")


def family(name, rng, n, k=15, params=DEFAULT_PARAMS, L=None, tail="anti"):
    bandwidth, chain, matches, gap = params
    if name == "colinear":
        return colinear(rng, n, k)
    if name == "ties":
        return ties(rng, n, k)
    if name == "saw":
        return saw(rng, n, k)
    if name == "anti":
        return anti(rng, n, k)
    if name == "prefix":
        return prefix(rng, n, max(1, n // 2) if L is None else L, k, tail)
    if name == "steps":
        return steps(rng, n, k)
    if name == "gaps":
        return gaps(rng, n, k, chain, matches, gap)
    if name == "slots":
        return slots(rng, n, chain, gap, k)
    if name == "late":
        return late(rng, n, k)
    raise ValueError(name)


def place(rng, lhs, r, strand, rhs_id, bandwidth, diag0=None, shift=0):
    """(group words, position words) of one interval: strand 0 mirrors r, every diagonal word lies in
    [diag0, diag0 + bandwidth] (so the interval is one band of the band loop and nothing else joins it)."""
    lhs = np.asarray(lhs, dtype=np.int64) + shift  # (shift: intervals that share an rhs id and strand stay distinct)
    r = np.asarray(r, dtype=np.int64)
    rhs = r if strand else (int(r.max()) + 1 - r)
    assert lhs.min() >= 0 and rhs.min() >= 0 and lhs.max() < (1 << 30) and rhs.max() < (1 << 30)
    if diag0 is None:
        diag0 = int(rng.integers(1 << 20, 1 << 31))
    diag = diag0 + rng.integers(0, bandwidth + 1, size=lhs.shape[0])
    if lhs.shape[0]:
        diag[0], diag[-1] = diag0, diag0 + bandwidth  # the band is used to its full width
    grp = (U((int(rhs_id) << 1) | int(strand)) << U(32)) | diag.astype(np.uint64)
    return grp, (lhs.astype(np.uint64) << U(32)) | rhs.astype(np.uint64)


def band(rng, strand, rhs_id0, k=15, params=DEFAULT_PARAMS):
    """Crafted diagonals, one scenario per rhs id from rhs_id0 on; positions are colinear in diagonal order with a spacing
    of k, and the scenarios are long enough to score `matches` where that is possible at all.  Returns (grp, pos, number
    of rhs ids used).
      0  two blocks whose diagonals differ by exactly bandwidth: one interval
      1  ... by bandwidth + 1: two intervals that abut (the extend rule must NOT join them)
      2  a window of exactly 4 (one match, then three a diagonal further) whose successor window overlaps it: the extend
         rule makes one interval that starts at that first match
      3  windows of 3: no interval at all; 4: a window of exactly 4 on its own
      5  a diagonal drifting by bandwidth / 5 (at least 1) every four matches: one interval far wider than the band
         (bandwidth 0: every four matches their own interval)"""
    bandwidth, chain, matches, gap = params
    m = max(chain, -(-matches // k), 4) + 2
    out_g, out_p = [], []

    def emit(rhs_id, diags):
        n = len(diags)
        lhs = 1 + np.arange(n, dtype=np.int64) * k
        r = 7 + np.arange(n, dtype=np.int64) * k
        rhs = r if strand else (int(r.max()) + 1 - r)
        out_g.append((U((int(rhs_id) << 1) | int(strand)) << U(32)) | np.asarray(diags, dtype=np.uint64))
        out_p.append((lhs.astype(np.uint64) << U(32)) | rhs.astype(np.uint64))

    d = 1 << 24
    emit(rhs_id0 + 0, [d] * m + [d + bandwidth] * m)
    emit(rhs_id0 + 1, [d] * m + [d + bandwidth + 1] * m)
    emit(rhs_id0 + 2, [d] + [d + 1] * 3 + [d + bandwidth + 1] * m + [d + 2 * bandwidth + 3] * m)
    emit(rhs_id0 + 3, [d] * 3 + [d + bandwidth + 1] * 3 + [d + 2 * bandwidth + 2] * 3)
    emit(rhs_id0 + 4, [d] * 4)
    step = max(1, bandwidth // 5)
    emit(rhs_id0 + 5, [d + step * (i // 4) for i in range(max(400, 4 * m))])
    return np.concatenate(out_g), np.concatenate(out_p), 6


# ---- read-level assembly ---------------------------------------------------------------------------------------------
class Batch:
    """Reads of crafted matches: per read a list of (grp, pos) blocks, shuffled inside the read's segment on build()."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.reads = []      # per read: list of (grp, pos)
        self.next_rhs = 11   # rhs ids are handed out in ascending order, one per interval unless the caller says otherwise

    def rhs_id(self):
        self.next_rhs += int(self.rng.integers(1, 1000))
        return self.next_rhs

    def interval(self, name, n, strand, k=15, params=DEFAULT_PARAMS, rhs_id=None, diag0=None, shift=0, **kw):
        lhs, r = family(name, self.rng, n, k, params, **kw)
        return place(self.rng, lhs, r, strand, self.rhs_id() if rhs_id is None else rhs_id, params[0], diag0, shift)

    def loose(self, n):
        """n <= 3 matches on an rhs id of their own: never an interval."""
        assert n <= 3
        rid = self.rhs_id()
        lhs = self.rng.choice(100000, size=n, replace=False).astype(np.uint64)
        grp = (U(rid << 1 | 1) << U(32)) | (U(3 << 30) + lhs)
        return grp, (lhs << U(32)) | (lhs + U(5))

    def add_read(self, blocks):
        self.reads.append(list(blocks))
        return len(self.reads) - 1

    def build(self, shuffle_seed=0):
        """(ids uint32[n], grp uint64[H], pos uint64[H], seg_off uint64[n + 1]); read ids are distinct and not indices."""
        rng = np.random.default_rng(shuffle_seed)
        n = len(self.reads)
        ids = (1000 + 7 * np.arange(n)).astype(np.uint32)
        if n:
            ids[-1] = (1 << 30) - 1  # the largest read id the device takes
        seg = np.zeros(n + 1, dtype=np.uint64)
        gs, ps = [], []
        for i, blocks in enumerate(self.reads):
            g = np.concatenate([b[0] for b in blocks]) if blocks else np.zeros(0, np.uint64)
            p = np.concatenate([b[1] for b in blocks]) if blocks else np.zeros(0, np.uint64)
            perm = rng.permutation(g.shape[0])
            gs.append(g[perm])
            ps.append(p[perm])
            seg[i + 1] = seg[i] + U(g.shape[0])
        grp = np.concatenate(gs) if gs else np.zeros(0, np.uint64)
        pos = np.concatenate(ps) if ps else np.zeros(0, np.uint64)
        return ids, grp.astype(np.uint64), pos.astype(np.uint64), seg


def read_of_total(b: Batch, total, name, strand, k=15, params=DEFAULT_PARAMS):
    """Blocks of one read of exactly `total` matches: one interval of the family, one of four matches, three loose ones."""
    assert total >= 16
    return [b.interval(name, total - 7, strand, k, params), b.interval("colinear", 4, 1 - strand, k, params), b.loose(3)]


def class_batch(seed=1, k=15, params=DEFAULT_PARAMS):
    """One batch that reaches every size class of the chain stage: intervals of cap - 1 / cap / cap + 1 for the small
    kernel and every LDS class, one of ~20 000 and one above 65 536 matches (global path, beyond u16 indices), reads whose
    totals sit at cap - 1 / cap / cap + 1 of every group-sort class, reads of 0, 1 and 3 matches first, last and in
    between, a read above 4096 matches made of many small intervals, both strands and several rhs ids in one read, an rhs
    id next to 2^31 - 1.  Returns (Batch, wanted): wanted = {"intervals": sizes that must occur, "totals": read totals}."""
    b = Batch(seed)
    names = ("colinear", "saw", "ties", "steps")
    want_iv, want_tot = [], []
    b.add_read([])                       # an empty read first
    at = 0
    for cap in (CHAIN_SMALL_CAP,) + CHAIN_CLASS_CAPS:
        blocks = []
        for n in (cap - 1, cap, cap + 1):
            blocks.append(b.interval(names[at % 4], n, at & 1, k, params))
            want_iv.append(n)
            at += 1
        b.add_read(blocks)
        if cap == 512:
            b.add_read([b.loose(1)])     # one match, in between
    b.add_read([b.loose(3)])
    for n, name in ((20000, "saw"), (65536 + 700, "colinear")):
        b.add_read([b.interval(name, n, at & 1, k, params), b.loose(2)])
        want_iv.append(n)
        at += 1
    for cap in SEG_CLASS_CAPS:
        for t in (cap - 1, cap, cap + 1):
            b.add_read(read_of_total(b, t, names[at % 4], at & 1, k, params))
            want_tot.append(t)
            want_iv.append(t - 7)
            at += 1
    # above the largest group-sort class, made of many small intervals (both strands of the same rhs ids)
    blocks = []
    for i in range(300):
        rid = b.rhs_id()
        for strand in (1, 0):
            blocks.append(b.interval(names[i % 4], int(b.rng.integers(4, 13)), strand, k, params, rhs_id=rid))
    blocks.append(b.interval("colinear", 40, 1, k, params, rhs_id=(1 << 31) - 1))
    blocks.append(b.interval("colinear", 9, 0, k, params, rhs_id=(1 << 31) - 2))
    b.add_read(blocks)
    want_tot.append(sum(x[0].shape[0] for x in blocks))
    b.add_read([b.loose(3)])
    b.add_read([])                       # ... and an empty read last
    return b, {"intervals": want_iv, "totals": want_tot}


REGIME_LENGTHS = (63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 5000)


def regime_batch(seed=2, k=15, params=DEFAULT_PARAMS, flip=0):
    """The search regimes of chain_wave — ballot masks up to 64 and up to 512, the six-level tree above (4097 and 5000:
    three rounds), speculated runs and the all-probes-precede fast path throughout — each met by a colinear prefix of L
    followed by descending noise (the chain stays L), a sawtooth and a tie grid (the chain grows from L), in an LDS-class
    interval and, for some, on the global path (more than 8192 matches); interval sizes n = 0, 1 and 63 mod 64.  Returns
    (Batch, [(read, L, tail, n)] of the tail="anti" intervals whose chain length must be exactly L)."""
    b = Batch(seed)
    exact = []
    at = flip
    mods = (0, 1, 63)
    for L in REGIME_LENGTHS:
        blocks = []
        for tail in ("anti", "saw", "ties"):
            n = ((L + 150 + 63) // 64) * 64 + mods[at % 3]
            blocks.append(b.interval("prefix", n, at & 1, k, params, L=L, tail=tail))
            if tail == "anti":
                exact.append((len(b.reads), L, tail, n))
            at += 1
        b.add_read(blocks)
    for i, L in enumerate((64, 65, 512, 513, 4096, 4097, 5000)):
        tail = ("anti", "saw", "ties")[i % 3]
        n = 8192 + 64 * (1 + i) + mods[i % 3]
        r = b.add_read([b.interval("prefix", n, at & 1, k, params, L=L, tail=tail), b.loose(i % 4)])
        if tail == "anti":
            exact.append((r, L, tail, n))
        at += 1
    # the families on their own around the regime boundaries, and an anti interval (chain length 1) in every path
    blocks = []
    for name in ("ties", "saw", "anti", "colinear", "late"):
        for n in (33, 64, 65, 127, 129, 577, 1025):
            blocks.append(b.interval(name, n, at & 1, k, params))
            at += 1
    b.add_read(blocks)
    b.add_read([b.interval("anti", 8192 + 65, at & 1, k, params), b.interval("ties", 8192 + 127, 1 - (at & 1), k, params)])
    return b, exact


def mixed_batch(seed, k, params):
    """Every family at small sizes (small kernel, first LDS classes) plus the `band` scenarios on both strands, built for
    one (k, bandwidth, chain, matches, gap): what a non-default engine is held to."""
    b = Batch(seed)
    bandwidth, chain, matches, gap = params
    at = 0
    b.add_read([b.loose(3)])
    for name in FAMILIES:
        blocks = []
        for n in (4, 5, 17, 31, 32, 33, 41, 64, 65, 130, 300):
            if name == "ties" and n < 8:
                continue
            blocks.append(b.interval(name, n, at & 1, k, params))
            at += 1
        b.add_read(blocks)
    for name in ("steps", "gaps", "gaps"):
        b.add_read([b.interval(name, 1100 + at, strand, k, params) for strand in (1, 0)])
        at += 1
    b.add_read([])
    for strand in (1, 0):
        rid = b.rhs_id()
        g, p, used = band(b.rng, strand, rid, k, params)
        b.next_rhs = rid + used
        b.add_read([(g, p), b.loose(2)])
    return b


def slots_batch(seed, chain, k=15, gap=50, bandwidth=100):
    """`slots` intervals for an engine (bandwidth, chain, 0, gap): in the small kernel (n <= 32), in LDS classes and on the
    global path, two of each back to back in one read (an overrun of one interval's slot region lands in its neighbour's),
    reads back to back as well.  Returns (Batch, [(read, n)]): each listed interval emits floor(n / chain) overlaps."""
    b = Batch(seed)
    params = (bandwidth, chain, 0, gap)
    listed = []
    at = 0
    for sizes in ((4, 8, 12, 29, 32, 32, 31, 30), (36, 64, 33, 40, 44, 128), (516, 4096, 4096), (8200, 8196)):
        blocks = []
        rid = b.rhs_id()
        for i, n in enumerate(sizes):
            # the same rhs id and strand, ascending diagonals: the intervals are neighbours in the sorted segment
            blocks.append(b.interval("slots", n, at & 1, k, params, rhs_id=rid, diag0=(1 << 22) + i * (2 * bandwidth + 7),
                                     shift=i * (1 << 25)))
            listed.append((len(b.reads), n))
        b.add_read(blocks)
        at += 1
    return b, listed


def above_small_batch(seed, chain, k=15, gap=50, bandwidth=100):
    """For an engine (bandwidth, chain, 0, gap) with chain above the small kernel's 32: intervals below 32 (the small
    kernel skips them: shorter than `chain`), between 32 and `chain` (no kernel takes them), of exactly `chain` and above."""
    b = Batch(seed)
    params = (bandwidth, chain, 0, gap)
    at = 0
    for name in ("slots", "colinear", "saw", "late"):
        blocks = []
        for n in (4, 20, 32, 33, chain - 1, chain, chain + 1, 2 * chain - 1, 2 * chain, 129, 300):
            blocks.append(b.interval(name, n, at & 1, k, params))
            at += 1
        b.add_read(blocks)
    return b
