"""The merge stage of a flush of FindOverlapsAndCreatePiles (raven_amd/csrc/pile.hip: rhs_keys_kernel and the sort by rhs,
pile_counts_kernel, pile_build_kernel, add_layers_kernel, truncate_sort_kernel, kept_write_kernel, and the kept lists
carried from one flush to the next) on crafted overlap lists: a plain reference of the stage and the cases.

MergeRef is construct.cc:72-107 written out in Python, single-threaded, on lists of tuples: append every overlap to its
lhs pile and its reversal to its rhs pile in the given (query, emission) order; then, for every pile that grew, AddLayers
of the new entries only (add_layers: pile.cc:33-62 as the sweep it is, uint32 wrap-around included), counted =
min(size, kmax), and at size >= kmax the oracle's own std::sort by GetOverlapLength (oracle.truncate: libstdc++'s
unstable permutation is part of the result) and the cut to kmax.  tests/test_merge_cases.py holds it to the oracle's
whole pass on the lambda reads.

cases() returns a list of dicts:
  name      the case; one case is one pass of one or several flushes
  family    one of FAMILIES, named after what the case places
  lengths   uint32[n]: the reads' lengths (a pile has len >> 4 cells; pile ids are read indices)
  kmax
  flushes   one OVERLAP_DTYPE array per flush, grouped by ascending lhs_id, lhs_id < rhs_id
  claims    what the case holds BY CONSTRUCTION (sizes, cells, values); test_merge_cases.py asserts each of the
            reference's output, test_gpu_merge.py runs the cases on the device
Every generator keeps to input the reference defines (assert_defined).  Nothing here looks at what the code under test
returns."""
import functools

import numpy as np

from oracle import oracle

DT = oracle.OVERLAP_DTYPE
FAMILIES = ("order", "piles", "kmax", "sort", "tiles")
TILE = 8192  # cells of one tile of add_layers_kernel
PSS = 4      # pile.h:21


# ---- the reference ---------------------------------------------------------------------------------------------------

def reverse(o):
    """OverlapReverse (overlap_utils.cc:5-8): the two sides change places, score and strand stay."""
    return (o[3], o[4], o[5], o[0], o[1], o[2], o[6], o[7])


def overlap_length(o):
    """GetOverlapLength (overlap_utils.cc:10-12)."""
    return max(o[5] - o[4], o[2] - o[1])


def add_layers(data, pile_id, entries):
    """Pile::AddLayers (pile.cc:33-62) of `entries` (tuples) on the uint16 cells `data`, in place: the events are kept as
    (cell << 1 | is_end) in 32 bits and sorted, `coverage` is a uint32 that may wrap below 0, and a stretch of cells gets
    clamp(data + coverage) in uint32 arithmetic whenever coverage != 0 — once per cell per call.  Raises where pile.cc
    would write beyond the pile."""
    ev = []
    for o in entries:
        if o[0] == pile_id:
            b, e = o[1], o[2]
        elif o[3] == pile_id:
            b, e = o[4], o[5]
        else:
            continue
        ev.append((((b >> PSS) + 1) << 1) & 0xFFFFFFFF)
        ev.append(((((e >> PSS) - 1) << 1) | 1) & 0xFFFFFFFF)
    ev.sort()
    coverage, last = 0, 0
    for it in ev:
        x = it >> 1
        if coverage > 0 and x > last:
            if x > data.shape[0]:
                raise IndexError("pile %d: AddLayers writes cells [%d, %d) of %d" % (pile_id, last, x, data.shape[0]))
            s = data[last:x].astype(np.uint32) + np.uint32(coverage)  # (wraps like the reference's uint32 sum)
            data[last:x] = np.minimum(s, np.uint32(65535)).astype(np.uint16)
        last = x
        coverage = (coverage + (0xFFFFFFFF if it & 1 else 1)) & 0xFFFFFFFF


class MergeRef:
    """State of a pass between flushes: lists[p] (tuples), counted[p], coverage[p] (uint16[len >> 4])."""

    def __init__(self, lengths, kmax):
        self.lengths = np.asarray(lengths, dtype=np.uint32)
        self.n = int(self.lengths.shape[0])
        self.kmax = int(kmax)
        self.lists = [[] for _ in range(self.n)]
        self.counted = [0] * self.n
        self.coverage = [np.zeros(int(c), dtype=np.uint16) for c in (self.lengths >> PSS)]

    def flush(self, overlaps):
        """construct.cc:72-107 for the Map results of one flush window, in the order given."""
        grew = set()
        for o in np.asarray(overlaps, dtype=DT).tolist():
            self.lists[o[0]].append(o)
            self.lists[o[3]].append(reverse(o))
            grew.add(o[0])
            grew.add(o[3])
        for p in sorted(grew):
            lst = self.lists[p]
            add_layers(self.coverage[p], p, lst[self.counted[p]:])
            self.counted[p] = min(len(lst), self.kmax)
            if len(lst) < self.kmax:
                continue
            self.lists[p] = oracle.truncate(np.array(lst, dtype=DT), self.kmax).tolist()

    def piles(self):
        """(cells of all piles, uint64 offsets[n + 1]) — what Pass1.piles() returns."""
        off = np.zeros(self.n + 1, dtype=np.uint64)
        np.cumsum((self.lengths >> PSS).astype(np.uint64), out=off[1:])
        data = np.concatenate(self.coverage) if self.n else np.zeros(0, np.uint16)
        return data.astype(np.uint16), off

    def overlaps(self):
        """(lists of all piles, uint32 offsets[n + 1]) — what Pass1.overlaps() returns."""
        off = np.zeros(self.n + 1, dtype=np.uint32)
        np.cumsum(np.array([len(x) for x in self.lists], dtype=np.uint32), out=off[1:])
        flat = [t for lst in self.lists for t in lst]
        return (np.array(flat, dtype=DT) if flat else np.zeros(0, DT)), off

    def state(self):
        data, poff = self.piles()
        ovl, ooff = self.overlaps()
        return dict(data=data, pile_offsets=poff, overlaps=ovl, offsets=ooff)


def run(case):
    """The reference's state after every flush of the case."""
    ref = MergeRef(case["lengths"], case["kmax"])
    out = []
    for f in case["flushes"]:
        ref.flush(f)
        out.append(ref.state())
    return out


def flush_windows(lengths, flush_bases):
    """[first, last) read ranges of the flushes of one index batch (construct.cc:56-60: a window closes with the read
    that brings its bases to flush_bases, and with the last read)."""
    out, first, acc, n = [], 0, 0, len(lengths)
    for k in range(n):
        acc += int(lengths[k])
        if k != n - 1 and acc < flush_bases:
            continue
        acc = 0
        out.append((first, k + 1))
        first = k + 1
    return out


def diff_state(got, want):
    """None when two states (dicts of data, pile_offsets, overlaps, offsets) are the same integers in the same order,
    else a sentence about the first difference."""
    for key in ("pile_offsets", "offsets"):
        g, w = np.asarray(got[key]).astype(np.int64), np.asarray(want[key]).astype(np.int64)
        if g.shape != w.shape:
            return "%s: %d entries, expected %d" % (key, g.shape[0], w.shape[0])
        bad = np.flatnonzero(g != w)
        if bad.size:
            i = int(bad[0])
            return "%s[%d] = %d, expected %d (list or pile %d)" % (key, i, g[i], w[i], max(i - 1, 0))
    poff = np.asarray(want["pile_offsets"]).astype(np.int64)
    g, w = np.asarray(got["data"]), np.asarray(want["data"])
    if g.shape != w.shape:
        return "coverage: %d cells, expected %d" % (g.shape[0], w.shape[0])
    bad = np.flatnonzero(g != w)
    if bad.size:
        i = int(bad[0])
        p = int(np.searchsorted(poff, i, side="right")) - 1
        return "coverage of pile %d, cell %d (tile %d, cell %d of it) = %d, expected %d; %d cells differ" % (
            p, i - poff[p], (i - poff[p]) // TILE, (i - poff[p]) % TILE, g[i], w[i], bad.size)
    ooff = np.asarray(want["offsets"]).astype(np.int64)
    g, w = np.asarray(got["overlaps"]), np.asarray(want["overlaps"])
    if g.shape != w.shape:
        return "overlaps: %d entries, expected %d" % (g.shape[0], w.shape[0])
    bad = np.flatnonzero(g != w)
    if bad.size:
        i = int(bad[0])
        p = int(np.searchsorted(ooff, i, side="right")) - 1
        fields = [f for f in DT.names if g[i][f] != w[i][f]]
        return "list of pile %d, entry %d of %d: %s differ: %s, expected %s; %d entries differ" % (
            p, i - ooff[p], ooff[p + 1] - ooff[p], ", ".join(fields), g[i].tolist(), w[i].tolist(), bad.size)
    return None


# ---- helpers of the generators and of the tests ----------------------------------------------------------------------

def events(ovl, pile_id):
    """(begin-event cells, end-event cells) of the entries of `ovl` on pile `pile_id`, as AddLayers places them."""
    o = np.asarray(ovl)
    b = np.concatenate([o["lhs_begin"][o["lhs_id"] == pile_id], o["rhs_begin"][o["rhs_id"] == pile_id]]).astype(np.int64)
    e = np.concatenate([o["lhs_end"][o["lhs_id"] == pile_id], o["rhs_end"][o["rhs_id"] == pile_id]]).astype(np.int64)
    return (b >> PSS) + 1, (e >> PSS) - 1


def assert_defined(lengths, ovl):
    """The input the reference itself defines: lhs_id < rhs_id in (query, emission) order, every end in [16, len], and
    an overlap whose end event precedes its begin event (it makes `coverage` wrap) keeps the begin event inside the pile,
    because pile.cc then writes every cell up to it."""
    o = np.asarray(ovl)
    lengths = np.asarray(lengths).astype(np.int64)
    n = lengths.shape[0]
    if o.shape[0] == 0:
        return
    assert o.dtype == DT
    assert np.all(o["lhs_id"] < o["rhs_id"]) and np.all(o["rhs_id"] < n)
    assert np.all(np.diff(o["lhs_id"].astype(np.int64)) >= 0)
    for side in ("lhs", "rhs"):
        ln = lengths[o[side + "_id"]]
        b, e = o[side + "_begin"].astype(np.int64), o[side + "_end"].astype(np.int64)
        assert np.all(b < e) and np.all(e >= 16) and np.all(e <= ln)
        xb, xe = (b >> PSS) + 1, (e >> PSS) - 1
        wraps = xe < xb
        assert np.all(xb[wraps] <= (ln[wraps] >> PSS))
        assert np.all(xe[~wraps] <= (ln[~wraps] >> PSS) - 1)


def lhs_offsets(ovl, n):
    """uint32[n + 1]: first overlap of every query read in a list grouped by ascending lhs_id (Map's per-read offsets)."""
    off = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum(np.bincount(np.asarray(ovl)["lhs_id"], minlength=n)[:n], out=off[1:])
    return off


def lhs_boundaries(ovl):
    """Indices at which a list grouped by lhs_id may be cut into parts: 0, every change of lhs_id, and the end."""
    lhs = np.asarray(ovl)["lhs_id"].astype(np.int64)
    return [0] + (np.flatnonzero(np.diff(lhs) != 0) + 1).tolist() + [lhs.shape[0]]


def split_parts(ovl, k):
    """The list cut at lhs boundaries into k parts of about the same number of queries (parts may come out empty)."""
    cuts = lhs_boundaries(ovl)
    pick = [cuts[(len(cuts) - 1) * i // k] for i in range(k + 1)]
    return [ovl[pick[i]:pick[i + 1]] for i in range(k)]


def boundary_between_feeders(ovl):
    """An lhs boundary whose two neighbouring queries both feed one rhs pile: (index, that pile), or None."""
    o = np.asarray(ovl)
    cuts = lhs_boundaries(o)
    for a, c, b in zip(cuts[:-2], cuts[1:-1], cuts[2:]):
        both = np.intersect1d(o["rhs_id"][a:c], o["rhs_id"][c:b])
        if both.size:
            return c, int(both[0])
    return None


def span(x, y, jb=0, je=0):
    """(begin, end) in bases with the begin event on cell x (>= 1) and the end event on cell y: covers cells [x, y)."""
    assert x >= 1 and 0 <= jb < 16 and 0 <= je < 16
    return ((x - 1) * 16 + jb, (y + 1) * 16 + je)


def short(e, gap):
    """(begin, end) of a short overlap whose END event (cell e) precedes its BEGIN event (cell e + gap, gap 1 or 2): the
    reference's coverage wraps to 2^32 - 1 over cells [e, e + gap)."""
    if gap == 1:
        return (e * 16, (e + 1) * 16 + 7)
    assert gap == 2
    return ((e + 1) * 16, (e + 1) * 16 + 9)


class _Builder:
    """Overlaps of one flush in arrival order; flush() groups them by query (stable), as Map's results are drained."""

    def __init__(self, lengths, wmod=89):
        self.lengths = np.asarray(lengths, dtype=np.uint32)
        self.c = 0
        self.cur = []
        self.wmod = wmod

    def auto(self, p, side):
        """A sane span inside pile p that varies with the running counter; the four coordinates of an overlap fall in
        four residue classes mod 16 (lhs begin 0, lhs end 5, rhs begin 1, rhs end 9), so all of them differ."""
        assert int(self.lengths[p]) >= 3040
        c = self.c
        x = 1 + (c * 7 + 3 * side) % 97
        w = 3 + (c * 5 + 2 * side) % self.wmod
        return (16 * x + side, 16 * (x + w) + (9 if side else 5))

    def add(self, l, r, lspan=None, rspan=None):
        assert l < r
        lspan = self.auto(l, 0) if lspan is None else lspan
        rspan = self.auto(r, 1) if rspan is None else rspan
        self.cur.append((l, lspan[0], lspan[1], r, rspan[0], rspan[1], 100000 + self.c, self.c & 1))
        self.c += 1

    def flush(self):
        cur = sorted(self.cur, key=lambda o: o[0])  # (stable)
        self.cur = []
        out = np.array(cur, dtype=DT) if cur else np.zeros(0, dtype=DT)
        assert_defined(self.lengths, out)
        return out


def _case(name, family, lengths, kmax, flushes, **claims):
    lengths = np.asarray(lengths, dtype=np.uint32)
    for f in flushes:
        assert_defined(lengths, f)
        f.setflags(write=False)
    lengths.setflags(write=False)
    assert family in FAMILIES
    return dict(name=name, family=family, lengths=lengths, kmax=kmax, flushes=flushes, claims=claims)


# ---- order -----------------------------------------------------------------------------------------------------------

ORDER_Q, ORDER_T, ORDER_L = (2, 3, 4, 5), (6, 7, 8), (9, 10, 11, 12)
ORDER_COUNTS = (63, 64, 65)


def _order_case(kmax):
    """Piles 6, 7, 8 are the rhs of the queries 2 .. 5 (whose emissions alternate between the three and the later piles)
    and the lhs of their own overlaps to 9 .. 12.  Flush 1 leaves them 63, 64 and 65 entries (kept, where kmax allows);
    flush 2 brings 63 / 64 / 65 incoming and 63 / 64 / 65 own."""
    lengths = 4000 + 16 * np.arange(13)
    b = _Builder(lengths)

    def one(n_in, n_own):
        seqs = [[(ORDER_Q[j % 4], t) for j in range(a)] + [(t, ORDER_L[(j + t) % 4]) for j in range(o)]
                for t, a, o in zip(ORDER_T, n_in, n_own)]
        for j in range(max(len(s) for s in seqs)):
            for s in seqs:
                if j < len(s):
                    b.add(*s[j])
            if j % 5 == 0:
                b.add(ORDER_Q[j % 4], ORDER_L[j % 4])  # passes the three piles by
        return b.flush()

    f1 = one((40, 40, 40), (23, 24, 25))
    f2 = one(ORDER_COUNTS, ORDER_COUNTS)
    return _case("order:kmax%d" % kmax, "order", lengths, kmax, [f1, f2],
                 arrived={t: [(40, 23 + i), (c, c)] for i, (t, c) in enumerate(zip(ORDER_T, ORDER_COUNTS))})


# ---- piles -----------------------------------------------------------------------------------------------------------

PILE_COUNTS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)


def _piles_case(n):
    """n piles; every fifth has no overlap at all and sits among the others."""
    lengths = 3200 + 16 * (np.arange(n) % 7)
    active = [i for i in range(n) if i % 5 != 2]
    b = _Builder(lengths)
    flushes = []
    for rnd in range(2):
        for idx, i in enumerate(active[:-1]):
            if rnd and idx % 2:
                continue
            rest = len(active) - idx - 1
            b.add(i, active[idx + 1 + (idx * 7 + rnd) % rest])
            if idx % 3 == 0:
                b.add(i, active[idx + 1 + (idx * 11 + 5) % rest])
        flushes.append(b.flush())
    return _case("piles:%d" % n, "piles", lengths, 32, flushes, quiet=[i for i in range(n) if i % 5 == 2])


def _piles_wide():
    """70 000 piles of 64 bases (4 cells); every third is a query whose rhs id is spread over everything above it, so
    the rhs keys use 17 bits and every digit pass of the 32-bit sort has work or is all zero; every third has nothing."""
    n = 70000
    lengths = np.full(n, 64)
    spans = ((0, 48), (16, 64), (0, 64))
    b = _Builder(lengths)
    flushes = []
    for rnd, step in enumerate((1, 10)):
        for i in range(0, n - 1, 3 * step):
            j = i + 1 + (i * 40503 + rnd) % (n - 1 - i)
            if j % 3 == 2:
                j -= 1
            b.add(i, j, lspan=spans[b.c % 3], rspan=spans[(b.c // 3) % 3])
        flushes.append(b.flush())
    return _case("piles:70000", "piles", lengths, 32, flushes, quiet=list(range(2, n, 3)))


# ---- kmax ------------------------------------------------------------------------------------------------------------

KMAX_VALUES = (1, 2, 16, 17, 32)
KMAX_FEED, KMAX_SINK = (0, 1, 2, 3), (9, 10, 11, 12)
KMAX_GROW, KMAX_FULL, KMAX_SKIP, KMAX_ONE, KMAX_NEVER = 4, 5, 6, 7, 8


def _kmax_case(kmax):
    """Three flushes.  Pile 4 grows to kmax - 1, then by one, then by one (sizes kmax - 1 / kmax / kmax + 1 before the
    cut); pile 5 sits at kmax and receives 3 kmax + 5 more, then one; piles 6 (kmax + 1 entries, cut) and 7 (one entry) are
    touched in flushes 1 and 3 only; pile 8 never.  Few distinct lengths, so that ties sit on the cut."""
    lengths = 4000 + 16 * np.arange(13)
    b = _Builder(lengths, wmod=7)

    plan = ({KMAX_GROW: kmax - 1, KMAX_FULL: kmax, KMAX_SKIP: kmax + 1, KMAX_ONE: 1},
            {KMAX_GROW: 1, KMAX_FULL: 3 * kmax + 5},
            {KMAX_GROW: 1, KMAX_FULL: 1, KMAX_SKIP: 2, KMAX_ONE: 1})
    flushes = []
    for step in plan:
        # the targets' arrivals interleaved; each target alternates between a feeder's overlap (it arrives reversed)
        # and one of its own
        for j in range(max(step.values())):
            for t in sorted(step):
                if j < step[t]:
                    if j % 2 == 0:
                        b.add(KMAX_FEED[(j // 2 + t) % 4], t)
                    else:
                        b.add(t, KMAX_SINK[(j // 2 + t) % 4])
        flushes.append(b.flush())
    return _case("kmax:%d" % kmax, "kmax", lengths, kmax, flushes, arrived=[dict(s) for s in plan])


# ---- sort ------------------------------------------------------------------------------------------------------------

SORT_KMAX = 16
SORT_SIZES = (16, 17, 40, 100)
SORT_PATTERNS = ("equal", "two", "cut_ties", "sides")


def _sort_lengths(pattern, m):
    """Overlap length of entry j (arrival order) of a list of m entries."""
    if pattern == "equal":
        return [480] * m
    if pattern == "two":
        return [480 if (j * 7) % 3 == 0 else 640 for j in range(m)]
    if pattern == "cut_ties":
        # distinct lengths by rank, except that ranks kmax - 2 .. kmax + 1 share one; arrival order j -> rank 7 j mod m
        by_rank = [2400 - 16 * r for r in range(m)]
        for r in range(SORT_KMAX - 2, min(SORT_KMAX + 2, m)):
            by_rank[r] = by_rank[SORT_KMAX - 2]
        return [by_rank[(7 * j) % m] for j in range(m)]
    assert pattern == "sides"
    return [480 + 16 * ((j * 5) % 9) for j in range(m)]


def _sort_patterns_case():
    """One pile per (size, pattern) at kmax 16: every list is sorted, the lists of 16 are not cut.  Every third entry of
    a list arrives reversed from a feeder, the others are the pile's own.  In `sides` the pile's own side is the longer
    one for even entries and the shorter one for odd entries."""
    feed, first = (0, 1, 2, 3), 4
    targets = [(s, p) for s in SORT_SIZES for p in SORT_PATTERNS]
    sinks = tuple(range(first + len(targets), first + len(targets) + 4))
    lengths = 4000 + 16 * np.arange(sinks[-1] + 1)
    b = _Builder(lengths)
    where = {}
    for t, (m, pattern) in enumerate(targets, start=first):
        where[(m, pattern)] = t
        for j, ln in enumerate(_sort_lengths(pattern, m)):
            begin = 16 * (1 + j % 5)
            other = ln - 16 * (1 + j % 2)
            mine = ln
            if pattern == "sides" and j % 2:
                mine, other = ln - 32, ln
            if j % 3 == 0:
                b.add(feed[j % 4], t, lspan=(begin + 16, begin + 16 + other), rspan=(begin, begin + mine))
            else:
                b.add(t, sinks[j % 4], lspan=(begin, begin + mine), rspan=(begin + 32, begin + 32 + other))
    return _case("sort:patterns", "sort", lengths, SORT_KMAX, [b.flush()], where=where)


KILLER_N = 1000
KILLER_PILES = (20, 44)


def _sort_killer_case():
    """64 piles = the 64 lanes of one wave of truncate_sort_kernel.  Piles 20 and 44 hold 1000 own entries (and nothing
    else) whose lengths are McIlroy's adversary for libstdc++'s introsort (oracle.antiqsort; pile 44: the same divided by
    7, heavy ties): std::sort gives up quicksort at its depth limit there, while every other lane sorts an ordinary list
    or has none."""
    n = 64
    lengths = np.full(n, 4000)
    b = _Builder(lengths)
    for i in range(n - 1):
        for j in range(3):
            r = i + 1 + (j * 5 + i) % (n - 1 - i)
            if i not in KILLER_PILES and r not in KILLER_PILES:
                b.add(i, r)
    lens = (np.uint32(KILLER_N + 5) - oracle.antiqsort(KILLER_N)).astype(np.int64)
    for p, ln in zip(KILLER_PILES, (lens, lens // 7)):
        above = [r for r in range(p + 1, n) if r not in KILLER_PILES]
        for j in range(KILLER_N):
            b.add(p, above[j % len(above)], lspan=(16, 16 + 48 + int(ln[j])), rspan=(32, 32 + 48))
    return _case("sort:killer", "sort", lengths, 32, [b.flush()],
                 killer={p: (48 + ln).tolist() for p, ln in zip(KILLER_PILES, (lens, lens // 7))})


DEEP_N = 66000


def _sort_deep_case():
    """Pile 0 receives 66 000 overlaps in one flush, all of them over cell 11: one lane sorts 66 000 keys, and the cell
    saturates at 65535 from depth alone."""
    n = 130
    lengths = np.full(n, 4000)
    b = _Builder(lengths)
    for j in range(DEEP_N):
        b.add(0, 1 + j % 128, lspan=(160, 160 + 48 + 16 * ((j * 7) % 50) + j % 3), rspan=(16 * (1 + j % 9), 16 * (5 + j % 9 + j % 4)))
    return _case("sort:deep", "sort", lengths, 32, [b.flush()], cell=(0, 11), depth=DEEP_N)


# ---- tiles -----------------------------------------------------------------------------------------------------------

TILE_CELLS = (8191, 8192, 8193, 16384, 16385, 8447, 8448, 8449, 16641, 16641)
TILE_CARRY_PILE = 9      # one overlap only: tile 1 of it has no event
TILE_EDGES = (1, 2, 8191, 8192, 8193, 16383, 16384, 16385)


def _tiles_case():
    """Piles of 8191 .. 16 641 cells (last tiles of 1, 255, 256, 257 cells among them) with begin and end events on every
    pair of the cells next to a tile edge, on cell 1 (a begin event cannot sit lower) and on the last cell; an overlap
    inside tile 1; one from tile 0 into tile 2 on a pile that has nothing else; a second flush on top of the first."""
    sink = len(TILE_CELLS)
    lengths = [c * 16 + (i * 5) % 16 for i, c in enumerate(TILE_CELLS)] + [8000]
    b = _Builder(lengths)
    for p, cells in enumerate(TILE_CELLS):
        if p == TILE_CARRY_PILE:
            b.add(p, sink, lspan=span(100, 16500))
            continue
        at = sorted({x for x in TILE_EDGES + (cells - 1,) if 1 <= x <= cells - 1})
        for x in at:
            for y in at:
                if x <= y:
                    b.add(p, sink, lspan=span(x, y, jb=(x + y) % 16, je=(3 * x + y) % 16 if y < cells - 1 else 0))
        if cells > 8300:
            b.add(p, sink, lspan=span(8200, 8300))
    f1 = b.flush()
    for p, cells in enumerate(TILE_CELLS):
        b.add(p, sink, lspan=span(1, cells - 1))
        if cells > TILE + 2:
            b.add(p, sink, lspan=span(TILE - 1, TILE + 1))
    f2 = b.flush()
    return _case("tiles:edges", "tiles", lengths, 32, [f1, f2], sink=sink)


WRAP_CELLS = 8449
WRAP_FIVES, WRAP_ZEROS, WRAP_FIVES2, WRAP_ZEROS2 = 0, 1, 2, 3


def _tiles_wrap_case():
    """Short overlaps, whose end event precedes their begin event: the reference's coverage wraps to 2^32 - 1 over the
    cells between them, so a cell holding 0 becomes 65535 and a cell holding 5 becomes 4.  Piles 0 and 2 hold 5 where the
    short overlaps fall (flush 1), piles 1 and 3 hold 0.  Flush 2 places them inside a tile (cell 100; cells 200, 201),
    across cells 8191 / 8192, with the begin event on the first cell of tile 1, with the end event on cell 0 and with the
    begin event one past the last cell.  Flushes 3 and 4 go on from the saturated cells of pile 1: 65535 - 1 = 65534 by
    another wrap, then + 1 and + 2 onto 65534 and 65535, and - 1 from 65535 at the tile edge."""
    sink = 4
    lengths = [WRAP_CELLS * 16 + 15] * 4 + [8000]
    last = WRAP_CELLS - 1
    b = _Builder(lengths)
    for p in (WRAP_FIVES, WRAP_FIVES2):
        for _ in range(5):
            b.add(p, sink, lspan=span(90, 210))
            b.add(p, sink, lspan=span(8185, 8200))
    f1 = b.flush()
    for p in (WRAP_FIVES, WRAP_ZEROS):
        for s in (short(100, 1), short(200, 2), short(8191, 2)):
            b.add(p, sink, lspan=s)
    for p in (WRAP_FIVES2, WRAP_ZEROS2):
        for s in (short(8191, 1), short(8189, 2), short(0, 1), short(last, 1)):
            b.add(p, sink, lspan=s)
    f2 = b.flush()
    b.add(WRAP_ZEROS, sink, lspan=short(100, 1))
    b.add(WRAP_ZEROS, sink, lspan=short(200, 1))
    f3 = b.flush()
    b.add(WRAP_ZEROS, sink, lspan=span(100, 101))
    b.add(WRAP_ZEROS, sink, lspan=span(200, 202))
    b.add(WRAP_ZEROS, sink, lspan=span(200, 202))
    b.add(WRAP_ZEROS, sink, lspan=short(8191, 1))
    f4 = b.flush()
    # (flush, pile, cell) -> value, by the rules above
    cells = {}
    for p, base in ((WRAP_FIVES, 4), (WRAP_ZEROS, 65535)):
        for c in (100, 200, 201, 8191, 8192):
            cells[(1, p, c)] = base
        cells[(1, p, 99)] = cells[(1, p, 101)] = cells[(1, p, 202)] = cells[(1, p, 8190)] = cells[(1, p, 8193)] = 5 if base == 4 else 0
    for p, base in ((WRAP_FIVES2, 4), (WRAP_ZEROS2, 65535)):
        for c in (8189, 8190, 8191):
            cells[(1, p, c)] = base
        cells[(1, p, 8188)] = cells[(1, p, 8192)] = 5 if base == 4 else 0
        cells[(1, p, 0)] = cells[(1, p, last)] = 65535   # (no sane overlap ever covers the first or the last cell)
        cells[(1, p, 1)] = cells[(1, p, last - 1)] = 0
    cells.update({(2, WRAP_ZEROS, 100): 65534, (2, WRAP_ZEROS, 200): 65534, (2, WRAP_ZEROS, 201): 65535,
                  (3, WRAP_ZEROS, 100): 65535, (3, WRAP_ZEROS, 200): 65535, (3, WRAP_ZEROS, 201): 65535,
                  (3, WRAP_ZEROS, 8191): 65534, (3, WRAP_ZEROS, 8192): 65535, (3, WRAP_ZEROS, 101): 0})
    return _case("tiles:wrap", "tiles", lengths, 32, [f1, f2, f3, f4], cells=cells, sink=sink,
                 prior={(3, WRAP_ZEROS, 100): 65534, (3, WRAP_ZEROS, 200): 65534, (3, WRAP_ZEROS, 201): 65535,
                        (3, WRAP_ZEROS, 8191): 65535})


# ---- all of them -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cases():
    out = [_order_case(k) for k in (200, 65, 32)]
    out += [_piles_case(n) for n in PILE_COUNTS] + [_piles_wide()]
    out += [_kmax_case(k) for k in KMAX_VALUES]
    out += [_sort_patterns_case(), _sort_killer_case(), _sort_deep_case()]
    out += [_tiles_case(), _tiles_wrap_case()]
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def names():
    return [c["name"] for c in cases()]


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


# a representative subset of every family for the other entry points (one-shot, device pointers, parts)
SUBSET = ("order:kmax65", "piles:5", "piles:257", "kmax:2", "kmax:17", "sort:patterns", "tiles:edges", "tiles:wrap")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference's state after every flush of the case, computed once per process and read-only."""
    out = run(by_name(name))
    for st in out:
        for a in st.values():
            a.setflags(write=False)
    return tuple(out)
