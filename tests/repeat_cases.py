"""ResolveRepeatInducedOverlaps on the device (raven_amd/csrc/repeats.hip, repeats.h: the eleven kernels behind
rvn_resolve_repeat_induced_overlaps) on crafted piles and overlaps: a plain reference of the stage, RepeatRef, and the
cases, tagged by the class of edge they place (TAGS).  tests/test_repeat_cases.py holds RepeatRef, the restatement
program and the host build of repeats.h to each other on every case and checks that every case is what its tags and
claims say; tests/test_gpu_repeat_cases.py runs the device over them.

cases() returns dicts: name, family (A regions of one pile, B components and medians, C update / check, D the loop),
tags, the StageInput fields (overlaps, coverage, kmers, begin, end, median, invalid) and claims: what the case holds BY
CONSTRUCTION, worked out by hand where a comment gives the arithmetic (regions, is_repetitive, iterations, components,
removed, removed_per_iteration, first-sweep runs, raw counts, the median a pile was judged with, a slope pair's fate).
Nothing here looks at what the code under test returns.

RepeatRef is raven::ResolveRepeatInducedOverlaps in plain Python, written from the reference alone: the loop of
RavenLib/src/construct.cc:493-559, GetOverlapType and ConnectedComponents (overlap_utils.cc:82-113, :135-178, the BFS with
its deque), Pile::FindRepetitiveRegions / UpdateRepetitiveRegions / CheckRepetitiveRegions / ClearRepetitiveRegions
(pile.cc:230-371), MergeRegions (pile.cc:373-400) and FindSlopes (pile.cc:403-600) with the monotone deques as written
there.  It shares no code with raven_amd/csrc/repeats.h, slopes.h, the oracle or tests/host/repeats_reference.cpp.

The reference's types are kept by hand: uint32 sums and differences wrap (U32), products are Python floats (IEEE
doubles, as in C++), clamp() caps at 65535, and a double assigned to a uint16 / uint32 is truncated (int()).  Its quirks
are kept too: FindRepetitiveRegions appends to repetitive_regions_ and merges the whole vector, regions are cleared only
for the members of the iteration's components and only when an overlap was removed, is_repetitive is never reset.

One departure, shared with the oracle: FindSlopes primes the right deque with data_[i] for i < w = 52 even when the pile
is shorter, which reads past the vector; here, as there, the priming stops at the pile's end.

Besides the dict the device call returns, RepeatRef keeps what the tests of the cases need: per pile the runs of the
first sweep, the final slopes, every (up, down) pair with the outcome of each rule, the raw number of regions before
MergeRegions, and per iteration the number of removed overlaps and the median each member was judged with."""
import functools
from collections import deque

import numpy as np

U32 = 0xFFFFFFFF
PSS = 4                # pile.h:21
W_SLOPE = 847 >> PSS   # 52
W_KMER = 479 >> PSS    # 29
GROUP = 12
FUZZ = 420 >> PSS      # 26
Q = 1.42

OVERLAP_DTYPE = np.dtype([("lhs_id", "<u4"), ("lhs_begin", "<u4"), ("lhs_end", "<u4"), ("rhs_id", "<u4"),
                          ("rhs_begin", "<u4"), ("rhs_end", "<u4"), ("score", "<u4"), ("strand", "<u4")])


def clamp(v):
    """pile.cc:12-17, on a double or an integer"""
    return v if v < 65535 else 65535


def overlap_type(o, begin, end):
    """GetOverlapType (overlap_utils.cc:82-113); begin / end: the piles' valid regions in bases."""
    l, lb, le, r, rb, re, _, strand = o
    lhs_length = (end[l] - begin[l]) & U32
    lhs_begin = (lb - begin[l]) & U32
    lhs_end = (le - begin[l]) & U32
    rhs_length = (end[r] - begin[r]) & U32
    if strand:
        rhs_begin = (rb - begin[r]) & U32
        rhs_end = (re - begin[r]) & U32
    else:
        rhs_begin = (rhs_length - ((re - begin[r]) & U32)) & U32
        rhs_end = (rhs_length - ((rb - begin[r]) & U32)) & U32
    overhang = (min(lhs_begin, rhs_begin) + min((lhs_length - lhs_end) & U32, (rhs_length - rhs_end) & U32)) & U32
    ll, rl = (lhs_end - lhs_begin) & U32, (rhs_end - rhs_begin) & U32
    if ll < ((ll + overhang) & U32) * 0.875 or rl < ((rl + overhang) & U32) * 0.875:
        return 0
    if lhs_begin <= rhs_begin and ((lhs_length - lhs_end) & U32) <= ((rhs_length - rhs_end) & U32):
        return 1
    if rhs_begin <= lhs_begin and ((rhs_length - rhs_end) & U32) <= ((lhs_length - lhs_end) & U32):
        return 2
    return 3 if lhs_begin > rhs_begin else 4


def connected_components(overlaps, begin, end, invalid):
    """ConnectedComponents (overlap_utils.cc:135-178): lists of pile ids in the order the BFS reaches them."""
    n = len(begin)
    connections = [[] for _ in range(n)]
    for o in overlaps:
        if overlap_type(o, begin, end) > 2:
            connections[o[0]].append(o[3])
            connections[o[3]].append(o[0])
    dst, visited = [], [False] * n
    for i in range(n):
        if invalid[i] or visited[i]:
            continue
        dst.append([])
        que = deque([i])
        while que:
            j = que.popleft()
            if visited[j]:
                continue
            visited[j] = True
            dst[-1].append(j)
            que.extend(connections[j])
    return dst


def merge_regions(src):
    """MergeRegions (pile.cc:373-400)"""
    dst, merged = [], [False] * len(src)
    for i in range(len(src)):
        if merged[i]:
            continue
        first, second = src[i]
        while True:
            merged[i] = False
            for j in range(i + 1, len(src)):
                if merged[j]:
                    continue
                if first < src[j][1] and second > src[j][0]:
                    merged[i] = merged[j] = True
                    first, second = min(first, src[j][0]), max(second, src[j][1])
            if not merged[i]:
                break
        dst.append([first, second])
    return dst


def _add(s, value, position):
    while s and s[-1][1] <= value:
        s.pop()
    s.append((position, value))


def _update(s, position):
    while s and s[0][0] <= position:
        s.popleft()


class _Runs:
    """first_x / last_x / found_x of FindSlopes and the emplace_back that goes with them"""

    def __init__(self, dst, kind):
        self.dst, self.kind, self.found, self.first, self.last = dst, kind, False, 0, 0

    def hit(self, i):
        if self.found:
            if ((i - self.last) & U32) > 1:
                self.dst.append([(self.first << 1 | self.kind) & U32, self.last])
                self.first = i
        else:
            self.found, self.first = True, i
        self.last = i

    def finish(self):
        if self.found:
            self.dst.append([(self.first << 1 | self.kind) & U32, self.last])


def find_slopes(data, q, first_sweep=None):
    """Pile::FindSlopes (pile.cc:403-600) on a list of ints; first_sweep (a list) receives a copy of the runs as they
    stand after the first loop, sorted."""
    dst = []
    w, size = W_SLOPE, len(data)
    left, right = deque(), deque()
    down, up = _Runs(dst, 0), _Runs(dst, 1)
    for i in range(min(w, size)):
        _add(right, data[i], i)
    for i in range(size):
        if i > 0:
            _add(left, data[i - 1], i - 1)
        _update(left, i - 1 - w)
        if i < size - w:
            _add(right, data[i + w], i + w)
        _update(right, i)
        d = int(clamp(data[i] * q))  # uint16 d
        if i != 0 and left[0][1] > d:
            down.hit(i)
        if i != size - 1 and right[0][1] > d:
            up.hit(i)
    down.finish()
    up.finish()
    if first_sweep is not None:
        first_sweep.extend(tuple(r) for r in sorted(dst))
    if not dst:
        return dst

    # separate overlapping slopes
    while True:
        dst.sort()
        changed = False
        for i in range(len(dst) - 1):
            if dst[i][1] < (dst[i + 1][0] >> 1):
                continue
            if dst[i][0] & 1:
                right.clear()
                up.found = False
                sb, se = dst[i][0] >> 1, min(dst[i][1], dst[i + 1][1])
                for j in range(sb, se + 1):
                    _add(right, data[j], j)
                for j in range(sb, se):
                    _update(right, j)
                    if clamp(data[j] * q) < right[0][1]:
                        up.hit(j)
                up.finish()
                dst[i][0] = (se << 1 | 1) & U32
            else:
                if dst[i][1] == (dst[i + 1][0] >> 1):
                    continue
                left.clear()
                down.found = False
                sb, se = max(dst[i][0] >> 1, dst[i + 1][0] >> 1), dst[i][1]
                for j in range(sb, se + 1):
                    if left and clamp(data[j] * q) < left[0][1]:
                        down.hit(j)
                    _add(left, data[j], j)
                down.finish()
                dst[i][1] = sb
            changed = True
            break
        if not changed:
            break

    # narrow slopes
    for i in range(len(dst) - 1):
        if (dst[i][0] & 1) and not (dst[i + 1][0] & 1):
            sb, se = dst[i][1], dst[i + 1][0] >> 1
            if ((se - sb) & U32) > w:
                continue
            max_coverage = 0
            for j in range(sb + 1, se):
                max_coverage = max(max_coverage, data[j])
            valid_point = dst[i][0] >> 1
            for j in range(dst[i][0] >> 1, sb + 1):
                if max_coverage > clamp(data[j] * q):
                    valid_point = j
            dst[i][1] = valid_point
            valid_point = dst[i + 1][1]
            for j in range(se, dst[i + 1][1] + 1):
                if max_coverage > clamp(data[j] * q):
                    valid_point = j
                    break
            dst[i + 1][0] = (valid_point << 1) & U32
    return dst


class PileTrace:
    """What one call of FindRepetitiveRegions went through."""

    def __init__(self):
        self.first_sweep = []  # (cell << 1 | is_up, last cell), sorted
        self.slopes = []       # the same pairs after FindSlopes
        self.pairs = []        # dict(up, down, span_ok, interior, found_peak, num_valid, accepted)
        self.kmer_groups = []
        self.raw = []          # the regions appended, in order


def new_regions(data, kmers, begin_, end_, median):
    """The regions pile.cc:230-310 appends (before MergeRegions) and their trace."""
    t = PileTrace()
    if len(kmers):
        region, count = [0, 0], 0
        for i in range(len(kmers)):
            if kmers[i] == 0:
                continue
            if count and ((i - region[1]) & U32) <= W_KMER:
                region[1] = i
                count += 1
                continue
            if count > GROUP:
                t.kmer_groups.append(tuple(region))
            region, count = [i, i], 1
        if count > GROUP:
            t.kmer_groups.append(tuple(region))
    t.raw.extend(t.kmer_groups)
    slopes = find_slopes(data, Q, t.first_sweep)
    t.slopes = [tuple(s) for s in slopes]
    if slopes:
        min_value = int(clamp(Q * median))
        for i in range(len(slopes) - 1):
            if not slopes[i][0] & 1:
                continue
            for j in range(i + 1, len(slopes)):
                if slopes[j][0] & 1:
                    continue
                b, e = slopes[i], slopes[j]
                rec = dict(up=tuple(b), down=tuple(e), span_ok=False, interior=0, found_peak=False, num_valid=0,
                           accepted=False)
                t.pairs.append(rec)
                span = ((((e[0] >> 1) + e[1]) & U32) // 2 - (((b[0] >> 1) + b[1]) & U32) // 2) & U32
                if span > 0.84 * ((end_ - begin_) & U32):
                    continue
                rec["span_ok"] = True
                peak_value = int(clamp(Q * max(data[b[1]], data[e[0] >> 1])))
                found_peak, num_valid = False, 0
                for x in range(b[1] + 1, e[0] >> 1):
                    rec["interior"] += 1
                    if data[x] > min_value:
                        num_valid += 1
                    if data[x] > peak_value:
                        found_peak = True
                rec["found_peak"], rec["num_valid"] = found_peak, num_valid
                if not found_peak or num_valid < 0.9 * (((e[0] >> 1) - b[1]) & U32):
                    continue
                rec["accepted"] = True
                t.raw.append((int(b[1] - 0.336 * ((b[1] - (b[0] >> 1)) & U32)) & U32,
                              int((e[0] >> 1) + 0.336 * ((e[1] - (e[0] >> 1)) & U32)) & U32))
    return t


class RepeatRef:
    """State of the stage: run() is construct.cc:504-555.  Inputs as rvn_resolve_repeat_induced_overlaps takes them
    (a tests.repeats_util.StageInput or anything with its fields)."""

    def __init__(self, inp):
        self.n = int(inp.n)
        self.overlaps = [tuple(int(x) for x in o) for o in np.asarray(inp.overlaps).tolist()]
        coff, koff = inp.coverage_offsets, inp.kmers_offsets
        self.data = [inp.coverage[int(coff[i]):int(coff[i + 1])] for i in range(self.n)]
        self.kmers = [inp.kmers[int(koff[i]):int(koff[i + 1])] for i in range(self.n)]
        self.begin = [int(x) for x in inp.begin]  # bases: Pile::begin() / end()
        self.end = [int(x) for x in inp.end]
        self.begin_ = [b >> PSS for b in self.begin]
        self.end_ = [e >> PSS for e in self.end]
        self.median = [int(x) for x in inp.median]
        self.invalid = [bool(x) for x in inp.invalid]
        self.regions = [[] for _ in range(self.n)]  # repetitive_regions_: [first, second]
        self.is_repetitive = [False] * self.n
        self._memo = {}
        # the trace
        self.trace = {}            # pile -> PileTrace of its last FindRepetitiveRegions
        self.removed_per_iteration = []
        self.medians_used = []     # per iteration: {pile: median}
        self.components_per_iteration = []

    def _new_regions(self, p, median):
        key = (self.data[p].tobytes(), self.kmers[p].tobytes(), self.begin_[p], self.end_[p], median)
        t = self._memo.get(key)
        if t is None:  # the appended regions are a pure function of these
            t = self._memo[key] = new_regions(self.data[p].tolist(), self.kmers[p].tolist(), self.begin_[p],
                                              self.end_[p], median)
        return t

    def find_repetitive_regions(self, p, median):
        t = self._new_regions(p, median)
        self.trace[p] = t
        if t.raw:
            self.is_repetitive[p] = True
        self.regions[p] = merge_regions(self.regions[p] + [list(r) for r in t.raw])
        for it in self.regions[p]:
            it[0] = (max(self.begin_[p], it[0]) << 1) & U32
            it[1] = min(self.end_[p], it[1])

    def _coords(self, p, o):
        if p == o[0]:
            return o[1] >> PSS, o[2] >> PSS
        return o[4] >> PSS, o[5] >> PSS

    def update_repetitive_regions(self, p, o):
        if not self.regions[p] or (p != o[0] and p != o[3]):
            return
        begin, end = self._coords(p, o)
        begin_, end_ = self.begin_[p], self.end_[p]
        offset = int(0.1 * ((end_ - begin_) & U32))
        for it in self.regions[p]:
            if begin < it[1] and (it[0] >> 1) < end:
                if (it[0] >> 1) < ((begin_ + offset) & U32) and ((begin - begin_) & U32) < ((end_ - end) & U32):
                    if end >= ((it[1] + FUZZ) & U32):
                        it[0] |= 1
                elif it[1] > ((end_ - offset) & U32) and ((begin - begin_) & U32) > ((end_ - end) & U32):
                    if ((begin + FUZZ) & U32) <= (it[0] >> 1):
                        it[0] |= 1

    def check_repetitive_regions(self, p, o):
        if not self.regions[p] or (p != o[0] and p != o[3]):
            return False
        begin, end = self._coords(p, o)
        begin_, end_ = self.begin_[p], self.end_[p]
        offset = int(0.1 * ((end_ - begin_) & U32))
        for it in self.regions[p]:
            if begin < it[1] and (it[0] >> 1) < end:
                if (it[0] >> 1) < ((begin_ + offset) & U32):
                    if end < ((it[1] + FUZZ) & U32) and (it[0] & 1):
                        return True
                elif it[1] > ((end_ - offset) & U32):
                    if ((begin + FUZZ) & U32) > (it[0] >> 1) and (it[0] & 1):
                        return True
        return False

    def run(self):
        iterations, components, removed = 0, 0, 0
        while True:
            iterations += 1
            comps = connected_components(self.overlaps, self.begin, self.end, self.invalid)
            if iterations == 1:
                components = len(comps)
            self.components_per_iteration.append([tuple(c) for c in comps])
            used = {}
            for comp in comps:
                medians = sorted(self.median[j] for j in comp)  # nth_element(size / 2)
                med = medians[len(medians) // 2]
                for j in comp:
                    used[j] = med
                    self.find_repetitive_regions(j, med)
            self.medians_used.append(used)
            for o in self.overlaps:
                self.update_repetitive_regions(o[0], o)
                self.update_repetitive_regions(o[3], o)
            kept = [o for o in self.overlaps
                    if not (self.check_repetitive_regions(o[0], o) or self.check_repetitive_regions(o[3], o))]
            gone = len(self.overlaps) - len(kept)
            self.removed_per_iteration.append(gone)
            removed += gone
            self.overlaps = kept
            if not gone:
                break
            for comp in comps:
                for j in comp:
                    self.regions[j] = []
        roff = np.zeros(self.n + 1, np.uint32)
        roff[1:] = np.cumsum([len(r) for r in self.regions])
        flat = [it for r in self.regions for it in r]
        return dict(overlaps=np.array(self.overlaps, dtype=OVERLAP_DTYPE).reshape(-1),
                    regions=np.array(flat, dtype=np.uint32).reshape(-1, 2), region_offsets=roff,
                    is_repetitive=np.array(self.is_repetitive, dtype=np.uint8).reshape(-1), iterations=iterations,
                    components=components, removed=removed)


# ---- the cases: building blocks ---------------------------------------------------------------------------------------

FAMILIES = ("A", "B", "C", "D")
TAGS = {
    # A: regions of one pile
    "plateau": "A", "median flip": "A", "validity rule": "A", "span rule": "A", "found_peak": "A", "clamp": "A",
    "spike": "A", "non-adjacent pair": "A", "first try full": "A", "retry": "A", "kmer push": "A", "kmer group": "A",
    "kmer gap": "A", "kmers empty": "A", "kmer edge": "A", "touch": "A", "rescan": "A", "kmer+plateau": "A",
    "clip": "A", "outside": "A", "length": "A", "lds split": "A", "chunk boundary": "A", "one-cell gap": "A",
    "scan boundary": "A", "pile end": "A",
    # B: components and medians
    "component size": "B", "ties": "B", "extreme medians": "B", "invalid member": "B", "no join": "B",
    "self overlap": "B", "sort bits": "B", "union-find": "B",
    # C: update / check
    "intersection": "C", "left branch": "C", "balance": "C", "fuzz": "C", "right branch": "C", "both ends": "C",
    "rhs role": "C", "self coordinates": "C", "two regions": "C", "roles": "C", "order": "C", "wrap": "C",
    "replicated": "C",
    # D: the loop
    "split": "D", "orphan": "D", "cascade": "D", "all removed": "D", "empty": "D",
}
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)
LDS_CELLS = 4096   # repeats.hip kRepCells
FIRST_TRY = 32     # repeats.hip kRepSlot
CHUNK = 64


def T(m):
    """clamp(1.42 * m) assigned to a uint16: min_value of a median, peak_value of a shoulder; strictly increasing below the
    clamp, since 1.42 > 1"""
    return int(clamp(Q * m))


def flat(cells, v=20):
    return np.full(cells, v, np.uint16)


def prof(cells, base, *spans):
    """base everywhere, then cells [lo, hi) at v for every (lo, hi, v)"""
    d = flat(cells, base)
    for lo, hi, v in spans:
        d[lo:hi] = v
    return d


def kset(cells, positions):
    """Pile::kmers_ of a pile: cells + 1 entries"""
    k = np.zeros(cells + 1, np.uint8)
    k[list(positions)] = 1
    return k


def up(first, last):
    return (first << 1 | 1, last)


def down(first, last):
    return (first << 1, last)


def o_(l, lb, le, r, rb, re, strand=1):
    """an overlap, coordinates in bases"""
    return (l, lb, le, r, rb, re, 0, strand)


def pre(p, e, q, q_cells=1000, extra=0):
    """cells [0, e) of p (+ extra bases) with the tail of q: GetOverlapType 4 (q longer than e cells), a join"""
    ln = e * 16 + extra
    return o_(p, 0, ln, q, q_cells * 16 - ln, q_cells * 16)


def suffix(p, b, p_cells, q):
    """cells [b, p_cells) of p with the head of q: type 3 (q longer), a join"""
    return o_(p, b * 16, p_cells * 16, q, 0, (p_cells - b) * 16)


def mid(p, b, e, q):
    """cells [b, e) inside p with the head of q: type 0 (internal), no join"""
    return o_(p, b * 16, e * 16, q, 0, (e - b) * 16)


def join(a, a_cells, b, ln=4):
    """the last ln cells of a with the first ln of b (b longer than ln): type 3.  On piles whose regions lie in the
    middle it meets no region, so it only joins."""
    return o_(a, (a_cells - ln) * 16, a_cells * 16, b, 0, ln * 16)


def _case(name, family, tags, coverage, median, overlaps=(), kmers=None, begin=None, end=None, invalid=None, **claims):
    n = len(coverage)
    coverage = [np.asarray(c, np.uint16) for c in coverage]
    assert all(TAGS[t] == family for t in tags), name
    return dict(name=name, family=family, tags=tuple(tags),
                overlaps=np.array(list(overlaps), dtype=OVERLAP_DTYPE).reshape(-1), coverage=coverage,
                kmers=[np.zeros(0, np.uint8)] * n if kmers is None else [np.asarray(k, np.uint8) for k in kmers],
                begin=np.zeros(n, np.uint32) if begin is None else np.asarray(begin, np.uint32),
                end=np.array([16 * len(c) for c in coverage], np.uint32) if end is None else np.asarray(end, np.uint32),
                median=np.full(n, median, np.uint16) if np.isscalar(median) else np.asarray(median, np.uint16),
                invalid=np.zeros(n, np.uint8) if invalid is None else np.asarray(invalid, np.uint8), claims=claims)


def stage_input(case):
    from tests import repeats_util as ru
    return ru.StageInput(case["overlaps"], case["coverage"], case["kmers"], case["begin"], case["end"], case["median"],
                         case["invalid"])


# ---- family A: regions of one pile (no overlaps: every valid pile is judged with its own median) ------------------------
#
# The plateau mark.  500 cells at 20, cells [200, 300) at 60, median 20.  First sweep: a cell at 20 has d = T(20) = 28 and
# is an up cell when a 60 lies within 52 cells on its right: cells 148..199; a down cell when one lies within 52 on its
# left: 300..351.  The cells at 60 have d = 85 and are neither.  The runs do not overlap and lie 101 > 52 cells apart, so
# the later sweeps leave them.  The pair: midpoints 173 and 325, 152 <= 0.84 * 500; peak_value = T(20) = 28 < 60;
# min_value = T(median); interior = cells 200..299, all 60.  Region: 199 - 0.336 * 51 = 181.86 -> 181 and
# 300 + 0.336 * 51 = 317.1 -> 317, so (181 << 1, 317) = (362, 317).
PLATEAU_REGION = (362, 317)


def plateau(h=60, base=20, cells=500):
    return prof(cells, base, (200, 300, h))


def stairs(steps, extra=0, step=60, base=10, top=200):
    """nested plateaus, each level twice the one below: every rise pairs with every fall; `extra` smaller plateaus behind
    them at 200-cell spacing"""
    cells = 2 * (steps * step + 100) + top + extra * 200
    d = flat(cells, base)
    lvl = base
    for s in range(steps):
        lvl *= 2
        d[100 + step * s:100 + 2 * steps * step + top - step * s] = lvl
    at = 2 * steps * step + top + 200
    for x in range(extra):
        d[at + 200 * x + 60:at + 200 * x + 120] = base * 4
    return d


def edge_profile(cells):
    """20 with three cells of 60 at either end (one at the end of a pile below 8 cells): slopes within 52 cells of both
    ends, where the device's zero padding stands for the missing cells"""
    d = flat(cells)
    if cells >= 8:
        d[:3] = 60
        d[-3:] = 60
    elif cells:
        d[-1] = 60
    return d


def _family_a():
    A = []

    def one(name, tags, cov, median=20, **kw):
        A.append(_case("A:" + name, "A", tags, [cov], median, **kw))

    # plateau / thresholds
    one("plateau:clean", ("plateau", "kmers empty"), plateau(), regions={0: [PLATEAU_REGION]}, is_repetitive={0: 1},
        runs={0: [up(148, 199), down(300, 351)]}, raw={0: 1})
    # T(42) = 59 < 60 (59.64), T(43) = 61 (61.06): every interior cell is valid at 42, none at 43
    one("median:42", ("median flip",), plateau(), 42, regions={0: [PLATEAU_REGION]}, is_repetitive={0: 1},
        flips_with="A:median:43")
    one("median:43", ("median flip",), plateau(), 43, regions={0: []}, is_repetitive={0: 0}, flips_with="A:median:42")
    # median 32: min_value = T(32) = 45 (45.44).  Plateau cells at 45 are not valid; their d = T(45) = 63 >= 60, so they
    # are no slope cells.  100 interior cells against 0.9 * (300 - 199) = 90.9: 91 valid pass, 90 do not.
    for dips in (9, 10):
        d = plateau()
        d[210:210 + 3 * dips:3] = 45
        one("dips:%d" % dips, ("validity rule",), d, 32, regions={0: [PLATEAU_REGION] if dips == 9 else []},
            is_repetitive={0: int(dips == 9)}, flips_with="A:dips:%d" % (19 - dips))
    # 120 cells, 0.84 * 120 = 100.8.  Plateau [20, 100): up 0..19 (midpoint 9), down 100..119 (109): 100 passes; region
    # 19 - 0.336 * 19 = 12.6 -> 12, 100 + 0.336 * 19 = 106.4 -> 106.  Plateau [20, 101): down 101..119 (110): 101 fails.
    # The issue's [8, 112): up 0..7 (3), down 112..119 (115): 112 fails.
    one("span:100", ("span rule",), prof(120, 20, (20, 100, 60)), regions={0: [(24, 106)]}, flips_with="A:span:101")
    one("span:101", ("span rule",), prof(120, 20, (20, 101, 60)), regions={0: []}, is_repetitive={0: 0},
        flips_with="A:span:100")
    one("span:112", ("span rule",), prof(120, 20, (8, 112, 60)), regions={0: []}, is_repetitive={0: 0})
    # found_peak false on its own: a pair whose interior is valid throughout (29 and 30 > T(20) = 28) but never above
    # peak_value = T(max of the two shoulders).  The first sweep alone cannot produce one (the cell that makes a shoulder
    # a slope cell lies above T(shoulder)); the narrowing of the slopes around a short plateau (pile.cc:565-597) does.
    one("peak:shoulders", ("found_peak",),
        np.concatenate([flat(18), flat(45, 29), flat(31, 30), flat(9), flat(10, 42), flat(8)]),
        pair={0: dict(span_ok=True, found_peak=False, interior=42, num_valid=42, accepted=False)})
    # the narrowest plateau: one cell of 60 at 200: up 148..199, down 201..252, one interior cell
    one("spike", ("spike",), prof(500, 20, (200, 201, 60)),
        runs={0: [up(148, 199), down(201, 252)]}, pair={0: dict(span_ok=True, interior=1)})
    # clamp and uint16: coverage 65535; min_value = T(65535) = 65535 is above every cell, T(0) = 0 below every plateau;
    # 46152 * 1.42 = 65535.84 clamps to 65535 (no slope against a plateau of 65535), 46151 * 1.42 = 65534.42 does not
    one("clamp:coverage", ("clamp",), plateau(65535), regions={0: [PLATEAU_REGION]})
    one("clamp:median65535", ("clamp",), plateau(65535), 65535, regions={0: []}, is_repetitive={0: 0})
    one("clamp:median0", ("clamp",), plateau(1, base=0), 0, regions={0: [PLATEAU_REGION]})
    one("clamp:base46152", ("clamp",), plateau(65535, base=46152), regions={0: []}, is_repetitive={0: 0}, slopes={0: 0})
    one("clamp:base46151", ("clamp",), plateau(65535, base=46151), regions={0: [PLATEAU_REGION]})

    # all pairs: plateaus of 60 cells a short gap apart; whether (up of the first, down of the last) holds depends on the
    # share of gap cells: gap 10: 120 of 130 interior cells against 0.9 * 131 = 117.9; gap 40: 120 of 160 against 144.9
    one("pairs:two:accept", ("non-adjacent pair",), prof(600, 20, (200, 260, 60), (270, 330, 60)),
        non_adjacent={0: True})
    one("pairs:two:reject", ("non-adjacent pair",), prof(600, 20, (200, 260, 60), (300, 360, 60)),
        non_adjacent={0: False})
    one("pairs:three", ("non-adjacent pair",), prof(700, 20, (200, 260, 60), (265, 325, 60), (330, 390, 60)),
        non_adjacent={0: True})
    # nested staircases (median 5 under a base of 10): raw counts at, just above and far above the first try's 32
    one("stairs:32", ("first try full",), stairs(4, extra=3), 5, raw={0: 32})
    # five steps count 36 over the whole pile; a valid region of 1260 cells lets the span rule drop three of them
    one("stairs:33", ("retry",), stairs(5, extra=2), 5, end=[1260 * 16], raw={0: 33})
    one("stairs:97", ("retry",), stairs(10), 5, raw={0: 97})
    # the same pile as stairs:32 with one k-mer group in front: 33
    one("stairs:kmer33", ("retry", "kmer push"), stairs(4, extra=3), 5, kmers=[kset(1480, range(13))], raw={0: 33})
    A.append(_case("A:retry:several", "A", ("retry",),
                   [stairs(10), plateau(), stairs(5, extra=2), stairs(4, extra=3), stairs(11)], 5,
                   end=[1600 * 16, 500 * 16, 1260 * 16, 1480 * 16, 1720 * 16], raw={0: 97, 1: 1, 2: 33, 3: 32, 4: 115}))

    # k-mer groups on a flat pile (no slopes): more than 12 set cells, at most 29 apart
    one("kmers:12", ("kmer group",), flat(200), kmers=[kset(200, range(50, 62))], regions={0: []}, is_repetitive={0: 0})
    one("kmers:13", ("kmer group",), flat(200), kmers=[kset(200, range(50, 63))], regions={0: [(100, 62)]},
        is_repetitive={0: 1})
    one("kmers:gap29", ("kmer gap",), flat(400), kmers=[kset(400, range(10, 10 + 13 * 29, 29))],
        regions={0: [(20, 358)]})
    one("kmers:gap30", ("kmer gap",), flat(400), kmers=[kset(400, range(10, 10 + 13 * 30, 30))], regions={0: []},
        is_repetitive={0: 0})
    A.append(_case("A:kmers:empty", "A", ("kmers empty",), [plateau(), plateau()], 20,
                   kmers=[np.zeros(0, np.uint8), np.zeros(501, np.uint8)],
                   regions={0: [PLATEAU_REGION], 1: [PLATEAU_REGION]}))
    # groups at entry 0 and at the last entry, index `cells`: (0, 12) and (188, 200) -> (0, 12), (188 << 1, 200)
    one("kmers:edges", ("kmer edge",), flat(200), kmers=[kset(200, list(range(13)) + list(range(188, 201)))],
        regions={0: [(0, 12), (376, 200)]})

    # merge and clip, on the plateau mark's (181, 317) before the shift; k-mer groups come first in the vector.
    # MergeRegions: r.first < s.second && r.second > s.first, both strict
    def group(a, b):
        return kset(500, list(range(a, a + 12)) + [b])
    one("merge:touch-left", ("touch",), plateau(), kmers=[group(150, 181)], regions={0: [(300, 181), PLATEAU_REGION]})
    one("merge:overlap-left", ("touch", "kmer+plateau"), plateau(), kmers=[group(150, 182)], regions={0: [(300, 317)]})
    one("merge:touch-right", ("touch",), plateau(), kmers=[group(317, 345)], regions={0: [(634, 345), PLATEAU_REGION]})
    one("merge:overlap-right", ("touch", "kmer+plateau"), plateau(), kmers=[group(316, 345)],
        regions={0: [(362, 345)]})
    # A = (150, 185), C = (310, 345), B = the plateau's (181, 317): A misses C, absorbs B, and only the rescan meets C
    one("merge:rescan", ("rescan",), plateau(), kmers=[kset(500, list(range(150, 162)) + [185] + list(range(310, 322)) + [345])],
        regions={0: [(300, 345)]}, raw={0: 3})
    # the clip to [begin_, end_]: max(begin_, first) << 1, min(end_, second); a region outside keeps its inverted pair
    one("clip:left", ("clip",), plateau(), begin=[190 * 16], regions={0: [(380, 317)]})
    one("clip:right", ("clip",), plateau(), end=[310 * 16], regions={0: [(362, 310)]})
    one("clip:outside-left", ("outside",), flat(200), kmers=[kset(200, range(50, 63))], begin=[100 * 16],
        regions={0: [(200, 62)]})
    one("clip:outside-right", ("outside",), flat(200), kmers=[kset(200, range(188, 201))], end=[150 * 16],
        regions={0: [(376, 150)]})

    # wave geometry: pile lengths around the chunk of 64 and the LDS copy of 4096
    for n in LENGTHS:
        if n < 4095:
            one("len:%d" % n, ("length",), edge_profile(n), is_repetitive={0: 0} if n < 2 else {})
    d = edge_profile(4095)
    d[2000:2100] = 60
    one("len:4095", ("length", "lds split"), d)
    # the plateau mark at [2000, 2100): 1999 - 17.136 -> 1981, 2100 + 17.136 -> 2117
    for n in (4096, 4097):
        one("len:%d" % n, ("length", "lds split"), prof(n, 20, (2000, 2100, 60)), regions={0: [(3962, 2117)]})
    # runs of the first sweep against the chunks of 64 lanes.  An up run before a plateau that starts at s is s-52..s-1,
    # a down run behind one that ends before e is e..e+51; a step of 30 (T(30) = 42 < 60, 30 > 28) between 20 and 60
    # stretches a run beyond 52 cells.
    one("run:up:lane0", ("chunk boundary",), prof(300, 20, (116, 176, 60)), runs={0: [up(64, 115)]})
    one("run:up:lane63", ("chunk boundary",), prof(300, 20, (128, 188, 60)), runs={0: [up(76, 127)]})
    one("run:up:cross", ("chunk boundary",), prof(300, 20, (92, 152, 60)), runs={0: [up(40, 91)]})
    one("run:up:cross2", ("chunk boundary",), prof(300, 20, (112, 150, 30), (150, 210, 60)), runs={0: [up(60, 149)]})
    one("run:down:lane0", ("chunk boundary",), prof(300, 20, (20, 64, 60)), runs={0: [down(64, 115)]})
    one("run:down:lane63", ("chunk boundary",), prof(300, 20, (30, 76, 60)), runs={0: [down(76, 127)]})
    one("run:down:cross", ("chunk boundary",), prof(300, 20, (10, 40, 60)), runs={0: [down(40, 91)]})
    one("run:down:cross2", ("chunk boundary",), prof(300, 20, (10, 60, 60), (60, 100, 30)), runs={0: [down(60, 151)]})
    # two runs one unflagged cell apart: cell c at 50 (T(50) = 71 >= 60) between cells at 20.  Up: a plateau from c + 20
    # flags c-32.., the 50 itself flags c-52..c-1.  Down: a plateau that ends before c - 20; the 50 flags c+1..c+52.
    for c in (63, 64, 65):
        one("gap:up:%d" % c, ("one-cell gap",), prof(300, 20, (c, c + 1, 50), (c + 20, c + 60, 60)),
            runs={0: [up(c - 52, c - 1), up(c + 1, c + 19)]})
        one("gap:down:%d" % c, ("one-cell gap",), prof(300, 20, (c - 40, c - 20, 60), (c, c + 1, 50)),
            runs={0: [down(c - 20, c - 1), down(c + 1, c + 52)]})
    # the interior scan [b.second + 1, e.first >> 1) = the plateau's cells, beginning and / or ending on a multiple of 64
    one("scan:begin64", ("scan boundary",), prof(520, 20, (192, 300, 60)), regions={0: [(346, 317)]})
    one("scan:end64", ("scan boundary",), prof(520, 20, (200, 320, 60)), regions={0: [(362, 337)]})
    # [192, 320): 128 cells = two full ballots against 0.9 * 129 = 116.1; dips (45 at median 32, as above) in the first
    # and last lane of both: 11 dips leave 117, 12 leave 116
    for dips in (11, 12):
        d = prof(520, 20, (192, 320, 60))
        d[[192, 255, 256, 319] + list(range(200, 235, 5)) + ([300] if dips == 12 else [])] = 45
        one("scan:both:%d" % dips, ("scan boundary", "validity rule"), d, 32,
            regions={0: [(346, 337)] if dips == 11 else []}, flips_with="A:scan:both:%d" % (23 - dips))
    # slopes within 52 cells of both ends: down 3..54 behind the head, up 45..96 before the tail
    one("ends", ("pile end",), edge_profile(100), runs={0: [down(3, 54), up(45, 96)]})
    return A


def family_a_union():
    """Every pile of family A in one call (no overlaps), the piles of 4096 and 4097 cells next to the 0-cell pile."""
    A = [c for c in cases() if c["family"] == "A"]
    order = sorted(range(len(A)), key=lambda i: (A[i]["name"] not in ("A:len:4096", "A:len:0", "A:len:4097"),
                                                 {"A:len:4096": 0, "A:len:0": 1, "A:len:4097": 2}.get(A[i]["name"], 3)))
    A = [A[i] for i in order]
    cat = lambda k: [x for c in A for x in c[k]]
    return _case("A:union", "A", (), cat("coverage"), np.array(cat("median"), np.uint16), kmers=cat("kmers"),
                 begin=cat("begin"), end=cat("end"), invalid=cat("invalid")), A


# ---- family B: components and medians -----------------------------------------------------------------------------------
#
# Probes: the plateau mark with a plateau of height h is accepted iff T(median) < h (peak_value = T(20) = 28 < h, and the
# slopes do not depend on h > 28).  T is strictly increasing, so for a median M the pile hi(M) = plateau(T(M) + 1) is
# accepted iff the component's median is <= M, and lo(M) = plateau(T(M)) iff it is < M: the two bracket the median the
# stage used.  Their regions lie in the middle of the pile (181 >= 50 = offset, 317 <= 450), so no overlap flags them,
# and join() meets none of them.

def hi(M):
    return plateau(T(M) + 1)


def lo(M):
    return plateau(T(M))


def _component_case(name, tags, piles, edges, **claims):
    """piles: (coverage, median) or (coverage, median, invalid); edges: (a, b) joined by join(a, b)"""
    cov = [p[0] for p in piles]
    ovl = [join(a, len(cov[a]), b) for a, b in edges]
    return _case("B:" + name, "B", tags, cov, [p[1] for p in piles], overlaps=ovl,
                 invalid=[p[2] if len(p) > 2 else 0 for p in piles], **claims)


def _bracket_claims(hi_pile, lo_pile, M, **more):
    """what a component of median exactly M leaves on its two probes"""
    c = dict(regions={hi_pile: [PLATEAU_REGION], lo_pile: []}, median_used={hi_pile: M, lo_pile: M})
    c.update(more)
    return c


def _family_b():
    B = []
    s = flat(40)
    # sizes 1..5 with median 50 = the size / 2-th smallest (the upper one for even sizes)
    B.append(_component_case("size:1", ("component size",), [(hi(50), 50), (lo(50), 50)], [],
                             **_bracket_claims(0, 1, 50, components=2)))
    for k, meds in ((2, (40, 50)), (3, (40, 50, 60)), (4, (40, 45, 50, 60)), (5, (40, 45, 50, 60, 70))):
        piles = [(hi(50), meds[0]), (lo(50), meds[1])] + [(s, m) for m in meds[2:]]
        B.append(_component_case("size:%d" % k, ("component size",), piles, [(i, i + 1) for i in range(k - 1)],
                                 **_bracket_claims(0, 1, 50, components=1)))
    # ties: {50, 50, 50, 20} and {20, 20, 50, 50}: index 2 of either is 50
    B.append(_component_case("ties", ("ties",),
                             [(hi(50), 50), (lo(50), 50), (s, 50), (s, 20), (hi(50), 20), (lo(50), 20), (s, 50), (s, 50)],
                             [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7)],
                             regions={0: [PLATEAU_REGION], 1: [], 4: [PLATEAU_REGION], 5: []},
                             median_used={0: 50, 4: 50}, components=2))
    # {0, 65535} -> 65535: nothing is valid; {0, 0, 65535} -> 0: a plateau of 1 over 0 is; {46152, 46152} -> T = 65535
    # against a plateau of 65535, {46151, 46151} -> 65534
    B.append(_component_case("extremes", ("extreme medians",),
                             [(plateau(1, base=0), 0), (s, 65535), (plateau(1, base=0), 0), (s, 0), (s, 65535),
                              (plateau(65535), 46152), (s, 46152), (plateau(65535), 46151), (s, 46151)],
                             [(0, 1), (2, 3), (3, 4), (5, 6), (7, 8)],
                             regions={0: [], 2: [PLATEAU_REGION], 5: [], 7: [PLATEAU_REGION]},
                             median_used={0: 65535, 2: 0, 5: 46152, 7: 46151}, is_repetitive={0: 0, 5: 0}, components=4))
    # invalid piles: reached from a valid one, their median counts ({40, 50} -> 50) and they get regions; a component of
    # invalid piles only and an isolated invalid pile get none and are not counted
    B.append(_component_case("invalid", ("invalid member",),
                             [(s, 40), (hi(50), 50, 1), (s, 40), (lo(50), 50, 1), (plateau(), 20, 1), (s, 20, 1),
                              (plateau(), 20, 1), (plateau(), 20)],
                             [(0, 1), (2, 3), (4, 5)],
                             regions={1: [PLATEAU_REGION], 3: [], 4: [], 6: [], 7: [PLATEAU_REGION]},
                             median_used={1: 50, 3: 50}, is_repetitive={1: 1, 3: 0, 4: 0, 6: 0, 7: 1}, components=3))
    # overlaps of type 0 (internal), 1 (lhs contained) and 2 (rhs contained) join nothing: hi(50) keeps its own median
    # 50 (joined with the 90 it would be judged with 90)
    B.append(_case("B:type012", "B", ("no join",), [hi(50), flat(200)], [50, 90],
                   overlaps=[mid(0, 100, 150, 1), o_(1, 0, 3200, 0, 1600, 4800), o_(0, 1600, 4800, 1, 0, 3200)],
                   types=[0, 1, 2], components=2, regions={0: [PLATEAU_REGION]}, median_used={0: 50}))
    # a self-overlap (type 3) joins a pile with itself
    B.append(_case("B:self", "B", ("self overlap",), [hi(50), lo(50)], [50, 50],
                   overlaps=[o_(0, 4000, 8000, 0, 0, 4000), o_(1, 4000, 8000, 1, 0, 4000)], types=[3, 3],
                   components=2, regions={0: [PLATEAU_REGION], 1: []}))
    # n around 2^8: the sort key is (root << 16 | median) with non-members under root n, which needs one bit more than
    # n - 1 at n = 256.  Pile 0 roots a bracketed component; the non-members 3, 4 (65535) and n - 1 (0) would turn its
    # median into 60 if they fell into its segment.  A second bracketed component sits at the top ids.
    for n in (255, 256, 257):
        piles = [(s, 45)] * n
        piles[0:5] = [(hi(50), 40), (lo(50), 50), (s, 60), (s, 65535, 1), (s, 65535, 1)]
        piles[n - 4:n] = [(s, 60), (lo(50), 50), (hi(50), 40), (s, 0, 1)]
        B.append(_component_case("n:%d" % n, ("sort bits",), piles, [(0, 1), (1, 2), (n - 4, n - 3), (n - 3, n - 2)],
                                 regions={0: [PLATEAU_REGION], 1: [], n - 2: [PLATEAU_REGION], n - 3: []},
                                 median_used={0: 50, n - 2: 50}, components=n - 7))
    # union-find under contention; 2k piles, k medians of 40 and k of 50: index k is 50, and 40 as soon as one pile of
    # 50 is missed or the index is one lower
    tiny = flat(8)

    def crowd(name, n, edges, probes):
        piles = [(tiny, 40 if i < n // 2 else 50) for i in range(n)]
        piles[probes[0]] = (hi(50), piles[probes[0]][1])
        piles[probes[1]] = (lo(50), piles[probes[1]][1])
        B.append(_component_case(name, ("union-find",), piles, edges, **_bracket_claims(probes[0], probes[1], 50,
                                                                                        components=1)))
    path = [(i, i + 1) for i in range(4095)]
    crowd("path:ascending", 4096, path, (0, 4095))
    crowd("path:descending", 4096, path[::-1], (0, 4095))
    crowd("path:shuffled", 4096, [path[i] for i in np.random.default_rng(20261020).permutation(4095)], (0, 4095))
    crowd("star:hub-largest", 300, [(i, 299) for i in range(299)], (0, 1))
    crowd("star:hub-smallest", 300, [(0, i) for i in range(1, 300)], (298, 299))
    crowd("dense", 40, [(i, j) for i in range(40) for j in range(i + 1, 40)], (0, 39))
    return B


# ---- family C: update / check --------------------------------------------------------------------------------------------
#
# The update / check mark.  1000 cells at 20 with [20, 80) at 60: up 0..19, down 80..131, 61 > 52 cells apart.  Region:
# 19 - 0.336 * 19 = 12.6 -> 12, 80 + 0.336 * 51 = 97.1 -> 97: (24, 97); offset = 100, so it is a left region (12 < 100).
# An overlap [0, e) of the pile is on its left side (0 < 1000 - e); it sets the flag when e >= 97 + 26 = 123 and is removed
# when the flag is set and e < 123.  Mirrored: [920, 980) at 60: up 868..919, down 980..999; 919 - 17.136 -> 901,
# 980 + 0.336 * 19 = 986.4 -> 986: (1802, 986), a right region (986 > 900): [b, 1000) sets when b + 26 <= 901, i.e. b <= 875,
# and is removed when b >= 876.
LEFT_REGION, LEFT_FLAGGED = (24, 97), (25, 97)
RIGHT_REGION, RIGHT_FLAGGED = (1802, 986), (1803, 986)


def zl(h=60, cells=1000):
    return prof(cells, 20, (20, 80, h))


def _unit(z, a, b, c=300):
    """ten overlaps on a pile z = zl(cells=300) (offset 30, still a left region) and two flat neighbours"""
    return [pre(z, 122, b, c), mid(z, 97, 120, a), mid(z, 96, 120, a), pre(z, 12, b, c), pre(z, 13, a, c),
            pre(z, 123, a, c), o_(b, (c - 122) * 16, c * 16, z, 0, 122 * 16), join(a, c, b), pre(z, 150, b, c),
            mid(z, 150, 200, a)]


UNIT_REMOVED = (0, 2, 4, 6)  # [0, 122), [96, 120), [0, 13) and [0, 122) through the rhs role


def _replicated(name, units):
    cov, ovl = [], []
    for u in range(units):
        cov += [zl(cells=300), flat(300), flat(300)]
        ovl += _unit(3 * u, 3 * u + 1, 3 * u + 2)
    gone = [10 * u + k for u in range(units) for k in UNIT_REMOVED]
    return _case(name, "C", ("replicated",), cov, 20, overlaps=ovl, removed=len(gone), iterations=2,
                 survivors=sorted(set(range(10 * units)) - set(gone)), regions={0: [LEFT_FLAGGED], 3 * units - 3: [LEFT_FLAGGED]})


def _family_c():
    C = []
    N = flat(1000)

    def add(name, tags, cov, ovl, **claims):
        C.append(_case("C:" + name, "C", tags, cov, 20, overlaps=ovl, **claims))

    kept = lambda m, gone=(): sorted(set(range(m)) - set(gone))
    weak, setter = pre(0, 122, 2), pre(0, 123, 1)
    # the mark: the setter stands after the overlap it condemns; Update sees every overlap before any Check
    add("mark:weak+setter", ("fuzz", "order"), [zl(), N, N], [weak, setter], removed=1, iterations=2, components=1,
        survivors=[1], regions={0: [LEFT_FLAGGED]})
    add("mark:weak", ("fuzz",), [zl(), N, N], [weak], removed=0, iterations=1, components=2, regions={0: [LEFT_REGION]})
    add("mark:short-setter", ("fuzz",), [zl(), N, N], [weak, pre(0, 123, 1, extra=-1)], removed=0, iterations=1,
        components=1, regions={0: [LEFT_REGION]})
    # the intersection begin < second && (first >> 1) < end on (12, 97): [97, 120) and [0, 12) miss it, [96, 120) and
    # [0, 13) meet it and end below 123
    add("intersect", ("intersection",), [zl(), N, N, N, N, N],
        [mid(0, 97, 120, 2), mid(0, 96, 120, 3), pre(0, 12, 4), pre(0, 13, 5), setter], removed=2, iterations=2,
        survivors=[0, 2, 4], regions={0: [LEFT_FLAGGED]})
    # 1009 cells: offset = uint32(100.9) = 100.  Plateau [118, 178): 117 - 17.136 -> 99 < 100, 178 + 17.136 -> 195: a left
    # region, set at e >= 221.  Plateau [119, 179): (100, 196), neither left (100 < 100) nor right: nothing is ever set.
    N9 = flat(1009)
    add("left:99", ("left branch",), [prof(1009, 20, (118, 178, 60)), N9, N9], [pre(0, 220, 2, 1009), pre(0, 221, 1, 1009)],
        removed=1, iterations=2, survivors=[1], regions={0: [(199, 195)]})
    add("left:100", ("left branch",), [prof(1009, 20, (119, 179, 60)), N9, N9], [pre(0, 220, 2, 1009), pre(0, 222, 1, 1009)],
        removed=0, iterations=1, regions={0: [(200, 196)]})
    # begin - begin_ < end_ - end: [0, 1000) has 0 on either side and falls to neither branch of Update; [0, 999) sets
    add("balance:equal", ("balance",), [zl(), N, N], [weak, o_(0, 0, 16000, 1, 0, 16000)], removed=0, iterations=1,
        regions={0: [LEFT_REGION]})
    add("balance:less", ("balance",), [zl(), N, N], [weak, o_(0, 0, 999 * 16, 1, 16, 16000)], removed=1, iterations=2,
        survivors=[1], regions={0: [LEFT_FLAGGED]})
    # the right region
    zr = prof(1000, 20, (920, 980, 60))
    add("right:875", ("right branch", "fuzz"), [zr, N, N], [suffix(0, 876, 1000, 2), suffix(0, 875, 1000, 1)], removed=1,
        iterations=2, survivors=[1], regions={0: [RIGHT_FLAGGED]})
    add("right:876", ("right branch", "fuzz"), [zr, N, N], [suffix(0, 876, 1000, 2), suffix(0, 876, 1000, 1)], removed=0,
        iterations=1, regions={0: [RIGHT_REGION]})
    # 400 flat cells, offset 40, a k-mer region (30, 370): left (30 < 40) and right (370 > 360) at once.  [4, 400) fails
    # the left branch's balance (4 < 0), so Update's else-if takes the right branch: 4 + 26 <= 30 sets.  Check has no
    # balance term and never reaches its right branch: [10, 50) is removed (50 < 396), [20, 400) stays although
    # 20 + 26 > 30.  With [5, 400) in place of [4, 400) nothing is set.
    K = flat(400)
    kk = [kset(400, list(range(30, 343, 26)) + [370])] + [np.zeros(0, np.uint8)] * 3
    both = [mid(0, 10, 50, 2), o_(0, 20 * 16, 6400, 3, 0, 380 * 16)]
    C.append(_case("C:both:set", "C", ("both ends",), [K, K, K, K], 20, kmers=kk,
                   overlaps=[o_(0, 4 * 16, 6400, 1, 0, 396 * 16)] + both, removed=1, iterations=2, survivors=[0, 2],
                   regions={0: [(61, 370)]}))
    C.append(_case("C:both:miss", "C", ("both ends",), [K, K, K, K], 20, kmers=kk,
                   overlaps=[o_(0, 5 * 16, 6400, 1, 0, 395 * 16)] + both, removed=0, iterations=1,
                   regions={0: [(60, 370)]}))
    # the pile as rhs: its own coordinates are the rhs ones
    rweak, rsetter = o_(2, 878 * 16, 16000, 0, 0, 122 * 16), o_(1, 877 * 16, 16000, 0, 0, 123 * 16)
    add("rhs-role", ("rhs role",), [zl(), N, N], [rweak, rsetter], removed=1, iterations=2, survivors=[1],
        regions={0: [LEFT_FLAGGED]})
    # set through the rhs role, removed through the lhs role
    add("roles", ("roles", "rhs role"), [zl(), N, N], [weak, rsetter], removed=1, iterations=2, survivors=[1],
        regions={0: [LEFT_FLAGGED]})
    # lhs == rhs: the lhs coordinates both times.  ([0, 123), [877, 1000)) sets, ([877, 1000), [0, 122)) is not removed;
    # ([877, 1000), [0, 123)) does not set
    add("self:lhs", ("self coordinates",), [zl(), N, N],
        [weak, o_(0, 0, 123 * 16, 0, 877 * 16, 16000), o_(0, 877 * 16, 16000, 0, 0, 122 * 16)], removed=1, iterations=2,
        survivors=[1, 2], regions={0: [LEFT_FLAGGED]})
    add("self:rhs", ("self coordinates",), [zl(), N, N], [weak, o_(0, 877 * 16, 16000, 0, 0, 123 * 16)], removed=0,
        iterations=1, regions={0: [LEFT_REGION]})
    # two regions, the left one flagged: [876, 1000) stays
    add("two-regions", ("two regions",), [prof(1000, 20, (20, 80, 60), (920, 980, 60)), N, N, N],
        [weak, setter, suffix(0, 876, 1000, 3)], removed=1, iterations=2, survivors=[1, 2],
        regions={0: [LEFT_FLAGGED, RIGHT_REGION]})
    # begin_ = 10: plateau [30, 90): up 0..29 -> 29 - 0.336 * 29 = 19.3 -> 19, 90 + 17.136 -> 107: (38, 107), set at
    # e >= 133.  [5, 133) starts before begin_: 5 - 10 wraps and fails the balance; [10, 133) sets.
    zb = prof(1000, 20, (30, 90, 60))
    for b, gone in ((5, 0), (10, 1)):
        C.append(_case("C:wrap:begin:%d" % b, "C", ("wrap",), [zb, N, N], 20, begin=[160, 0, 0],
                       overlaps=[o_(0, 160, 132 * 16, 2, 0, 122 * 16), o_(0, b * 16, 133 * 16, 1, 0, (133 - b) * 16)],
                       removed=gone, iterations=1 + gone, regions={0: [(38 + gone, 107)]}))
    # [0, 1010) ends after end_: 1000 - 1010 wraps above 0 and passes the balance
    add("wrap:end", ("wrap",), [zl(), flat(1010), N], [weak, o_(0, 0, 1010 * 16, 1, 0, 1010 * 16)], removed=1,
        iterations=2, survivors=[1], regions={0: [LEFT_FLAGGED]})
    # the unit of ten overlaps on disjoint pile triples: 70 000 overlaps cross many blocks of the compaction
    C.append(_replicated("C:replicated", 7000))
    C.append(_replicated("C:replicated:small", 438))
    return C


# ---- family D: the loop --------------------------------------------------------------------------------------------------

def _family_d():
    D = []
    N, F = flat(1000), flat(200)
    weak, setter = pre(1, 122, 2), pre(1, 123, 3)
    # P = hi(50) hangs on Z = zl(200) (a region up to median 140).  {50, 50, 90, 90} -> 90: P has none; the weak overlap
    # Z-F goes, {50, 50, 90} -> 50: P's region appears.
    D.append(_case("D:split:appears", "D", ("split",), [hi(50), zl(200), N, N], [50, 50, 90, 90],
                   overlaps=[join(0, 500, 1), weak, setter], iterations=2, removed=1, removed_per_iteration=[1, 0],
                   components=1, survivors=[0, 2], regions={0: [PLATEAU_REGION], 1: [LEFT_FLAGGED]}, is_repetitive={0: 1},
                   median_per_iteration={0: [90, 50]}))
    # {20, 20, 50, 90, 90} -> 50: P has its region; F and G leave with the weak overlap, {50, 90, 90} -> 90: it is gone,
    # is_repetitive stays
    D.append(_case("D:split:disappears", "D", ("split",), [hi(50), zl(200), N, N, N], [50, 90, 20, 90, 20],
                   overlaps=[join(0, 500, 1), weak, setter, join(2, 1000, 4)], iterations=2, removed=1,
                   removed_per_iteration=[1, 0], components=1, survivors=[0, 2, 3],
                   regions={0: [], 1: [LEFT_FLAGGED]}, is_repetitive={0: 1}, median_per_iteration={0: [50, 90]}))
    # {valid Z, invalid B}: B gets its region in the first iteration, loses its only overlap, and is no member afterwards
    D.append(_case("D:orphan", "D", ("orphan",), [zl(), plateau(), N], 20, invalid=[0, 1, 0],
                   overlaps=[pre(0, 122, 1, 500), pre(0, 123, 2)], iterations=2, removed=1, removed_per_iteration=[1, 0],
                   components=1, survivors=[1], regions={0: [LEFT_FLAGGED], 1: []}, is_repetitive={0: 1, 1: 1}))
    # the cascade.  Z1 = zl(200), Z2 = zl(60), Z3 = zl(40) (piles 0..2, median 20) with their setters' flat neighbours 3..5
    # and L = 6 form the core (seven medians of 20); K = 7..14 (eight of 35) hangs on Z2's weak overlap, H = 15..29
    # (fifteen of 100) on Z1's, L on Z3's.  Iteration 1: 30 piles, index 15 -> 100, T = 142: only Z1 has a region, H
    # leaves.  2: 15 piles, index 7 -> 35, T = 49 < 60: Z2's appears, K leaves.  3: 7 piles -> 20, T = 28 < 40: Z3's
    # appears, L leaves.  4: nothing.
    cov = [zl(200), zl(60), zl(40)] + [F] * 27
    med = [20] * 7 + [35] * 8 + [100] * 15
    ovl = [pre(0, 122, 15, 200), pre(1, 122, 7, 200), pre(2, 122, 6, 200), pre(0, 123, 3, 200), pre(1, 123, 4, 200),
           pre(2, 123, 5, 200), join(3, 200, 4), join(4, 200, 5)]
    ovl += [join(i, 200, i + 1) for i in range(7, 14)] + [join(i, 200, i + 1) for i in range(15, 29)]
    D.append(_case("D:cascade", "D", ("cascade",), cov, med, overlaps=ovl, iterations=4, removed=3,
                   removed_per_iteration=[1, 1, 1, 0], components=1, survivors=list(range(3, len(ovl))),
                   regions={0: [LEFT_FLAGGED], 1: [LEFT_FLAGGED], 2: [LEFT_FLAGGED]},
                   median_per_iteration={0: [100, 35, 20, 20]}))
    # each of the two overlaps sets the flag of its lhs pile ([0, 123)) and falls to the flag of its rhs pile ([0, 122))
    D.append(_case("D:all-removed", "D", ("all removed",), [zl(), zl()], 20,
                   overlaps=[o_(0, 0, 123 * 16, 1, 0, 122 * 16), o_(1, 0, 123 * 16, 0, 0, 122 * 16)], iterations=2,
                   removed=2, removed_per_iteration=[2, 0], survivors=[], regions={0: [LEFT_REGION], 1: [LEFT_REGION]}))
    D.append(_case("D:empty:n0", "D", ("empty",), [], 20, iterations=1, removed=0, components=0))
    D.append(_case("D:empty:m0", "D", ("empty",), [plateau(), flat(30)], 20, iterations=1, removed=0, components=2,
                   regions={0: [PLATEAU_REGION], 1: []}))
    return D


# ---- all of them ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cases():
    out = _family_a() + _family_b() + _family_c() + _family_d()
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def names():
    return [c["name"] for c in cases()]


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the dict RepeatRef returns, the RepeatRef with its trace) of a case, computed once per process and read-only"""
    case = family_a_union()[0] if name == "A:union" else by_name(name)
    ref = RepeatRef(stage_input(case))
    out = ref.run()
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out, ref
