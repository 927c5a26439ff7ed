"""A plain numpy statement of the part of Map between the sketch and the chain — index build (stable sort, runs, member
counts), ram's Filter, the probe and the self-join — and the crafted minimizer streams the GPU tests feed to the engine
(tests/test_gpu_match.py).  Imports nothing of the engine; tests/test_match_reference.py holds it to the oracle.

An origin word is (id << 32) | (pos << 1) | strand; bit 63 = "also a query minimizer" (kQueryFlag), bit 62 = "query only:
a minimizer of a read outside the index batch" (kForeignFlag; raven_amd/csrc/common.h).

LEGAL STREAMS.  The kernels index per-read arrays with the ids of a stream and take the foreign entries of a run from its
front, so a stream must keep these rules or the device writes out of bounds — check_legal() asserts them and every
generator below ends with it:
  * every id is below n_reads_total (and below 2^30), every position below 2^31, every value below 4^k;
  * foreign entries come first in the stream and carry smaller ids than every member; a foreign entry is a query.
"""
from collections import namedtuple

import numpy as np

QUERY_FLAG = np.uint64(1 << 63)
FOREIGN_FLAG = np.uint64(1 << 62)
ID_MASK = np.uint64(0x3FFFFFFF)
NO_FILTER = 0xFFFFFFFF
POS_MAX = (1 << 31) - 1
_U = np.uint64

Index = namedtuple("Index", "values origins keys starts members")
Probe = namedtuple("Probe", "grp pos seg filtered")
Join = namedtuple("Join", "grp pos seg")


def origin(rid, pos, strand, query=False, foreign=False):
    return (int(rid) << 32) | (int(pos) << 1) | int(strand) | (int(QUERY_FLAG) if query or foreign else 0) | (
        int(FOREIGN_FLAG) if foreign else 0)


def ids_of(origins):
    return ((origins >> _U(32)) & ID_MASK).astype(np.int64)


def check_legal(values, origins, k, n_reads_total):
    values = np.asarray(values, dtype=np.uint64)
    origins = np.asarray(origins, dtype=np.uint64)
    assert values.shape == origins.shape
    if values.shape[0] == 0:
        return
    assert int(values.max()) < (1 << (2 * k))
    ids = ids_of(origins)
    assert int(ids.max()) < min(n_reads_total, 1 << 30)
    foreign = (origins & FOREIGN_FLAG) != 0
    nf = int(foreign.sum())
    assert foreign[:nf].all(), "foreign entries come first"
    assert ((origins[:nf] & QUERY_FLAG) != 0).all()
    if 0 < nf < ids.shape[0]:
        assert int(ids[:nf].max()) < int(ids[nf:].min()), "foreign reads have smaller ids than every member"


# ---- the reference ---------------------------------------------------------------------------------------------------

def sort_index(values, origins):
    """The index: values and origins stably sorted by value, the distinct keys, the run starts (u + 1) and the member
    count of every run = its length minus the foreign entries at its front."""
    values = np.ascontiguousarray(values, dtype=np.uint64)
    origins = np.ascontiguousarray(origins, dtype=np.uint64)
    order = np.argsort(values, kind="stable")
    v, o = values[order], origins[order]
    n = v.shape[0]
    if n == 0:
        return Index(v, o, v[:0], np.zeros(1, np.int64), np.zeros(0, np.int64))
    heads = np.flatnonzero(np.concatenate(([True], v[1:] != v[:-1])))
    starts = np.concatenate((heads, [n])).astype(np.int64)
    member_at = np.where((o & FOREIGN_FLAG) == 0, np.arange(n, dtype=np.int64), n)
    first_member = np.minimum(np.minimum.reduceat(member_at, heads), starts[1:])  # front of the run only
    return Index(v, o, v[heads], starts, starts[1:] - first_member)


def occurrence(member_counts, f):
    """ram's Filter: the value at index (1 - f) * U of the sorted per-key counts, plus one; no filter for f == 0 or no key."""
    u = len(member_counts)
    if f == 0 or u == 0:
        return NO_FILTER
    nth = int((1 - f) * u)  # the double expression of oracle/raven_oracle.cpp Filter and of index.hip index_filter
    if nth >= u:
        nth = u - 1
    return int(np.sort(np.asarray(member_counts))[nth]) + 1


def _match_words(qo, ro):
    """ram Map's (group, positions) of query origin words qo against index origin words ro."""
    lhs = (qo & _U(0xFFFFFFFF)) >> _U(1)
    rhs = (ro & _U(0xFFFFFFFF)) >> _U(1)
    strand = ((qo & _U(1)) == (ro & _U(1))).astype(np.uint64)
    with np.errstate(over="ignore"):
        diagonal = np.where(strand == 0, rhs + lhs, rhs - lhs + _U(3 << 30))
    rid = (ro >> _U(32)) & ID_MASK
    return (((rid << _U(1)) | strand) << _U(32)) | diagonal, (lhs << _U(32)) | rhs


def _expand(counts):
    """For counts c_0, c_1, ...: (index of the owner, index within the owner) of every element, owners in order."""
    counts = np.asarray(counts, dtype=np.int64)
    total = int(counts.sum())
    owner = np.repeat(np.arange(counts.shape[0], dtype=np.int64), counts)
    first = np.cumsum(counts) - counts
    return owner, np.arange(total, dtype=np.int64) - np.repeat(first, counts)


def probe_matches(index, q_values, q_origins, q_read_off, occurrence, avoid_equal, avoid_symmetric):
    """ram's Map up to the chain: for every query minimizer in order, Find; more than `occurrence` entries -> filtered;
    otherwise one match per entry of the run, in run order, unless avoid_equal / avoid_symmetric drops it.  Returns the
    matches of all reads back to back, the per-read offsets and the per-minimizer filtered flags."""
    q_values = np.ascontiguousarray(q_values, dtype=np.uint64)
    q_origins = np.ascontiguousarray(q_origins, dtype=np.uint64)
    q_read_off = np.asarray(q_read_off, dtype=np.int64)
    nq, u = q_values.shape[0], index.keys.shape[0]
    j = np.searchsorted(index.keys, q_values)
    found = j < u
    found[found] = index.keys[j[found]] == q_values[found]
    j = np.where(found, j, 0)
    n = np.where(found, index.starts[j + 1] - index.starts[j], 0) if u else np.zeros(nq, np.int64)
    filtered = n > occurrence
    n = np.where(filtered, 0, n)
    q, within = _expand(n)
    ro = index.origins[index.starts[j[q]] + within] if u else np.zeros(0, np.uint64)
    qo = q_origins[q]
    qid, rid = ids_of(qo), ids_of(ro)
    keep = np.ones(q.shape[0], bool)
    if avoid_equal:
        keep &= qid != rid
    if avoid_symmetric:
        keep &= qid <= rid
    grp, pos = _match_words(qo[keep], ro[keep])
    per_q = np.bincount(q[keep], minlength=nq)
    m_off = np.concatenate(([0], np.cumsum(per_q))).astype(np.uint64)
    return Probe(grp, pos, m_off[q_read_off], filtered.astype(np.uint8))


def join_matches(index, n_reads_total, occurrence, all_query, avoid_equal, avoid_symmetric, q_lo=0, q_hi=NO_FILTER):
    """The self-join over the sorted index (the rules above join_kernel in map.hip and beside kForeignFlag in common.h):
    a run of c entries whose first f are foreign has c - f members; it takes part when 0 < c - f <= occurrence.  Every
    entry of such a run that is a query (all of them with all_query, else those with kQueryFlag) and whose read id lies in
    [q_lo, q_hi) is matched with every MEMBER of the run (itself included unless avoid_equal), subject to avoid_equal /
    avoid_symmetric.  The matches of read id land in segment id; their order inside a segment is not defined (here: run
    order)."""
    u = index.keys.shape[0]
    lengths = index.starts[1:] - index.starts[:-1]
    live = (index.members > 0) & (index.members <= occurrence)
    run, within = _expand(np.where(live, lengths, 0))
    ent = index.starts[run] + within  # every entry of a live run, as a query candidate
    qo = index.origins[ent] if u else np.zeros(0, np.uint64)
    qid = ids_of(qo)
    is_q = (qid >= q_lo) & (qid < q_hi)
    if not all_query:
        is_q &= (qo & QUERY_FLAG) != 0
    ent, run, qo, qid = ent[is_q], run[is_q], qo[is_q], qid[is_q]
    e, jj = _expand(index.members[run])
    ro = index.origins[index.starts[run[e] + 1] - index.members[run[e]] + jj] if u else np.zeros(0, np.uint64)
    qo, qid = qo[e], qid[e]
    rid = ids_of(ro)
    keep = np.ones(e.shape[0], bool)
    if avoid_equal:
        keep &= qid != rid
    if avoid_symmetric:
        keep &= qid <= rid
    qo, ro, qid = qo[keep], ro[keep], qid[keep]
    order = np.argsort(qid, kind="stable")
    grp, pos = _match_words(qo[order], ro[order])
    seg = np.concatenate(([0], np.cumsum(np.bincount(qid, minlength=n_reads_total)))).astype(np.uint64)
    return Join(grp, pos, seg)


# ---- comparison helpers (each returns a list of mismatch messages; [] = equal) -----------------------------------------

def _first_diff(a, b):
    n = min(a.shape[0], b.shape[0])
    d = np.flatnonzero(a[:n] != b[:n])
    return int(d[0]) if d.shape[0] else n


def diff_arrays(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return []
    d = _first_diff(got.ravel(), want.ravel())
    return ["%s: %d entries, reference %d; first difference at %d: %s, reference %s" % (
        name, got.shape[0], want.shape[0], d, got.ravel()[d:d + 1], want.ravel()[d:d + 1])]


def diff_index(got_values, got_origins, got_u, ref):
    """Sorted content of the index, ORDER INCLUDED: the origins of a run must come out in stream order (stability)."""
    errs = diff_arrays("index values", got_values, ref.values) + diff_arrays("index origins", got_origins, ref.origins)
    if int(got_u) != ref.keys.shape[0]:
        errs.append("distinct keys: %d, reference %d" % (got_u, ref.keys.shape[0]))
    return errs


def diff_occurrence(got, want):
    return [] if int(got) == int(want) else ["occurrence: %d, reference %d" % (got, want)]


def diff_probe(got, want):
    """Probe output, exact and in order: segment offsets, both match words, filtered flags."""
    return (diff_arrays("segment offsets", got.seg, want.seg) + diff_arrays("match groups", got.grp, want.grp) +
            diff_arrays("match positions", got.pos, want.pos) + diff_arrays("filtered flags", got.filtered, want.filtered))


def _sorted_segments(grp, pos, seg):
    """(group, positions) pairs sorted inside every segment."""
    seg = np.asarray(seg, dtype=np.int64)
    owner = np.repeat(np.arange(seg.shape[0] - 1), np.diff(seg))
    order = np.lexsort((pos, grp, owner))
    return grp[order], pos[order]


def diff_join(got, want):
    """Join output: segment offsets exactly, every segment's matches as a sorted multiset."""
    errs = diff_arrays("segment offsets", got.seg, want.seg)
    if errs or got.grp.shape != want.grp.shape or got.pos.shape != want.pos.shape:
        return errs + ["matches: %d, reference %d" % (got.grp.shape[0], want.grp.shape[0])]
    gg, gp = _sorted_segments(got.grp, got.pos, got.seg)
    wg, wp = _sorted_segments(want.grp, want.pos, want.seg)
    return diff_arrays("match groups (sorted per segment)", gg, wg) + diff_arrays("match positions (sorted per segment)", gp, wp)


# ---- generators ------------------------------------------------------------------------------------------------------

SORT_PATTERNS = ("equal", "top_byte", "one_bit", "ascending", "descending", "alternating", "dups")


def sort_keys(pattern, n, bits, seed=0):
    """n keys of `bits` bits."""
    rng = np.random.default_rng(1000 + seed)
    mask = (1 << bits) - 1
    i = np.arange(n, dtype=np.uint64)
    if pattern == "equal":
        v = np.full(n, mask & 0x2B5A5A5A5A5A5A5A, np.uint64)
    elif pattern == "top_byte":  # bits [bits - 8, bits) vary, the rest is constant
        v = (rng.integers(0, 256, n).astype(np.uint64) << _U(bits - 8)) | _U(mask >> 8 & 0x15555555555555)
    elif pattern == "one_bit":
        v = (rng.integers(0, 2, n).astype(np.uint64) << _U(bits // 2 + 1)) | _U(mask & 0x0808080808080808)
    elif pattern == "ascending":
        v = (i * _U(mask // max(n, 1))) if mask >= n else i * _U(mask + 1) // _U(max(n, 1))
    elif pattern == "descending":
        v = sort_keys("ascending", n, bits)[::-1].copy()
    elif pattern == "alternating":
        v = np.where(i & _U(1), _U(1), _U(mask))
    elif pattern == "dups":
        pool = rng.integers(0, mask + 1, 300, dtype=np.uint64)
        v = pool[rng.integers(0, 300, n)]
    elif pattern == "random":
        v = rng.integers(0, mask + 1, n, dtype=np.uint64)
    else:
        raise ValueError(pattern)
    assert v.shape[0] == n and (n == 0 or int(v.max()) <= mask)
    return v.astype(np.uint64)


def serial_origins(n, per_read=4096):
    """Distinct origins in stream order (read, position): entry i = read i / per_read, position i % per_read."""
    i = np.arange(n, dtype=np.uint64)
    return ((i // _U(per_read)) << _U(32)) | ((i % _U(per_read)) << _U(1)) | (i & _U(1))


def sort_stream(pattern, n, k, seed=0):
    v, o = sort_keys(pattern, n, 2 * k, seed), serial_origins(n)
    check_legal(v, o, k, n // 4096 + 1)
    return v, o


def distinct_keys(u, k, seed=0):
    """u distinct values below 4^k, ascending."""
    space = 1 << (2 * k)
    assert u <= space
    if u * 2 >= space:
        return np.sort(np.random.default_rng(seed).permutation(space)[:u]).astype(np.uint64)
    v = np.unique(np.random.default_rng(seed).integers(0, space, 2 * u + 16, dtype=np.uint64))
    assert v.shape[0] >= u
    return np.sort(np.random.default_rng(seed + 1).permutation(v)[:u]).astype(np.uint64)


def counts_stream(member_counts, k, foreign_counts=None, foreign_only=0, seed=0, keys=None, per_read=4096):
    """A stream with one key per entry of member_counts (that many members, in shuffled stream positions) — plus, with
    foreign_counts, that many foreign entries of the key ahead of its members, and foreign_only further keys that have
    foreign entries (two each) and no member.  Returns values, origins, n_reads_total and the keys (ascending; key i has
    member_counts[i] members; the foreign-only keys are the last foreign_only ones).  per_read: entries per read id."""
    rng = np.random.default_rng(seed)
    mc = np.asarray(member_counts, dtype=np.int64)
    fc = np.zeros_like(mc) if foreign_counts is None else np.asarray(foreign_counts, dtype=np.int64)
    u = mc.shape[0] + foreign_only
    keys = distinct_keys(u, k, seed) if keys is None else np.asarray(keys, dtype=np.uint64)
    assert keys.shape[0] == u
    fc_all = np.concatenate((fc, np.full(foreign_only, 2, np.int64)))
    mc_all = np.concatenate((mc, np.zeros(foreign_only, np.int64)))
    fv = rng.permutation(np.repeat(keys, fc_all))
    mv = rng.permutation(np.repeat(keys, mc_all))
    n_foreign_reads = (fv.shape[0] + per_read - 1) // per_read
    fo = serial_origins(fv.shape[0], per_read) | QUERY_FLAG | FOREIGN_FLAG
    mo = serial_origins(mv.shape[0], per_read) + (_U(n_foreign_reads) << _U(32))
    mo = np.where(rng.integers(0, 2, mv.shape[0]) == 1, mo | QUERY_FLAG, mo)
    values, origins = np.concatenate((fv, mv)), np.concatenate((fo, mo))
    n_reads_total = n_foreign_reads + (mv.shape[0] + per_read - 1) // per_read + 1
    check_legal(values, origins, k, n_reads_total)
    return values, origins, n_reads_total, keys


# Filter: (name, member counts, f, the count the quantile must land on).  The histogram keeps counts below 256 in LDS, 256 ..
# 65534 in the global bins and 65535 and more in the overflow list (index.hip: occ_hist_kernel, index_filter).
FILTER_CASES = {
    "median_255_top_of_lds": ([1, 2, 255, 256, 257], 0.5, 255),
    "median_256_first_global_bin": ([1, 255, 256, 257, 257], 0.5, 256),
    "median_257": ([255, 256, 257, 257, 257], 0.5, 257),
    "all_counts_median_257": ([1, 2, 255, 256, 257, 65534, 65535, 65536, 70000], 0.5, 257),
    "median_65534_last_global_bin": ([1, 2, 255, 65534, 65535, 65536, 70000], 0.5, 65534),
    "median_65535_first_overflow": ([1, 65534, 65535, 65536, 70000], 0.5, 65535),
    "median_65536_second_overflow": ([65534, 65535, 65536, 70000], 0.5, 65536),
}
FILTER_FREQUENCIES = (0, 1e-9, 0.001, 0.5, 1.0)


class Runs:
    """A crafted index given run by run.  add(entries) makes one key; an entry = (read id, position, strand, query flag,
    foreign flag).  build() lays the entries out as a legal stream — foreign entries first, then by (id, position) — so the
    stable sort hands every run back in exactly that order."""

    def __init__(self, k, n_reads_total, keys=None, seed=0):
        self.k, self.n_reads_total, self.keys, self.seed, self.runs = k, n_reads_total, keys, seed, []

    def add(self, entries):
        self.runs.append([tuple(e) + (False,) * (5 - len(e)) for e in entries])
        return len(self.runs) - 1

    def build(self):
        keys = distinct_keys(len(self.runs), self.k, self.seed) if self.keys is None else np.asarray(self.keys, np.uint64)
        assert keys.shape[0] == len(self.runs) and np.unique(keys).shape[0] == keys.shape[0]
        rows = [(not e[4], e[0], e[1], e[2], int(keys[r]), origin(*e)) for r, run in enumerate(self.runs) for e in run]
        rows.sort(key=lambda t: t[:4])
        values = np.array([t[4] for t in rows], dtype=np.uint64)
        origins = np.array([t[5] for t in rows], dtype=np.uint64)
        check_legal(values, origins, self.k, self.n_reads_total)
        return values, origins


def members(ids, pos0=10, step=7, strand=0, query=True):
    """One member entry per id, at distinct positions."""
    return [(rid, pos0 + step * i, (strand + i) & 1 if strand == 2 else strand, query) for i, rid in enumerate(ids)]


def join_edge_runs(k=15, n_reads_total=300, foreign_reads=3):
    """The join's edge cases in one index of n_reads_total = 300 reads: ids [0, foreign_reads) are foreign reads.  Returns
    (Runs, dict name -> run number)."""
    R = Runs(k, n_reads_total)
    F = foreign_reads
    named = {}
    named["members_2_3_4_5"] = [R.add(members(range(F + 1, F + 1 + c))) for c in (2, 3, 4, 5)]
    # the member count decides, not the run length: 3 members behind 4 foreign entries
    named["foreign_prefix_3_members"] = R.add([(i % F, 5 + i, i & 1, True, True) for i in range(4)] + members([10, 11, 12]))
    named["only_foreign"] = R.add([(i % F, 50 + i, 0, True, True) for i in range(3)])
    named["single_entry"] = R.add(members([20]))
    named["single_member_behind_foreign"] = R.add([(1, 77, 1, True, True)] + members([21]))
    named["same_read_twice_both_strands"] = R.add([(30, 100, 0, True), (30, 900, 1, True), (31, 40, 1, True)])
    named["flagged_and_unflagged_of_one_read"] = R.add([(40, 11, 0, True), (40, 500, 0, False), (41, 9, 1, False), (42, 8, 0, True)])
    named["no_query_at_all"] = R.add(members([50, 51, 52], query=False))
    # both diagonal formulas at the ends of the position range
    named["positions_near_0_and_2_31"] = R.add([(60, 0, 0, True), (61, POS_MAX, 0, True), (62, 0, 1, True),
                                                (63, POS_MAX, 1, True), (64, 1, 0, True), (65, POS_MAX - 1, 1, True)])
    # reads without matches between reads with matches: ids around 0 (behind the foreign ones), 255, 256, 257 and 299
    named["ids_around_block_size"] = R.add(members([F, 254, 255, 256, 257, 258, 298, 299], strand=2))
    return R, named


def join_many_runs(n_runs, k=15, n_reads_total=300, seed=3):
    """n_runs runs (255 / 256 / 257: one block of join_kernel, exactly, and one more) of 1 to 4 members each."""
    rng = np.random.default_rng(seed)
    R = Runs(k, n_reads_total, seed=seed)
    for r in range(n_runs):
        c = 1 + r % 4
        ids = np.sort(rng.integers(0, n_reads_total, c))
        R.add([(int(rid), 3 * r + 1000 * i, int(rng.integers(0, 2)), bool(rng.integers(0, 4))) for i, rid in enumerate(ids)])
    return R


def join_big_run(c=1500, k=15, n_reads_total=300):
    """One run of c entries, all queries: c * c matches without avoid rules."""
    R = Runs(k, n_reads_total)
    R.add([(i % n_reads_total, 16 * (i // n_reads_total) + (i % 13), i & 1, True) for i in range(c)])
    return R


def probe_index(k, case, seed=0):
    """Crafted indexes for the probe path: (values, origins, n_reads_total, keys ascending, per-key counts)."""
    space = 1 << (2 * k)
    if case == "single_key":  # u = 1
        keys = np.array([space // 3], np.uint64)
    elif case == "gaps":  # table_kernel: bp = -1, neighbours at most 8 / more than 8 buckets apart, tail above the largest key
        keys = gap_keys(k)
    elif case == "dense":  # k = 5: so many keys that the table has one bucket per value (shift == 0)
        keys = distinct_keys(600, k, seed)
    elif case == "ends":  # value 0 and value 4^k - 1 are keys
        keys = np.unique(np.concatenate((np.array([0, 1, space - 2, space - 1], dtype=np.uint64), distinct_keys(40, k, seed))))
    else:
        raise ValueError(case)
    counts = 1 + (np.arange(keys.shape[0]) * 7 + seed) % 6
    values, origins, n_reads_total, keys = counts_stream(counts, k, seed=seed, keys=keys, per_read=64)  # (read ids 0 .. ~20)
    return values, origins, n_reads_total, keys, counts


def table_geometry(u, k):
    """(bits, shift) of the bucket table index.hip builds for u distinct keys."""
    bits = 1
    while (1 << bits) < 2 * u:
        bits += 1
    bits = min(max(8, bits), min(2 * k, 26))
    return bits, 2 * k - bits


def gap_keys(k, u=300):
    """u keys laid out by BUCKET of the table built for u keys (1024 buckets for 300 keys): the first key in bucket 3 (the
    fill before the first key), then twice the bucket steps 0 (v and v + 2 in one bucket, v + 1 absent), 1, 8 (the longest
    gap a lane fills alone), 9 (the shortest the wave fills), 40 and 200, the rest one or two buckets apart, and the last
    key below the top buckets (the tail fill)."""
    bits, shift = table_geometry(u, k)
    assert shift >= 2
    keys, b = [], 3
    steps = [0, 1, 8, 9, 40, 200] * 2
    while len(keys) < u:
        keys.append((b << shift) + 1)
        s = steps.pop(0) if steps else 1 + len(keys) % 2
        if s == 0:
            keys.append((b << shift) + 3)
            s = 1
        b += s
    keys = np.array(keys[:u], dtype=np.uint64)
    assert int(keys[-1] >> _U(shift)) < (1 << bits) - 2
    return keys


def bucket_gaps(keys, k):
    bits, shift = table_geometry(keys.shape[0], k)
    return np.diff((keys >> _U(shift)).astype(np.int64)), bits, shift


def probe_queries(keys, k, n_reads=9, seed=0):
    """Query values around an index with the given keys: every key; v - 1 and v + 1 of every key (absent ones among them,
    with both neighbours present where the keys are two apart); values below the smallest and above the largest key; 0 and
    4^k - 1.  Spread over n_reads reads of which reads 2 and 5 and the last one have no minimizer.  Returns q_values,
    q_origins, q_read_off and the ids of the query reads (they overlap the index's read ids)."""
    rng = np.random.default_rng(seed)
    space = 1 << (2 * k)
    ki = keys.astype(object)
    cand = [0, space - 1, max(int(ki[0]) - 1, 0), int(ki[0]) // 2, min(int(ki[-1]) + 1, space - 1),
            (int(ki[-1]) + space) // 2]
    for v in ki:
        cand += [int(v), max(int(v) - 1, 0), min(int(v) + 1, space - 1)]
    qv = np.array(cand, dtype=np.uint64)
    qv = qv[rng.permutation(qv.shape[0])]
    nq = qv.shape[0]
    empty = {2, 5, n_reads - 1}
    full = [r for r in range(n_reads) if r not in empty]
    cuts = np.sort(rng.integers(0, nq + 1, len(full) - 1))
    sizes = np.diff(np.concatenate(([0], cuts, [nq])))
    per_read = np.zeros(n_reads, np.int64)
    per_read[full] = sizes
    off = np.concatenate(([0], np.cumsum(per_read))).astype(np.uint32)
    rid = np.repeat(np.arange(n_reads, dtype=np.uint64), per_read)
    pos = np.arange(nq, dtype=np.uint64) - np.repeat(off[:-1].astype(np.uint64), per_read)
    qo = (rid << _U(32)) | ((pos * _U(3)) << _U(1)) | (rng.integers(0, 2, nq).astype(np.uint64))
    return qv, qo, off
