"""The second mapping pass (raven_amd/csrc/pass2.hip: add_kmers_flags_kernel, update_kernel, ed_pairs_kernel, the bounded
edit distance, identity_keep_kernel, classify_kernel, dedup_kernel, merge_invalid_kernel, the final sweep, reads_subset /
gather_reads_kernel) and the identity filter of ResolveContainedReads on crafted input: a plain reference and the cases.

The reference is the reference's own text written out in Python, single-threaded, on tuples and strings:
  overlap_length / overlap_update / overlap_type   overlap_utils.cc:10-113 (uint32 arithmetic reduced mod 2^32, the two
                                                   double comparisons with the reference's operand order)
  add_kmers                                        pile.cc:64-120 (std::unique on lists of strings, cells + 1 entries)
  edit_distance                                    the textbook unit-cost DP, a numpy row at a time
  identity_score                                   construct.cc:176-203 (inflated spans, rhs reverse-complemented on
                                                   strand 0, 1. - d / max(len) in double)
  Pass2Ref                                         construct.cc:316-491: prepare (:324-349), batch (:373-455), finish (:466-480)
  identity_filter_ref                              construct.cc:162-217 on CSR lists
tests/test_pass2_cases.py holds each of them to the oracle and every claim of every case to the reference's output;
tests/test_gpu_pass2_cases.py runs the cases on the device.

cases() returns a list of dicts:
  name, family   the case; family is one of FAMILIES
  reads          list of uint8 code arrays (A=0 C=1 G=2 T=3); ids are the indices
  begin, end     uint32[n]: the piles' valid regions in bases; invalid uint8[n]: the piles invalid at entry
  batches        list of dict(q_first, q_last, maps): the query reads [q_first, q_last) counted among the valid reads and
                 what Map gave for them, maps = [(query id, OVERLAP_DTYPE array, filtered positions, other positions)] in
                 Map order; `other positions` are the read's minimizers the occurrence filter did not skip (the device
                 sees them with flag 0, the reference not at all).  The `subset` family has batch_bases and freq instead:
                 whole read sets that go through the real Map.
  identity, kmer_len (== k of the engine the case needs)
  claims         what the case holds BY CONSTRUCTION (see check_claims)
Every generator keeps to input the reference defines (assert_defined).  Nothing here looks at what the code under test
returns."""
import functools
import zlib

import numpy as np

from oracle import oracle

DT = oracle.OVERLAP_DTYPE
FAMILIES = ("rules", "dedup", "finish", "identity", "kmers", "subset")
M32 = 0xFFFFFFFF
PSS = 4  # pile.h:21
W = 5    # window of every engine the cases run on
IDENTITIES = (0.75, 0.78, 0.8, 0.9, 1.0)
SPANS = (84, 127, 128, 129, 500, 1500)


# ---- the reference ---------------------------------------------------------------------------------------------------

def overlap_length(o):
    """GetOverlapLength (overlap_utils.cc:10-12)."""
    return max((o[5] - o[4]) & M32, (o[2] - o[1]) & M32)


def overlap_update(o, begin, end, invalid):
    """OverlapUpdate (overlap_utils.cc:14-80): the updated tuple, or None where the reference returns false (and leaves
    the overlap as it was)."""
    li, lb, le, ri, rb, re, score, strand = o
    if invalid[li] or invalid[ri]:
        return None
    Lb, Le, Rb, Re = int(begin[li]), int(end[li]), int(begin[ri]), int(end[ri])
    if lb >= Le or le <= Lb or rb >= Re or re <= Rb:
        return None
    r_head = Rb - rb if rb < Rb else 0
    r_tail = re - Re if re > Re else 0
    l_head = Lb - lb if lb < Lb else 0
    l_tail = le - Le if le > Le else 0
    lhs_begin = (lb + (r_head if strand else r_tail)) & M32
    lhs_end = (le - (r_tail if strand else r_head)) & M32
    rhs_begin = (rb + (l_head if strand else l_tail)) & M32
    rhs_end = (re - (l_tail if strand else l_head)) & M32
    if lhs_begin >= Le or lhs_end <= Lb or rhs_begin >= Re or rhs_end <= Rb:
        return None
    lhs_begin = max(lhs_begin, Lb)
    lhs_end = min(lhs_end, Le)
    rhs_begin = max(rhs_begin, Rb)
    rhs_end = min(rhs_end, Re)
    if lhs_begin >= lhs_end or lhs_end - lhs_begin < 84 or rhs_begin >= rhs_end or rhs_end - rhs_begin < 84:
        return None
    return (li, lhs_begin, lhs_end, ri, rhs_begin, rhs_end, score, strand)


def overlap_type(o, begin, end):
    """GetOverlapType (overlap_utils.cc:82-113): 0 internal, 1 lhs contained, 2 rhs contained, 3 lhs -> rhs, 4 rhs -> lhs."""
    li, lb, le, ri, rb, re, _, strand = o
    Lb, Le, Rb, Re = int(begin[li]), int(end[li]), int(begin[ri]), int(end[ri])
    lhs_length = (Le - Lb) & M32
    lhs_begin = (lb - Lb) & M32
    lhs_end = (le - Lb) & M32
    rhs_length = (Re - Rb) & M32
    rhs_begin = (rb - Rb) & M32 if strand else (rhs_length - ((re - Rb) & M32)) & M32
    rhs_end = (re - Rb) & M32 if strand else (rhs_length - ((rb - Rb) & M32)) & M32
    overhang = (min(lhs_begin, rhs_begin) + min((lhs_length - lhs_end) & M32, (rhs_length - rhs_end) & M32)) & M32
    l_span, r_span = (lhs_end - lhs_begin) & M32, (rhs_end - rhs_begin) & M32
    if float(l_span) < float((l_span + overhang) & M32) * 0.875 or float(r_span) < float((r_span + overhang) & M32) * 0.875:
        return 0
    if lhs_begin <= rhs_begin and (lhs_length - lhs_end) & M32 <= (rhs_length - rhs_end) & M32:
        return 1
    if rhs_begin <= lhs_begin and (rhs_length - rhs_end) & M32 <= (lhs_length - lhs_end) & M32:
        return 2
    if lhs_begin > rhs_begin:
        return 3
    return 4


def inflate(codes):
    return "".join("ACGT"[c] for c in np.asarray(codes).tolist())


def _unique(items):
    """std::unique + erase: consecutive equal elements collapse to the first."""
    out = []
    for x in items:
        if not out or out[-1] != x:
            out.append(x)
    return out


def lc_stages(kmer):
    """The three collapses of pile.cc:77-113 on one k-mer string: the strings left after each (all three, whether or
    not the reference would have gone on)."""
    out = []
    kmer = "".join(_unique([c for c in kmer]))
    out.append(kmer)
    polymers = []
    for i, c in enumerate(kmer):
        if i % 2 == 1:
            polymers[-1] += c
        else:
            polymers.append(c)
    kmer = "".join(_unique(polymers))
    out.append(kmer)
    polymers = []
    for i, c in enumerate(kmer):
        if polymers and i % 2 == 0:
            polymers[-1] += c
        else:
            polymers.append(c)
    kmer = "".join(_unique(polymers))
    out.append(kmer)
    return out


def lc_passes(kmer, kmer_len):
    return all(len(s) >= kmer_len // 2 + 1 for s in lc_stages(kmer))


def add_kmers(codes, positions, kmer_len, cells=None):
    """Pile::AddKmers (pile.cc:64-120) on the read `codes`: kmers_ ((len >> 4) + 1 entries), updated in place when
    `cells` is given."""
    seq = inflate(codes)
    if cells is None:
        cells = np.zeros((len(seq) >> PSS) + 1, dtype=np.uint8)
    for it in np.asarray(positions).tolist():
        kmer = seq[it:it + kmer_len]
        assert len(kmer) == kmer_len, "InflateData beyond the read"
        if lc_passes(kmer, kmer_len):
            cells[it >> PSS] = 1
    return cells


def edit_distance(a, b):
    """Unit-cost edit distance of two code arrays (or byte strings): the textbook DP, one row of len(b) + 1 at a time."""
    a = np.frombuffer(a, dtype=np.uint8) if isinstance(a, (bytes, bytearray)) else np.asarray(a, dtype=np.uint8)
    b = np.frombuffer(b, dtype=np.uint8) if isinstance(b, (bytes, bytearray)) else np.asarray(b, dtype=np.uint8)
    m = b.shape[0]
    # Rows are kept as r[j] = D[i][j] - j, so that the left neighbour, D[i][j] = min(D[i][j], D[i][j - 1] + 1) for ascending
    # j, is a running minimum of r.  In that form the upper neighbour is r[j] + 1 and the diagonal r[j - 1] + (b[j - 1] != a[i]) - 1.
    diag = {c: (b != c).astype(np.int32) - 1 for c in set(a.tolist())}
    r = np.zeros(m + 1, dtype=np.int32)
    up, cur = np.empty(m, dtype=np.int32), np.empty(m + 1, dtype=np.int32)
    for i, c in enumerate(a.tolist()):
        np.add(r[1:], 1, out=up)
        np.add(r[:-1], diag[c], out=cur[1:])
        np.minimum(cur[1:], up, out=cur[1:])
        cur[0] = i + 1
        np.minimum.accumulate(cur, out=r)
    return int(r[m]) + m


def revcomp(codes):
    return (3 - np.asarray(codes, dtype=np.uint8))[::-1].copy()


def score_spans(o, reads):
    """The two strings edlibAlign sees for an (updated) overlap (construct.cc:177-188)."""
    lhs = np.asarray(reads[o[0]][o[1]:o[2]], dtype=np.uint8)
    rhs = np.asarray(reads[o[3]][o[4]:o[5]], dtype=np.uint8)
    if not o[7]:
        rhs = revcomp(rhs)
    return lhs, rhs


def identity_score(o, reads):
    """construct.cc:176-203: 1. - distance / max(length), in double."""
    lhs, rhs = score_spans(o, reads)
    return 1. - float(edit_distance(lhs, rhs)) / max(lhs.shape[0], rhs.shape[0])


def kmax_of(maxlen, identity):
    """The largest distance the reference's rule keeps at this length: !(1. - x / maxlen < identity)."""
    x = 0
    while x < maxlen and not (1. - float(x + 1) / maxlen < identity):
        x += 1
    assert not (1. - float(x) / maxlen < identity)
    return x


class Pass2Ref:
    """FindOverlapsAndRepetetiveRegions (construct.cc:316-491) with Map's results handed in."""

    def __init__(self, lengths, begin, end, invalid):
        self.lengths = [int(x) for x in lengths]
        self.n = len(self.lengths)
        self.begin = [int(x) for x in begin]
        self.end = [int(x) for x in end]
        self.invalid = [int(bool(x)) for x in invalid]
        self.invalid_at_entry = list(self.invalid)
        self.is_contained = [0] * self.n
        self.back = []  # overlaps.back()
        self.cells = {}
        self.prepare()

    def prepare(self):
        """:324-349: valid reads first, by id; s = position of the first invalid read, 0 when there is none (so that
        nothing is mapped when every pile is valid)."""
        self.order = sorted(range(self.n), key=lambda i: (self.invalid[i], i))
        self.s = 0
        for i, rid in enumerate(self.order):
            if self.invalid[rid]:
                self.s = i
                break
        self.mapped = self.order[:self.s]

    def index_batches(self, batch_bases=1 << 30):
        """:353-359 and :461: [j, i + 1) ranges of the sorted reads; each is mapped to by the reads [0, i + 1)."""
        out, acc, j = [], 0, 0
        for i in range(self.s):
            acc += self.lengths[self.order[i]]
            if i != self.s - 1 and acc < batch_bases:
                continue
            acc = 0
            out.append((j, i + 1))
            j = i + 1
        return out

    def batch(self, maps, identity, codes, kmer_len=15):
        """:373-455 for one index batch: maps = (query id, overlaps, filtered positions[, ...]) in Map order."""
        assert self.s > 0 or not maps, "the reference maps nothing when no pile is invalid"
        results = []
        for entry in maps:
            qid, ovl, filtered = entry[0], entry[1], entry[2]
            filtered = np.asarray(filtered).tolist()
            if filtered:  # pile.cc:67-72
                if qid not in self.cells:
                    self.cells[qid] = np.zeros((self.lengths[qid] >> PSS) + 1, dtype=np.uint8)
                add_kmers(codes[qid], filtered, kmer_len, self.cells[qid])
            dst = [tuple(int(v) for v in o) for o in np.asarray(ovl, dtype=DT).tolist()]
            if identity != 0:  # :385-424
                kept = []
                for o in dst:
                    u = overlap_update(o, self.begin, self.end, self.invalid)
                    if u is None:
                        continue
                    if identity_score(u, codes) < identity:
                        continue
                    kept.append(u)
                dst = kept
            results.append(dst)
        for dst in results:  # :430-455
            for jt in dst:
                jt = overlap_update(jt, self.begin, self.end, self.invalid)
                if jt is None:
                    continue
                t = overlap_type(jt, self.begin, self.end)
                if t == 0:
                    continue
                elif t == 1:
                    self.is_contained[jt[0]] = 1
                elif t == 2:
                    self.is_contained[jt[3]] = 1
                else:
                    if self.back and self.back[-1][0] == jt[0] and self.back[-1][3] == jt[3]:
                        if overlap_length(self.back[-1]) < overlap_length(jt):
                            self.back[-1] = jt
                    else:
                        self.back.append(jt)

    def finish(self):
        """:466-480."""
        for i in range(self.n):
            if self.is_contained[i]:
                self.invalid[i] = 1
        kept = []
        for o in self.back:
            u = overlap_update(o, self.begin, self.end, self.invalid)
            if u is not None:
                kept.append(u)
        self.back = kept

    # the shapes rvn_pass2_fetch returns
    @property
    def overlaps(self):
        return np.array(self.back, dtype=DT) if self.back else np.zeros(0, DT)

    @property
    def contained(self):
        return np.array(self.is_contained, dtype=np.uint8)

    @property
    def kmers_offsets(self):
        """Every pile valid at entry has (len >> 4) + 1 cells (all 0 when AddKmers never reached it), the others none."""
        off = np.zeros(self.n + 1, dtype=np.uint64)
        for i in range(self.n):
            off[i + 1] = off[i] + (0 if self.invalid_at_entry[i] else (self.lengths[i] >> PSS) + 1)
        return off

    @property
    def kmers(self):
        off = self.kmers_offsets
        out = np.zeros(int(off[-1]), dtype=np.uint8)
        for i, c in self.cells.items():
            out[int(off[i]):int(off[i + 1])] = c
        return out

    def state(self):
        return dict(overlaps=self.overlaps, contained=self.contained, kmers=self.kmers, kmers_offsets=self.kmers_offsets)


def run(case):
    """The reference's result for a case with crafted batches."""
    assert case["family"] != "subset"
    ref = Pass2Ref([len(r) for r in case["reads"]], case["begin"], case["end"], case["invalid"])
    if ref.s:
        for b in case["batches"]:
            ref.batch(b["maps"], case["identity"], case["reads"], case["kmer_len"])
    ref.finish()
    return ref.state()


@functools.lru_cache(maxsize=None)
def reference(name):
    return run(by_name(name))


def identity_filter_ref(overlaps, offsets, reads, begin, end, invalid, identity):
    """construct.cc:162-217 on per-pile lists (CSR): (surviving overlaps with their updated coordinates, offsets)."""
    ovl = np.asarray(overlaps, dtype=DT).tolist()
    off = [int(x) for x in offsets]
    out, out_off = [], [0]
    for i in range(len(off) - 1):
        for o in ovl[off[i]:off[i + 1]]:
            o = tuple(int(v) for v in o)
            if identity != 0:
                u = overlap_update(o, begin, end, invalid)
                if u is None:
                    continue
                if identity_score(u, reads) < identity:
                    continue
                o = u
            out.append(o)
        out_off.append(len(out))
    return (np.array(out, dtype=DT) if out else np.zeros(0, DT)), np.array(out_off, dtype=np.uint32)


def diff_state(got, want):
    """None when two results (dicts of overlaps, contained, kmers, kmers_offsets) hold the same integers in the same order,
    else a sentence about the first difference."""
    g, w = np.asarray(got["kmers_offsets"]).astype(np.int64), np.asarray(want["kmers_offsets"]).astype(np.int64)
    if g.shape != w.shape or np.any(g != w):
        i = int(np.flatnonzero(g != w)[0]) if g.shape == w.shape else -1
        return "kmers_offsets differ (first at %d): %s, expected %s" % (i, g[max(i, 0):i + 2].tolist(), w[max(i, 0):i + 2].tolist())
    g, w = np.asarray(got["contained"]), np.asarray(want["contained"])
    if g.shape != w.shape:
        return "contained: %d piles, expected %d" % (g.shape[0], w.shape[0])
    bad = np.flatnonzero(g != w)
    if bad.size:
        return "contained[%d] = %d, expected %d; %d piles differ" % (bad[0], g[bad[0]], w[bad[0]], bad.size)
    g, w = np.asarray(got["overlaps"]), np.asarray(want["overlaps"]).astype(np.asarray(got["overlaps"]).dtype)
    n = min(g.shape[0], w.shape[0])
    bad = np.flatnonzero(g[:n] != w[:n])
    if bad.size:
        i = int(bad[0])
        fields = [f for f in DT.names if g[i][f] != w[i][f]]
        return "overlap %d of %d (expected %d): %s differ: %s, expected %s; %d entries differ" % (
            i, g.shape[0], w.shape[0], ", ".join(fields), g[i].tolist(), w[i].tolist(), bad.size)
    if g.shape != w.shape:
        longer = g if g.shape[0] > n else w
        return "overlaps: %d entries, expected %d; the first one beyond: %s" % (g.shape[0], w.shape[0], longer[n].tolist())
    g, w = np.asarray(got["kmers"]), np.asarray(want["kmers"])
    if g.shape != w.shape:
        return "kmers: %d cells, expected %d" % (g.shape[0], w.shape[0])
    bad = np.flatnonzero(g != w)
    if bad.size:
        i = int(bad[0])
        off = np.asarray(want["kmers_offsets"]).astype(np.int64)
        p = int(np.searchsorted(off, i, side="right")) - 1
        return "k-mer cell %d of read %d = %d, expected %d; %d cells differ" % (i - off[p], p, g[i], w[i], bad.size)
    return None


# ---- what the device sees of a batch ---------------------------------------------------------------------------------

def valid_ids(case):
    return [i for i in range(len(case["reads"])) if not case["invalid"][i]]


def device_batch(case, batch):
    """The arguments of the hook for one batch: (q_first, q_last, origins uint64, read_off uint32[q_last - q_first + 1],
    filtered flags uint8, overlaps) — the query sketch in (read, position) order with the flag of every minimizer."""
    valid = valid_ids(case)
    qf, ql = batch["q_first"], batch["q_last"]
    per_read = {}
    for entry in batch["maps"]:
        per_read[entry[0]] = entry
    org, flags, off, ovl = [], [], [0], []
    for idx in range(qf, ql):
        rid = valid[idx]
        if rid in per_read:
            entry = per_read[rid]
            pos = [(int(p), 1) for p in np.asarray(entry[2]).tolist()]
            pos += [(int(p), 0) for p in (np.asarray(entry[3]).tolist() if len(entry) > 3 else [])]
            pos.sort()
            for j, (p, f) in enumerate(pos):
                org.append((rid << 32) | (p << 1) | (j & 1))
                flags.append(f)
        off.append(len(org))
    for entry in batch["maps"]:
        if np.asarray(entry[1]).shape[0]:
            ovl.append(np.asarray(entry[1], dtype=DT))
    return (qf, ql, np.array(org, dtype=np.uint64), np.array(off, dtype=np.uint32), np.array(flags, dtype=np.uint8),
            np.concatenate(ovl) if ovl else np.zeros(0, DT))


def assert_defined(case):
    """The input the reference itself defines: ids in range, lhs = the query, spans inside the reads with begin < end,
    regions inside the reads, queries of a batch ascending inside [q_first, q_last) of the valid reads, k-mer positions
    <= len - kmer_len, kmer_len == k of the engine the case asks for."""
    reads = case["reads"]
    n = len(reads)
    lens = [len(r) for r in reads]
    assert len(case["begin"]) == n and len(case["end"]) == n and len(case["invalid"]) == n
    for i in range(n):
        assert 0 <= case["begin"][i] <= case["end"][i] <= lens[i], (case["name"], i)
    assert case["kmer_len"] == case["k"] and 1 <= case["kmer_len"] <= 31
    assert 0 <= case["identity"] <= 1
    if case["family"] == "subset":
        assert case["batch_bases"] > 0
        return
    valid = valid_ids(case)
    assert len(valid) < n, "a crafted case needs an invalid pile: the reference maps nothing otherwise"
    n_ovl = 0
    for b in case["batches"]:
        assert 0 <= b["q_first"] <= b["q_last"] <= len(valid)
        last = -1
        for entry in b["maps"]:
            qid, ovl = entry[0], np.asarray(entry[1])
            assert qid in valid and b["q_first"] <= valid.index(qid) < b["q_last"] and valid.index(qid) > last
            last = valid.index(qid)
            for pos in entry[2:]:
                p = np.asarray(pos).astype(np.int64)
                assert p.size == 0 or (lens[qid] >= case["kmer_len"] and p.min() >= 0 and p.max() <= lens[qid] - case["kmer_len"])
            pos = np.concatenate([np.asarray(x).astype(np.int64) for x in entry[2:]])
            assert np.unique(pos).shape[0] == pos.shape[0], "one minimizer per position"
            if ovl.shape[0] == 0:
                continue
            assert ovl.dtype == DT
            n_ovl += ovl.shape[0]
            assert np.all(ovl["lhs_id"] == qid) and np.all(ovl["rhs_id"] < n) and np.all(ovl["rhs_id"] != qid)
            assert np.all(ovl["strand"] <= 1)
            ll, rl = np.array(lens)[ovl["lhs_id"]], np.array(lens)[ovl["rhs_id"]]
            assert np.all(ovl["lhs_begin"] < ovl["lhs_end"]) and np.all(ovl["lhs_end"] <= ll)
            assert np.all(ovl["rhs_begin"] < ovl["rhs_end"]) and np.all(ovl["rhs_end"] <= rl)
    assert n_ovl <= 12000 and max(lens) <= 3000


# ---- helpers of the generators ---------------------------------------------------------------------------------------

def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _random_read(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def _ovl(rows):
    return np.array(rows, dtype=DT) if rows else np.zeros(0, DT)


def _group_maps(rows):
    """Overlap rows in Map order (grouped by ascending lhs) -> maps entries without minimizers."""
    maps = []
    for r in rows:
        if maps and maps[-1][0] == r[0]:
            maps[-1][1].append(r)
        else:
            assert not maps or maps[-1][0] < r[0], "Map order: ascending query"
            maps.append((r[0], [r]))
    return [(q, _ovl(rs), np.zeros(0, np.uint32), np.zeros(0, np.uint32)) for q, rs in maps]


def _case(name, family, reads, begin, end, invalid, batches, identity=0.0, kmer_len=15, claims=None, **more):
    case = dict(name=name, family=family, reads=reads, begin=np.array(begin, dtype=np.uint32),
                end=np.array(end, dtype=np.uint32), invalid=np.array(invalid, dtype=np.uint8), batches=batches,
                identity=float(identity), kmer_len=kmer_len, k=kmer_len, claims=claims or {})
    case.update(more)
    assert_defined(case)
    return case


def _one_batch(n_valid, rows):
    return [dict(q_first=0, q_last=n_valid, maps=_group_maps(rows))]


# ---- rules -----------------------------------------------------------------------------------------------------------
# Every overlap has two piles of its own (ids 2i, 2i + 1), so its fate shows as: an entry of the result ("kept"),
# contained[lhs] ("contained_lhs"), contained[rhs] ("contained_rhs") or nothing at all ("dropped").

RLEN = 2200  # every read of the family


class _Rules:
    def __init__(self):
        self.rows, self.begin, self.end, self.invalid, self.fates = [], [], [], [], []

    def add(self, label, fate, strand, lhs, rhs, L=(100, 1900), R=(100, 1900), rhs_invalid=False):
        """lhs / rhs: the GIVEN spans in bases; L / R: the valid regions."""
        i = len(self.rows)
        self.rows.append((2 * i, lhs[0], lhs[1], 2 * i + 1, rhs[0], rhs[1], 100 + i, strand))
        self.begin += [L[0], R[0]]
        self.end += [L[1], R[1]]
        self.invalid += [0, 1 if rhs_invalid else 0]
        self.fates.append((label + (":fwd" if strand else ":rev"), fate, 2 * i, 2 * i + 1))

    def typed(self, label, fate, strand, lb, le, l_len, rb, re, r_len, l_head=0, l_tail=0, r_head=0, r_tail=0):
        """An overlap whose coordinates AFTER OverlapUpdate are, relative to the regions and with the rhs mirrored on the
        opposite strand as GetOverlapType sees them, lhs [lb, le) of l_len and rhs [rb, re) of r_len.  One side may stick
        out of its region (by l_head / l_tail, or r_head / r_tail bases of the GIVEN span); the other side then carries
        the same surplus at the matching end, inside its region, and loses it in the update."""
        assert not ((l_head or l_tail) and (r_head or r_tail))
        assert (not l_head or lb == 0) and (not l_tail or le == l_len)
        Lb, Rb = 300, 300
        pb, pe = (Rb + rb, Rb + re) if strand else (Rb + r_len - re, Rb + r_len - rb)  # the rhs after the update, absolute
        assert (not r_head or pb == Rb) and (not r_tail or pe == Rb + r_len)
        lhs = (Lb + lb - l_head - (r_head if strand else r_tail), Lb + le + l_tail + (r_tail if strand else r_head))
        rhs = (pb - r_head - (l_head if strand else l_tail), pe + r_tail + (l_tail if strand else l_head))
        if l_head or l_tail:
            assert Rb <= rhs[0] and rhs[1] <= Rb + r_len, "the surplus of the other side stays inside its region"
        if r_head or r_tail:
            assert Lb <= lhs[0] and lhs[1] <= Lb + l_len
        self.add(label, fate, strand, lhs, rhs, (Lb, Lb + l_len), (Rb, Rb + r_len))

    def case(self, name):
        n = len(self.begin)
        rng = _rng("rules", name)
        reads = [_random_read(rng, RLEN) for _ in range(n)] + [_random_read(rng, 100)]
        return _case("rules:" + name, "rules", reads, self.begin + [0], self.end + [96], self.invalid + [1],
                     _one_batch(n - sum(self.invalid), self.rows), claims=dict(fates=self.fates))


def _rules_cases():
    out = []
    g = _Rules()
    for s in (0, 1):  # the first test of OverlapUpdate, and the same after the shift by the other side's surplus
        g.add("lhs_begin==L.end", "dropped", s, (1900, 1990), (200, 290))
        g.add("lhs_begin==L.end-1", "dropped", s, (1899, 1990), (200, 291))
        g.add("lhs_end==L.begin", "dropped", s, (10, 100), (200, 290))
        g.add("lhs_end==L.begin+1", "dropped", s, (10, 101), (200, 291))
        g.add("rhs_begin==R.end", "dropped", s, (200, 290), (1900, 1990))
        g.add("rhs_end==R.begin", "dropped", s, (200, 290), (10, 100))
        # lhs [1500, 1990) on L = [100, 1900), the rhs sticks out by 500: at its head on the same strand (the lhs begin
        # moves to 2000 >= L.end), at its tail on the other
        g.add("shifted lhs_begin>=L.end", "dropped", s, (1500, 1990), (0, 990) if s else (1010, 2000), R=(500, 1500))
        g.add("shifted lhs_end<=L.begin", "dropped", s, (10, 500), (1010, 2000) if s else (0, 990), R=(500, 1500))
    out.append(g.case("edges"))

    g = _Rules()
    for s in (0, 1):
        for left, fate in ((84, True), (83, False)):
            # the lhs is cut to `left` bases at its head / tail; lhs region of left + 10 bases, the rest near-contained
            g.typed("lhs head cut to %d" % left, "contained_lhs" if fate else "dropped", s, 0, left, 94, 400, 400 + left + 40,
                    1800, l_head=100)
            g.typed("lhs tail cut to %d" % left, "kept" if fate else "dropped", s, 816, 816 + left, 816 + left, 10,
                    10 + left + 40, 1800, l_tail=100)
            # the rhs, in the read's own direction; GetOverlapType sees it mirrored on the opposite strand
            g.typed("rhs head cut to %d" % left, "contained_rhs" if fate else "dropped", s, 400, 400 + left + 40, 1800,
                    0 if s else 10, left if s else 10 + left, 10 + left, r_head=100)
            if s:
                g.typed("rhs tail cut to %d" % left, "kept" if fate else "dropped", s, 10, 10 + left + 40, 1800,
                        816, 816 + left, 816 + left, r_tail=100)
            else:
                g.typed("rhs tail cut to %d" % left, "kept" if fate else "dropped", s, 1800 - left - 40, 1800, 1800,
                        0, left, 816 + left, r_tail=100)
    out.append(g.case("84"))

    g = _Rules()
    for s in (0, 1):
        for d, fate in ((-1, "dropped"), (0, None), (1, None)):
            a = 140 + d  # overhang 20: internal below 7 * 20
            g.typed("lhs len==7*overhang%+d" % d, fate or "contained_lhs", s, 20, 20 + a, 20 + a, 50, 200, 230)
            g.typed("rhs len==7*overhang%+d" % d, fate or "contained_rhs", s, 50, 200, 230, 20, 20 + a, 20 + a)
            g.typed("type 0|3 at %+d" % d, fate or "kept", s, 30, 30 + a, 30 + a, 20, 170, 200)
            g.typed("type 0|4 at %+d" % d, fate or "kept", s, 20, 170, 200, 30, 30 + a, 30 + a)
    out.append(g.case("0.875"))

    g = _Rules()
    for s in (0, 1):
        g.typed("lb==rb, l_rest==r_rest: 1 beats 2", "contained_lhs", s, 10, 1790, 1800, 10, 1790, 1800)
        g.typed("type 1, lb==rb", "contained_lhs", s, 10, 1790, 1800, 10, 1780, 1800)
        g.typed("type 3, lb==rb+1", "kept", s, 11, 1790, 1800, 10, 1780, 1800)
        g.typed("type 2, rb==lb", "contained_rhs", s, 10, 1780, 1800, 10, 1790, 1800)
        g.typed("type 4, rb==lb+1", "kept", s, 10, 1780, 1800, 11, 1790, 1800)
        g.typed("type 1, l_rest==r_rest", "contained_lhs", s, 5, 1790, 1800, 10, 1790, 1800)
        g.typed("type 4, l_rest==r_rest+1", "kept", s, 5, 1789, 1800, 10, 1790, 1800)
        g.typed("type 2, r_rest==l_rest", "contained_rhs", s, 10, 1790, 1800, 5, 1790, 1800)
        g.typed("type 3, r_rest==l_rest+1", "kept", s, 10, 1790, 1800, 5, 1789, 1800)
        g.add("rhs pile invalid at entry", "dropped", s, (1000, 1900), (100, 1000), rhs_invalid=True)
    out.append(g.case("types"))
    return out


# ---- dedup -----------------------------------------------------------------------------------------------------------
# Kept overlaps (type 3) between reads of 3000 bases with the region [100, 2900): the lhs ends at its region's end, the rhs
# begins at its region's begin, on the same strand; GetOverlapLength = max(a, b).

DLEN = 3000


def _kept(lhs, rhs, a, b, score=0):
    assert 84 <= a < 2800 and 84 <= b < 2800
    return (lhs, 2900 - a, 2900, rhs, 100, 100 + b, score, 1)


def _internal(lhs, rhs):  # type 0
    return (lhs, 1000, 1500, rhs, 1000, 1500, 7, 1)


def _short(lhs, rhs):  # dropped by OverlapUpdate
    return (lhs, 1000, 1083, rhs, 1000, 1200, 7, 1)


class _Dedup:
    def __init__(self, n_reads):
        self.n = n_reads
        self.rows = []       # everything Map gave, in order
        self.survivors = []  # what the list holds before the final sweep, by construction
        self.heads = []      # index of every run head in the list of KEPT overlaps
        self.n_kept = 0
        self.score = 0
        self.contained = []  # piles the interrupting overlaps mark
        self.regions = {}    # pile -> (begin, end) other than [100, 2900)

    def run(self, lhs, rhs, lengths, winner, between=None):
        """A run of kept overlaps of (lhs, rhs) with the given (a, b) spans; `winner` = index of the one that stays;
        between[i] = rows of other pairs emitted before entry i that do not end the run."""
        if winner is not None:
            self.heads.append(self.n_kept)
        for i, (a, b) in enumerate(lengths):
            for extra in (between or {}).get(i, []):
                self.rows.append(extra)
            self.score += 1
            row = _kept(lhs, rhs, a, b, self.score)
            self.rows.append(row)
            self.n_kept += 1
            if i == winner:
                self.survivors.append(row)

    def filler(self, lhs, count):
        """`count` runs of one overlap each: the same query against alternating other reads."""
        others = [r for r in range(self.n) if r != lhs]
        last = self.rows[-1][3] if self.rows and self.rows[-1][0] == lhs else None
        j = 0
        for _ in range(count):
            while others[j % len(others)] == last:
                j += 1
            last = others[j % len(others)]
            j += 1
            self.run(lhs, last, [(300 + (self.n_kept % 50), 200)], 0)

    def case(self, name, batches=None, **claims):
        rng = _rng("dedup", name)
        reads = [_random_read(rng, DLEN) for _ in range(self.n)] + [_random_read(rng, 100)]
        if batches is None:
            batches = _one_batch(self.n, self.rows)
        left = [o for o in self.survivors if o[0] not in self.contained and o[3] not in self.contained]
        claims.update(result=_ovl(left), contained=sorted(self.contained), heads=list(self.heads))
        begin = [self.regions.get(i, (100, 2900))[0] for i in range(self.n)] + [0]
        end = [self.regions.get(i, (100, 2900))[1] for i in range(self.n)] + [96]
        return _case("dedup:" + name, "dedup", reads, begin, end, [0] * self.n + [1], batches, claims=claims)


def _dedup_cases():
    out = []
    g = _Dedup(4)
    g.run(0, 1, [(300, 200)] * 2, 0)                      # a run at index 0, equal lengths: the first stays
    g.run(0, 2, [(300, 200)], 0)
    g.run(0, 3, [(300, 200), (301, 200), (299, 200)], 1)  # the maximum in the middle
    g.run(1, 2, [(500, 200), (300, 200), (499, 200)], 0)  # ... first
    g.run(1, 3, [(300, 200), (300, 200), (200, 301)], 2)  # ... last
    g.run(2, 3, [(300, 300), (300, 300), (300, 300)], 0)  # all equal
    g.run(2, 0, [(500, 100), (100, 600), (550, 550)], 1)  # decided by the lhs span in one entry, by the rhs span in another
    g.run(2, 1, [(100, 600), (601, 100), (601, 601)], 1)  # a tie between an lhs-decided and a later equal one
    g.run(3, 0, [(400, 200), (401, 200)], 1)              # a run at the end of the list
    out.append(g.case("small"))

    g = _Dedup(5)
    # one run in the reference: the overlaps between its entries are internal, dropped, or mark pile 4 as contained (type 2:
    # its whole region [100, 2000) inside read 0)
    g.regions[4] = (100, 2000)
    g.contained = [3, 4]
    type2 = (0, 500, 2400, 4, 100, 2000, 7, 1)
    g.run(0, 1, [(300, 200), (400, 200), (350, 200), (400, 200), (399, 200)], 1,
          between={1: [_internal(0, 2)], 2: [_short(0, 3)], 3: [_internal(0, 3), _short(0, 2)], 4: [type2]})
    # two runs: after the (0, 1) run above, the kept (0, 2) overlap, then (0, 1) again — a kept overlap of another pair in
    # between, so the second (0, 1) run has a survivor of its own
    g.run(0, 2, [(300, 200)], 0)
    g.run(0, 1, [(300, 200), (400, 200)], 1)
    # (not a kept overlap: (1, 4) in the middle of both regions is internal, type 0, so (1, 2) stays one run)
    g.run(1, 2, [(300, 200), (299, 200)], 0, between={1: [(1, 1000, 1700, 4, 1000, 1700, 9, 0)]})
    # a type-1 overlap between the entries of a run marks the run's own lhs pile: the survivor dies in the final sweep
    g.run(3, 1, [(300, 200), (310, 200)], 1, between={1: [(3, 100, 2900, 2, 100, 2900, 5, 1)]})
    out.append(g.case("interrupted"))

    for shift in (0, 1, 2):  # run heads at 255 / 256 / 257 and 4095 / 4096 / 4097 of the kept list
        g = _Dedup(6)
        g.filler(0, 255 + shift)
        g.run(0, 1 if g.rows[-1][3] != 1 else 2, [(300, 200), (300, 200), (310, 200)], 2)
        q = 1
        while g.n_kept < 4095 + shift:
            step = min(1000, 4095 + shift - g.n_kept)
            g.filler(q, step)
            q += 1
        q -= 1  # the run belongs to the last query of the filler
        assert q <= 5 and g.rows[-1][0] == q
        g.run(q, 0 if g.rows[-1][3] != 0 else (q + 1) % 6 or 1, [(300, 200), (320, 200), (320, 200)], 1)
        g.filler(q, 40)
        assert 255 + shift in g.heads and 4095 + shift in g.heads
        out.append(g.case("heads:%d,%d" % (255 + shift, 4095 + shift)))

    for name, winner in (("middle", 700), ("first", 0), ("last", 999), ("equal", None)):
        g = _Dedup(4)
        g.filler(0, 200)
        lengths = [(300, 200)] * 1000
        if winner is not None:
            lengths[winner] = (301, 200)
            if name == "middle":
                lengths[900] = (200, 301)  # the same length again, later: the first of them stays
        g.run(0, 3 if g.rows[-1][3] != 3 else 2, lengths, winner or 0)
        g.filler(1, 30)
        out.append(g.case("run1000:" + name))

    # a run that goes on from the last kept overlap of one batch into the first of the next
    g = _Dedup(4)
    g.filler(0, 3)
    g.run(1, 2, [(300, 200), (350, 200)], None)
    first = list(g.rows)
    g.rows = []
    g.run(1, 2, [(340, 200), (360, 200), (360, 200)], 1, between={0: [_internal(0, 3), _short(0, 2)]})
    g.run(1, 3, [(300, 200)], 0)
    g.filler(2, 3)
    second = list(g.rows)
    out.append(g.case("across_batches", batches=_one_batch(4, first) + _one_batch(4, second), runs_across_batches=1))
    return out


# ---- finish ----------------------------------------------------------------------------------------------------------

def _contains(lhs, rhs, lhs_in_rhs=True):
    """A type-1 overlap (lhs contained in rhs) or, with the roles swapped, type 2: the contained read's whole region against
    the middle of the other's."""
    if lhs_in_rhs:
        return (lhs, 100, 2900, rhs, 100, 2900, 5, 1)  # lb == rb == 0, both rests 0: type 1
    return (lhs, 90, 2900, rhs, 100, 2900, 5, 1)


def _finish_cases():
    out = []
    n = 6
    rng = _rng("finish")
    reads = [_random_read(rng, DLEN) for _ in range(n)] + [_random_read(rng, 100)]
    begin, end, invalid = [100] * n + [0], [2900] * n + [96], [0] * n + [1]
    # regions: read 3 gets a longer region so that a type-2 overlap exists (the rhs read 4 inside read 3)
    begin3, end3 = list(begin), list(end)
    begin3[3], end3[3] = 50, 2950

    def case(name, b1, b2, contained, survivors, begin=begin, end=end):
        return _case("finish:" + name, "finish", reads, begin, end, invalid, _one_batch(n, b1) + _one_batch(n, b2),
                     claims=dict(contained=contained, result=_ovl(survivors)))

    # pile 2 becomes contained in batch 2 (as the lhs of a type-1 overlap); kept overlaps that touch it sit in batch 1 and in
    # batch 2, before and after that overlap, with 2 as lhs and as rhs
    k01, k02, k12, k23, k24, k34, k45 = (_kept(0, 1, 300, 200, 1), _kept(0, 2, 300, 200, 2), _kept(1, 2, 310, 200, 3),
                                         _kept(2, 3, 320, 200, 4), _kept(2, 4, 330, 200, 5), _kept(3, 4, 340, 200, 6),
                                         _kept(4, 5, 350, 200, 7))
    out.append(case("contained_in_batch2", [k01, k02, k12, k23, k34], [k02[:6] + (8, 1), k23[:6] + (9, 1), _contains(2, 5), k24, k45],
                    [2], [k01, k34, k45]))
    # pile 4 is contained only as the rhs of a type-2 overlap (read 3's region is the longer one)
    t2 = (3, 1000, 2950, 4, 100, 2900, 5, 1)  # read 4's whole region inside read 3's: rb == 0 <= lb, r_rest == 0 <= l_rest
    out.append(case("contained_through_rhs", [k01, k24, k34[:1] + (2950 - 340, 2950) + k34[3:]], [t2, k45], [4],
                    [k01], begin=begin3, end=end3))
    # every kept overlap dies
    out.append(case("all_die", [k02, k12, k23], [k24, _contains(2, 5)], [2], []))
    # no pile is contained: the sweep keeps everything as it is
    out.append(case("none_contained", [k01, k02, k12], [k23, k34, k45], [], [k01, k02, k12, k23, k34, k45]))
    return out


# ---- identity --------------------------------------------------------------------------------------------------------
# A pair = two reads of its own: the lhs span at the tail of the lhs read's region, the rhs span at the head of the rhs
# read's (its tail on the opposite strand) — type 3, so the overlap shows in the result when the filter keeps it.

def _substitute(read, sites, m):
    out = read.copy()
    for p in sites[:m]:
        out[p] = (out[p] + 1 + (p % 3)) & 3
    return out


def _tune(rng, reads, o, begin, end, invalid, targets):
    """Substitutions inside the rhs span as OverlapUpdate leaves it, one site after the other, until the DP on the two
    scored spans says `target`, for every target (ascending).  A substitution moves the distance by at most one, so
    every value up to the distance of the fully mutated span is met.  Returns {target: rhs read}."""
    u = overlap_update(o, begin, end, invalid)
    assert u is not None
    sites = (u[4] + rng.permutation(u[5] - u[4])).tolist()
    base = reads[o[3]]

    def dist(m):
        trial = list(reads)
        trial[o[3]] = _substitute(base, sites, m)
        return edit_distance(*score_spans(u, trial))

    out, lo = {}, 0
    for target in sorted(targets):
        if target == 0:
            out[0] = base.copy()
            continue
        lo = max(lo, target - 1)  # m substitutions give a distance <= m
        assert dist(lo) < target
        hi = min(len(sites), target + target // 6 + 2)
        while dist(hi) < target:
            assert hi < len(sites)
            hi = min(len(sites), hi + target // 4 + 2)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if dist(mid) < target:
                lo = mid
            else:
                hi = mid
        assert dist(hi) == target
        out[target] = _substitute(base, sites, hi)
    return out


class _Identity:
    def __init__(self, name, identity):
        self.name, self.identity = name, identity
        self.rng = _rng("identity", name)
        self.reads, self.begin, self.end, self.invalid, self.rows, self.fates, self.pairs = [], [], [], [], [], [], []

    def _read(self, codes, region=None, invalid=0):
        self.reads.append(np.asarray(codes, dtype=np.uint8))
        self.begin.append(0 if region is None else region[0])
        self.end.append(len(codes) if region is None else region[1])
        self.invalid.append(invalid)
        return len(self.reads) - 1

    def spacer(self):
        """An invalid read: from here on the index among the valid reads differs from the id."""
        self._read(_random_read(self.rng, 40 + len(self.reads)), invalid=1)

    def geometry(self, span_l, span_r, strand, x, y, clip=0):
        """Two reads and the overlap: lhs read = x bases + the lhs span, rhs read = the rhs span + y bases (y bases + the
        span on the opposite strand).  clip > 0: the rhs region leaves out `clip` bases of the span at the read's head
        (tail), so that OverlapUpdate cuts both spans by `clip` before they are scored."""
        rng = self.rng
        lhs_read = np.concatenate([_random_read(rng, x), span_l])
        li = self._read(lhs_read)
        flank = _random_read(rng, y)
        if strand:
            rhs_read, rb = np.concatenate([span_r, flank]), 0
            region = (clip, len(rhs_read)) if clip else None
        else:
            rhs_read, rb = np.concatenate([flank, revcomp(span_r)]), y
            region = (0, len(rhs_read) - clip) if clip else None
        ri = self._read(rhs_read, region)
        return (li, x, x + len(span_l), ri, rb, rb + len(span_r), 50 + len(self.rows), strand)

    def trio(self, span, strand, x, y, clip=0):
        """Three pairs of equal spans whose scored distance is kmax - 1, kmax and kmax + 1."""
        base = _random_read(self.rng, span)
        scored = span - clip
        kmax = kmax_of(scored, self.identity)
        targets = [t for t in (kmax - 1, kmax, kmax + 1) if 0 <= t <= scored]
        # x == 0: the lhs read is its span and no more, so a pair that passes the filter is type 1 and shows in contained[lhs]
        passed = "kept" if x else "contained_lhs"
        o = self.geometry(base, base.copy(), strand, x, y, clip)
        tuned = _tune(self.rng, self.reads, o, self.begin, self.end, self.invalid, targets)
        # the pair just made serves the first target; the others get reads of their own with the same lhs span
        for j, t in enumerate(targets):
            if j:
                o = self.geometry(base, base.copy(), strand, x, y, clip)
            self.reads[o[3]] = tuned[t]
            self.rows.append(o)
            label = "%s: span %d%s strand %d x %d: distance kmax%+d = %d" % (self.name, span, " clipped by %d" % clip if clip else "",
                                                                           strand, x, t - kmax, t)
            self.fates.append((label, passed if t <= kmax else "dropped", o[0], o[3]))
            self.pairs.append(dict(overlap=o, distance=t, kmax=kmax, maxlen=scored))

    def by_length(self, span, strand, x, y, rhs_longer):
        """Pairs whose spans differ in length by kmax, kmax + 1 and more: one span is the other without its last bases,
        so the distance is the difference.  rhs_longer: max(length) comes from the rhs."""
        base = _random_read(self.rng, span)
        kmax = kmax_of(span, self.identity)
        for d in (kmax, kmax + 1, kmax + 5):
            if span - d < 84:
                continue
            short = base[:span - d].copy()
            o = self.geometry(short, base.copy(), strand, x, y) if rhs_longer else self.geometry(base, short, strand, x, y)
            self.rows.append(o)
            label = "%s: spans %d and %d (%s longer) strand %d: distance %d, kmax %d" % (
                self.name, span, span - d, "rhs" if rhs_longer else "lhs", strand, d, kmax)
            self.fates.append((label, "kept" if d <= kmax else "dropped", o[0], o[3]))
            self.pairs.append(dict(overlap=o, distance=d, kmax=kmax, maxlen=span))

    def case(self):
        self.spacer()
        n_valid = len(self.reads) - sum(self.invalid)
        return _case("identity:" + self.name, "identity", self.reads, self.begin, self.end, self.invalid,
                     _one_batch(n_valid, self.rows), identity=self.identity,
                     claims=dict(fates=self.fates, pairs=self.pairs))


@functools.lru_cache(maxsize=None)
def _identity_cases():
    out = []
    begins = (31, 32, 33, 64)
    for ii, identity in enumerate(IDENTITIES):
        for si, span in enumerate(SPANS):
            g = _Identity("%g:%d" % (identity, span), identity)
            strand = (ii + si) & 1
            g.trio(span, strand, begins[(ii + si) % 4], 20 + si)
            g.spacer()
            if span <= 500:
                g.trio(span, 1 - strand, begins[(ii + si + 1) % 4], 33)
            out.append(g.case())
    for identity in (0.78, 0.9):
        g = _Identity("%g:lengths" % identity, identity)
        g.by_length(300, 1, 32, 20, rhs_longer=False)
        g.spacer()
        g.by_length(300, 0, 33, 31, rhs_longer=True)
        g.by_length(129, 1, 31, 32, rhs_longer=True)
        g.spacer()
        g.by_length(500, 0, 64, 20, rhs_longer=False)
        out.append(g.case())
    g = _Identity("0.78:begin0", 0.78)  # the lhs span begins at base 0 of its read
    g.trio(128, 1, 0, 40)
    g.spacer()
    g.trio(129, 0, 0, 33)
    out.append(g.case())
    for identity in (0.8, 1.0):
        g = _Identity("%g:clipped" % identity, identity)
        g.trio(200, 1, 32, 40, clip=16)
        g.spacer()
        g.trio(129 + 45, 0, 31, 40, clip=45)
        g.trio(84 + 7, 1, 33, 25, clip=7)  # exactly 84 bases are scored
        out.append(g.case())
    return out


def identity_lists(case, layout):
    """The overlaps of an identity case as per-pile lists (CSR by lhs), for the filter of ResolveContainedReads; layout
    "plain", or "gaps": three more piles without a list — one in front of all reads, one in the middle, one behind."""
    rows = [tuple(int(v) for v in o) for b in case["batches"] for e in b["maps"] for o in np.asarray(e[1]).tolist()]
    reads, begin, end, invalid = list(case["reads"]), case["begin"].tolist(), case["end"].tolist(), case["invalid"].tolist()
    if layout == "gaps":
        n = len(reads)
        mid = n // 2
        old = list(range(n))
        new = [i + 1 + (i >= mid) for i in old]  # a new pile at 0, at mid + 1, at the end
        rng = _rng("gaps", case["name"])
        reads2, begin2, end2, invalid2 = [], [], [], []
        for i in range(n + 3):
            if i in new:
                j = new.index(i)
                reads2.append(reads[j]), begin2.append(begin[j]), end2.append(end[j]), invalid2.append(invalid[j])
            else:
                reads2.append(_random_read(rng, 120)), begin2.append(0), end2.append(112), invalid2.append(0)
        rows = [(new[o[0]],) + o[1:3] + (new[o[3]],) + o[4:] for o in rows]
        reads, begin, end, invalid = reads2, begin2, end2, invalid2
    n = len(reads)
    off = np.zeros(n + 1, dtype=np.uint32)
    for o in rows:
        off[o[0] + 1] += 1
    off = np.cumsum(off).astype(np.uint32)
    rows.sort(key=lambda o: o[0])  # (stable: the order inside a pile stays)
    return dict(reads=reads, begin=np.array(begin, np.uint32), end=np.array(end, np.uint32),
                invalid=np.array(invalid, np.uint8), overlaps=_ovl(rows), offsets=off)


# ---- kmers -----------------------------------------------------------------------------------------------------------

def _expand(s, k):
    """`s` with its first characters doubled (the first one taking the rest), k characters in all: the same runs."""
    extra = k - len(s)
    assert extra >= 0
    out = []
    for i, c in enumerate(s):
        rep = 1 + (1 if i < extra else 0) + (max(0, extra - len(s)) if i == 0 else 0)
        out.append(c * rep)
    out = "".join(out)
    assert len(out) == k and lc_stages(out)[0] == lc_stages(s)[0]
    return out


def _lc_kmers(k):
    """(k-mer, stage at which pile.cc rejects it or None, label) with need = k / 2 + 1 characters."""
    need = k // 2 + 1
    unit = "ACGTCAGT"  # no stage removes anything from its repetitions
    full = (unit * 8)[:need + 2]
    assert [len(s) for s in lc_stages(full)] == [need + 2] * 3
    out = [("A" * k, 1, "homopolymer"), (("AC" * k)[:k], 2, "dinucleotide"), (("ACG" * k)[:k], None, "unit of 3"),
           (("ACGT" * k)[:k], None, "unit of 4"),
           (_expand(full[:need], k), None, "need left after stage 1"), (_expand(full[:need - 1], k), 1, "need - 1 after stage 1"),
           # AC AC in front: stage 2 takes one pair away
           (_expand("AC" + full[:need], k), None, "need left after stage 2"),
           (_expand("AC" + full[:need - 1], k), 2, "need - 1 after stage 2"),
           # T ACAC ...: the pairs of stage 2 are TA CA C., those of stage 3 T AC AC — only stage 3 takes a pair away
           (_expand("TAC" + full[:need - 1], k), None, "need left after stage 3"),
           (_expand("TAC" + full[:need - 2], k), 3, "need - 1 after stage 3"),
           (_expand("TACACGTGTACAC", k) if k == 15 else _expand("T" + "ACACGTGT" * 3 + "ACAC", k), 3,
            "stage 3 alone")]
    for kmer, stage, label in out:
        lens = [len(s) for s in lc_stages(kmer)]
        fails = [i + 1 for i, n in enumerate(lens) if n < need]
        assert len(kmer) == k and (fails[0] if fails else None) == stage, (kmer, lens, stage, label)
        if "left after" in label:
            assert lens[int(label[-1]) - 1] == need, (kmer, lens, label)
        if "- 1 after" in label:
            assert lens[int(label[-1]) - 1] == need - 1, (kmer, lens, label)
    return out


def _plant(read, pos, kmer):
    read[pos:pos + len(kmer)] = np.array(["ACGT".index(c) for c in kmer], dtype=np.uint8)


def _kmers_case(k):
    rng = _rng("kmers", k)
    reads, maps, marked, unmarked = [], [], [], []

    def complex_read(n, positions=()):
        """A random read whose k-mers at `positions` pass the low-complexity test."""
        while True:
            r = _random_read(rng, n)
            s = inflate(r)
            if all(lc_passes(s[p:p + k], k) for p in positions):
                return r

    def add(read, filtered=None, other=None):
        reads.append(read)
        rid = len(reads) - 1
        if filtered is not None or other is not None:
            maps.append((rid, np.zeros(0, DT), np.array(sorted(filtered or []), np.uint32), np.array(sorted(other or []), np.uint32)))
        return rid

    add(complex_read(200))                                   # 0: no minimizer at all, in front
    add(complex_read(333), other=[3, 40, 100, 333 - k])          # 1: minimizers, none filtered
    # 2: positions 0, 16 c - 1, 16 c, one whose k-mer straddles bit 64 of the packed words, two in one cell, len - k with
    # len = 16 m + 15 (cell len >> 4, the extra one, at k = 15)
    n2 = 16 * 20 + 15
    straddle = 32 - k // 2
    pos2 = [0, 47, 48, straddle, 100, 101, n2 - k]
    r2 = add(complex_read(n2, pos2), filtered=pos2, other=[7, 64, 200])
    marked += [(r2, p >> PSS) for p in pos2]
    unmarked += [(r2, 64 >> PSS), (r2, 200 >> PSS)]
    assert 2 * straddle < 64 < 2 * (straddle + k) and (k != 15 or (n2 - k) >> PSS == n2 >> PSS)
    invalid_at = len(reads)
    add(complex_read(150))                                   # 3: INVALID (ids and valid indices part here)
    add(complex_read(90))                                    # 4, 5: no minimizers, several in a row, in the middle
    add(complex_read(17))                                    # (too short for any)
    # 6: the low-complexity k-mers, each in a cell of its own
    lc = _lc_kmers(k)
    n6 = 64 + 64 * len(lc)
    r6read = complex_read(n6)
    pos6 = []
    for i, (kmer, stage, label) in enumerate(lc):
        p = 48 + 64 * i + (i % 3)
        _plant(r6read, p, kmer)
        pos6.append(p)
    r6 = add(r6read, filtered=pos6, other=[10])
    for p, (kmer, stage, label) in zip(pos6, lc):
        (marked if stage is None else unmarked).append((r6, p >> PSS))
    add(complex_read(64), other=[5, 30])                     # 7: not filtered
    p8 = 16 * 6 if k == 15 else 16 * 8 - k
    r8 = add(complex_read(p8 + k, [p8]), filtered=[p8])  # 8: the last position of the read
    marked.append((r8, p8 >> PSS))
    add(complex_read(70))                                    # 9: no minimizer, behind
    n = len(reads)
    invalid = [1 if i == invalid_at else 0 for i in range(n)]
    nv = n - 1
    begin, end = [0] * n, [(len(r) >> 4) << 4 for r in reads]
    valid = [i for i in range(n) if not invalid[i]]

    def batch(qf, ql):
        return dict(q_first=qf, q_last=ql, maps=[m for m in maps if qf <= valid.index(m[0]) < ql])

    claims = dict(marked=marked, unmarked=unmarked, lc=lc)
    out = [_case("kmers:k%d" % k, "kmers", reads, begin, end, invalid, [batch(0, nv)], kmer_len=k, claims=claims)]
    # the device group's form: query ranges that do not start at 0, one after the other
    out.append(_case("kmers:k%d:q_first>0" % k, "kmers", reads, begin, end, invalid,
                     [batch(2, 3), batch(0, 2), batch(3, nv - 1), batch(nv - 1, nv)], kmer_len=k,
                     claims=dict(claims, q_first=[2, 0, 3, nv - 1])))
    return out


# ---- subset ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _subset_reads():
    """Reads of 1 to 3 kb cut from a genome of 30 kb with a planted repeat (1.5 kb, 4 copies), both strands, ~2 % errors,
    and among them reads of 0, 1, 31, 32, 33, 64 and k + w - 2 bases."""
    rng = _rng("subset")
    g = _random_read(rng, 30_000)
    for c in range(1, 4):
        g[1000 + c * 7000:2500 + c * 7000] = g[1000:2500]
    reads = []
    tiny = [0, 1, 31, 32, 33, 64, 15 + W - 2]
    while sum(len(r) for r in reads) < 8 * g.shape[0]:
        n = int(rng.integers(1000, 3001))
        at = int(rng.integers(0, g.shape[0] - n + 1))
        r = g[at:at + n].copy()
        sub = rng.random(n) < 0.02
        r[sub] = (r[sub] + rng.integers(1, 4, size=int(sub.sum()))) & 3
        r = r[rng.random(n) >= 0.005]
        reads.append(revcomp(r) if rng.random() < 0.5 else r)
        if len(reads) % 12 == 3 and tiny:
            reads.append(_random_read(rng, tiny.pop(0)))
    assert not tiny
    return reads


def _subset_cases():
    reads = _subset_reads()
    n = len(reads)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    begin, end = np.zeros(n, np.uint32), ((lens >> 4) << 4).astype(np.uint32)
    tiny_ids = [i for i in range(n) if lens[i] <= 64]
    rng = _rng("subset", "validity")
    some = (rng.random(n) < 0.2).astype(np.uint8)
    some[tiny_ids] = 0  # the tiny reads stay valid

    def case(name, invalid, batch_bases, **claims):
        invalid = np.asarray(invalid, dtype=np.uint8)
        return _case("subset:" + name, "subset", reads, begin, end, invalid, [], claims=claims, batch_bases=int(batch_bases),
                     freq=0.01)

    first = some.copy()
    first[0], first[n - 1] = 1, 0
    last = some.copy()
    last[0], last[n - 1] = 0, 1
    one = np.zeros(n, np.uint8)
    one[n // 2] = 1
    valid_bases = int(lens[some == 0].sum())
    # the last index batch is one read: every base but the last valid read's fills the first batch exactly
    last_valid = int(np.flatnonzero(some == 0)[-1])
    busy = dict(overlaps=True, contained=True, cells=True)
    return [
        case("first_invalid", first, 1 << 30, **busy),
        case("last_invalid", last, 1 << 30, **busy),
        case("alternating", np.arange(n) % 2, 1 << 30, overlaps=True, cells=True),
        case("one_invalid", one, 1 << 30, **busy),
        case("all_invalid", np.ones(n, np.uint8), 1 << 30, empty=True),
        case("one_read_batches", some, 1, overlaps=True, contained=True),  # (an index of one read filters nothing)
        case("last_batch_one_read", some, valid_bases - int(lens[last_valid]), last_batch=1, **busy),
        case("three_batches", some, valid_bases // 3 + 1, **busy),
    ]


# ---- all of them -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cases():
    out = _rules_cases() + _dedup_cases() + _finish_cases() + list(_identity_cases()) + _kmers_case(15) + _kmers_case(31)
    out += _subset_cases()
    assert len({c["name"] for c in out}) == len(out)
    return out


def names(*families):
    return [c["name"] for c in cases() if not families or c["family"] in families]


def by_name(name):
    for c in cases():
        if c["name"] == name:
            return c
    raise KeyError(name)


def fate_of(state, lhs, rhs):
    """What became of the one overlap of the piles (lhs, rhs) in a result."""
    o = state["overlaps"]
    kept = bool(np.any((o["lhs_id"] == lhs) & (o["rhs_id"] == rhs)))
    cl, cr = bool(state["contained"][lhs]), bool(state["contained"][rhs])
    assert kept + cl + cr <= 1
    return "kept" if kept else "contained_lhs" if cl else "contained_rhs" if cr else "dropped"


def check_claims(case, state):
    """Every claim of a case against a result (the reference's, in tests/test_pass2_cases.py); returns how many it checked."""
    claims, n = case["claims"], 0
    for label, fate, lhs, rhs in claims.get("fates", []):
        assert fate_of(state, lhs, rhs) == fate, "%s: %s, claimed %s" % (label, fate_of(state, lhs, rhs), fate)
        n += 1
    if "result" in claims:
        assert np.array_equal(state["overlaps"], claims["result"]), "%s: the list is not the one claimed" % case["name"]
        assert np.flatnonzero(state["contained"]).tolist() == claims["contained"], case["name"]
        n += 1
    off = state["kmers_offsets"].astype(np.int64)
    for rid, cell in claims.get("marked", []):
        assert state["kmers"][off[rid] + cell] == 1, "cell %d of read %d is not marked" % (cell, rid)
        n += 1
    for rid, cell in claims.get("unmarked", []):
        assert state["kmers"][off[rid] + cell] == 0, "cell %d of read %d is marked" % (cell, rid)
        n += 1
    if "marked" in claims:
        assert int(state["kmers"].sum()) == len(set(claims["marked"]))
    if claims.get("overlaps"):
        assert state["overlaps"].shape[0] > 0
        n += 1
    if claims.get("contained") is True:
        assert state["contained"].any()
        n += 1
    if claims.get("cells"):
        assert state["kmers"].any()
        n += 1
    if claims.get("empty"):
        assert state["overlaps"].shape[0] == 0 and not state["contained"].any() and state["kmers"].shape[0] == 0
        n += 1
    return n
