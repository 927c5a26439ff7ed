"""The window-layer stage of a polishing round (raven_amd/csrc/polish.hip: layer_count_kernel, layer_fill_kernel,
window_finish_kernel, layer_quality_kernel, count_flags_kernel, stitch_kernel and the host planning around them) on
crafted best-overlap tables: a plain reference of the stage and the cases, each tagged with the class it stands for.

layers_from_best() is racon's bookkeeping between an overlap and its window layers written out in Python on top of
oracle.nw_breakpoints (the alignment path and its breakpoints, pinned elsewhere); best_from_oracle() is racon's choice of
one overlap per read on top of the oracle's Map.  Together they restate oracle.polish_layers (tests/test_layer_cases.py
holds them to it), and layers_from_best alone is the reference of a round whose table the test dictates through
Engine.polish_set_best.

cases() returns a list of dicts:
  name          the case; one case is one round
  tags          the classes of TAGS the case stands for
  targets       ReadSet (its ids need not be 0 .. n - 1), reads: ReadSet
  quals         None, or one uint8 Phred+33 array per read in the read's own orientation (what the reference sees)
  blocks        None, or the same qualities as one byte per 64 bases for Reads.attach_quality(blocks, block_shift=6)
                (quals is then their per-base expansion)
  best, best_t  the best-overlap table: OVERLAP_DTYPE[n_reads] and uint32[n_reads] (0xFFFFFFFF = the read is unused)
  w, q          window length and quality threshold of the round
  present       rows {window, read, first base, bases, begin, end, rc} the table has BY CONSTRUCTION
  absent        (window, read) pairs that have no row by construction
tests/test_layer_cases.py asserts every such claim, and what each tag promises, of the reference's output on the CPU;
tests/test_gpu_polish_layers.py runs the rounds on the device.  Nothing here looks at what the code under test returns."""
import numpy as np

from oracle import oracle
from raven_amd import seqio
from raven_amd.synth import mutate

UNUSED = 0xFFFFFFFF
TAGS = ("len_9", "len_10", "empty_window", "one_pair", "short_tail", "q_exact", "q_oriented", "q_blocks", "ties_130",
        "ties_interleaved", "unused_and_degenerate", "multi_target")


# ---- the reference ---------------------------------------------------------------------------------------------------

def revcomp(codes):
    return (3 - np.asarray(codes, dtype=np.uint8)[::-1]).astype(np.uint8)


def first_windows(targets, w):
    """Global number of every target's first window (and, last, the number of windows)."""
    fw = np.zeros(targets.n + 1, dtype=np.int64)
    np.cumsum((targets.lengths.astype(np.int64) + w - 1) // w, out=fw[1:])
    return fw


def oriented(reads, r, rc, quals=None):
    """Read r (and its qualities) in the orientation it is aligned in."""
    codes = reads.codes(r)
    qual = None if quals is None else np.asarray(quals[r], dtype=np.uint8)
    if rc:
        codes = revcomp(codes)
        qual = None if qual is None else qual[::-1]
    return codes, qual


def layers_from_best(targets, reads, best, best_t, quals=None, q=0.0, w=500):
    """racon's window layers of a round whose best-overlap table is given: uint32[n, 7] rows {window, read, first base
    in the oriented read, bases, begin, end, rc}, sorted by (window, begin, read)."""
    fw = first_windows(targets, w)
    t_codes = [targets.codes(t) for t in range(targets.n)]
    rows = []
    for r in range(reads.n):
        if int(best_t[r]) == UNUSED:
            continue
        o, t = best[r], int(best_t[r])
        if int(o["rhs_end"]) <= int(o["rhs_begin"]) or int(o["lhs_end"]) <= int(o["lhs_begin"]):
            continue  # an empty span has no aligned pair, hence no breakpoint
        qlen = int(reads.lengths[r])
        rc = int(o["strand"]) == 0
        codes, qual = oriented(reads, r, rc, quals)
        q_begin = qlen - int(o["lhs_end"]) if rc else int(o["lhs_begin"])
        q_end = qlen - int(o["lhs_begin"]) if rc else int(o["lhs_end"])
        t_begin, t_end = int(o["rhs_begin"]), int(o["rhs_end"])
        bp, _ = oracle.nw_breakpoints(codes[q_begin:q_end], t_codes[t][t_begin:t_end], q_begin, t_begin, w)
        for j in range(0, len(bp) - 1, 2):
            (first_t, first_q), (last_t, last_q) = (int(x) for x in bp[j]), (int(x) for x in bp[j + 1])
            bases = last_q - first_q
            if bases < 0.02 * w:
                continue
            if qual is not None and float(np.sum(qual[first_q:last_q].astype(np.int64) - 33)) / bases < q:
                continue
            ws = (first_t // w) * w
            begin, end = first_t - ws, last_t - ws - 1
            if begin >= end:
                continue
            backbone = min(w, int(targets.lengths[t]) - ws)
            rows.append((int(fw[t]) + first_t // w, r, first_q, bases, begin, min(end, backbone - 1), 1 if rc else 0))
    rows.sort(key=lambda x: (x[0], x[4], x[1]))
    return np.asarray(rows, dtype=np.uint32).reshape(-1, 7)


def best_from_oracle(targets, reads, err=0.3):
    """racon's best overlap per read from the oracle's Map of every read against the targets: (OVERLAP_DTYPE[n], uint32[n])."""
    eng = oracle.Engine(15, 5)
    eng.minimize(targets)
    eng.filter(0.001)
    id_to_t = {int(i): t for t, i in enumerate(targets.ids)}
    best = np.zeros(reads.n, dtype=oracle.OVERLAP_DTYPE)
    best_t = np.full(reads.n, UNUSED, dtype=np.uint32)

    def span(o):
        return max(int(o["lhs_end"]) - int(o["lhs_begin"]), int(o["rhs_end"]) - int(o["rhs_begin"]))

    for r in range(reads.n):
        ovl = eng.map(reads, r, avoid_equal=False, avoid_symmetric=False)["overlaps"]
        if ovl.shape[0] == 0:
            continue
        b = ovl[0]
        for o in ovl[1:]:
            if span(b) < span(o):
                b = o
        best[r] = b
        a, c = float(int(b["lhs_end"]) - int(b["lhs_begin"])), float(int(b["rhs_end"]) - int(b["rhs_begin"]))
        if 1.0 - min(a, c) / max(a, c) > err:
            continue
        best_t[r] = id_to_t.get(int(b["rhs_id"]), UNUSED)
    return best, best_t


def counts(case, table):
    """What the round's statistics must say, from the reference table: dict(n_layers, n_reads_used, n_windows) and, per
    target, the windows and the polished windows (racon: a window of fewer than three sequences stays as it is, i.e. a
    window is polished iff at least two layers beside the backbone survive)."""
    fw = first_windows(case["targets"], case["w"])
    per_window = np.bincount(table[:, 0].astype(np.int64), minlength=int(fw[-1]))
    polished = [int((per_window[fw[t]:fw[t + 1]] >= 2).sum()) for t in range(case["targets"].n)]
    return dict(n_layers=int(table.shape[0]), n_reads_used=int((case["best_t"] != UNUSED).sum()), n_windows=int(fw[-1]),
                windows=[int(fw[t + 1] - fw[t]) for t in range(case["targets"].n)], polished=polished)


def reference_consensus(case, table, trim=True):
    """The round's consensus from the reference table: oracle.poa_window of every window's backbone and layers, stitched
    per target.  Returns (list of code arrays, polished windows per target)."""
    targets, reads, quals, w = case["targets"], case["reads"], case["quals"], case["w"]
    fw = first_windows(targets, w)
    by_window = {}
    for row in table:
        by_window.setdefault(int(row[0]), []).append(row)
    out, polished = [], []
    for t in range(targets.n):
        tc = targets.codes(t)
        parts, n_pol = [], 0
        for k in range(int(fw[t + 1] - fw[t])):
            bb = tc[k * w:(k + 1) * w]
            layers, begins, ends, lq = [bb], [0], [len(bb) - 1], [np.full(len(bb), 33, dtype=np.uint8)]
            for _, r, fq, n, b, e, rc in by_window.get(int(fw[t]) + k, []):
                codes, qual = oriented(reads, int(r), bool(rc), quals)
                layers.append(codes[int(fq):int(fq) + int(n)])
                begins.append(int(b))
                ends.append(int(e))
                lq.append(None if qual is None else qual[int(fq):int(fq) + int(n)])
            cons, pol = oracle.poa_window(layers, begins, ends, None if quals is None else lq, trim=trim)
            parts.append(cons)
            n_pol += int(pol)
        out.append(np.concatenate(parts) if parts else np.zeros(0, np.uint8))
        polished.append(n_pol)
    return out, polished


# ---- the cases -------------------------------------------------------------------------------------------------------

def _seq(seed, n):
    return np.random.default_rng(seed).integers(0, 4, size=n, dtype=np.uint8)


def _overlap(r, read_len, q_begin, q_end, rc, t_id, t_begin, t_end):
    """The overlap record of read r whose span [q_begin, q_end) IN THE ORIENTATION IT IS ALIGNED IN goes to
    [t_begin, t_end) of the target with id t_id: lhs positions are those of the read as it is stored."""
    o = np.zeros(1, dtype=oracle.OVERLAP_DTYPE)[0]
    o["lhs_id"], o["rhs_id"], o["rhs_begin"], o["rhs_end"] = r, t_id, t_begin, t_end
    o["lhs_begin"], o["lhs_end"] = (read_len - q_end, read_len - q_begin) if rc else (q_begin, q_end)
    o["score"], o["strand"] = min(q_end - q_begin, t_end - t_begin), 0 if rc else 1
    return o


class _Round:
    """Collects the reads of one round."""

    def __init__(self, name, tags, targets, w=500, q=0.0, target_ids=None):
        self.name, self.tags, self.w, self.q = name, set(tags), w, q
        self.targets = [np.asarray(t, dtype=np.uint8) for t in targets]
        self.ids = list(range(len(targets))) if target_ids is None else list(target_ids)
        self.reads, self.best, self.best_t, self.quals = [], [], [], []
        self.present, self.absent, self.blocks = [], [], None

    def add(self, t, t_begin, t_end, rc, left=0, right=0, codes=None, qual=None):
        """A read = target t's span [t_begin - left, t_end + right) (or `codes`, which stands for that span) stored on the
        strand `rc` says, overlapping [t_begin, t_end) with all but its `left` first and `right` last oriented bases."""
        if codes is None:
            codes = self.targets[t][t_begin - left:t_end + right]
        n = len(codes)
        r = len(self.reads)
        self.reads.append(revcomp(codes) if rc else np.asarray(codes, dtype=np.uint8))
        self.best.append(_overlap(r, n, left, n - right, rc, self.ids[t], t_begin, t_end))
        self.best_t.append(t)
        if qual is not None:  # given in the ALIGNED orientation; stored in the read's own
            qual = np.asarray(qual, dtype=np.uint8)
            self.quals.append(qual[::-1].copy() if rc else qual)
        return r

    def add_raw(self, codes, overlap, target):
        r = len(self.reads)
        self.reads.append(np.asarray(codes, dtype=np.uint8))
        overlap["lhs_id"] = r
        self.best.append(overlap)
        self.best_t.append(target)
        return r

    def case(self):
        assert not self.quals or len(self.quals) == len(self.reads)
        best = np.zeros(len(self.best), dtype=oracle.OVERLAP_DTYPE)
        for i, o in enumerate(self.best):
            best[i] = o
        return dict(name=self.name, tags=self.tags, targets=seqio.pack_reads(self.targets, ids=self.ids),
                    reads=seqio.pack_reads(self.reads), quals=self.quals or None, blocks=self.blocks,
                    best=best, best_t=np.asarray(self.best_t, dtype=np.uint32),
                    w=self.w, q=self.q, present=self.present, absent=self.absent)


def _len_rule():
    """racon: a piece of fewer than 0.02 * w = 10 bases is no layer.  Overlap [491, 1009): 9 bases in the first and the
    last window; [490, 1010): 10 bases, layers (490, 499) and (0, 9).  Both strands; the reads reach beyond the overlap
    by different amounts on the two sides, so that a read addressed on the wrong strand gives other rows."""
    out = []
    for tag, a, b in (("len_9", 491, 1009), ("len_10", 490, 1010)):
        R = _Round(tag, [tag], [_seq(11, 1500)])
        for rc in (False, True):
            r = R.add(0, a, b, rc, left=41, right=91)
            R.present.append((1, r, 41 + 500 - a, 500, 0, 499, int(rc)))
            if tag == "len_9":
                R.absent += [(0, r), (2, r)]
            else:
                R.present += [(0, r, 41, 10, 490, 499, int(rc)), (2, r, 41 + 510, 10, 0, 9, int(rc))]
        out.append(R.case())
    return out


def _empty_window():
    """Target = P + L + A x 1040 + R + S, read = L + R with L ending and R beginning in a base other than A: the read's
    span starts at target position 100 and crosses windows 1 and 2 with deletions only, so their records carry no
    aligned pair (first_t == ~0).  Windows 0 and 3 get (100, 479) and (20, 399).  Both strands."""
    rng = np.random.default_rng(12)
    P, L, Rr, S = (rng.integers(0, 4, size=n, dtype=np.uint8) for n in (100, 380, 380, 100))
    L[-1], Rr[0] = 1, 2
    target = np.concatenate([P, L, np.zeros(1040, np.uint8), Rr, S])
    R = _Round("empty_window", ["empty_window"], [target])
    for rc in (False, True):
        r = R.add(0, 100, 1900, rc, codes=np.concatenate([L, Rr]))
        R.present += [(0, r, 0, 380, 100, 479, int(rc)), (3, r, 380, 380, 20, 399, int(rc))]
        R.absent += [(1, r), (2, r)]
    return [R.case()]


def _one_pair():
    """w = 50, where 0.02 * w = 1 and the length rule lets a piece of one base through: overlap [10, 101) leaves one
    aligned pair in window 2, begin = end = 0, which only racon's `begin >= end` rejects; [10, 102) gives (0, 1)."""
    R = _Round("one_pair", ["one_pair"], [_seq(13, 150)], w=50)
    for rc in (False, True):
        r = R.add(0, 10, 101, rc, left=3, right=5)
        R.present += [(0, r, 3, 40, 10, 49, int(rc)), (1, r, 43, 50, 0, 49, int(rc))]
        R.absent.append((2, r))
        r = R.add(0, 10, 102, rc, left=3, right=5)
        R.present.append((2, r, 93, 2, 0, 1, int(rc)))
    return [R.case()]


def _short_tail():
    """The last window of a target: 3 bases (2003 at w = 50 and at w = 500), 12 bases (2012), none extra (a multiple of
    w), one base (w * k + 1: a backbone of one base can hold no layer, begin = end = 0).  Reads run to the target's end."""
    out = []
    R = _Round("short_tail_w50", ["short_tail"], [_seq(14, 2003), _seq(15, 100), _seq(16, 151)], w=50)
    for rc in (False, True):
        r = R.add(0, 1930, 2003, rc, left=2)
        R.present += [(38, r, 2, 20, 30, 49, int(rc)), (39, r, 22, 50, 0, 49, int(rc)), (40, r, 72, 3, 0, 2, int(rc))]
        r = R.add(1, 40, 100, rc, left=4)
        R.present += [(41, r, 4, 10, 40, 49, int(rc)), (42, r, 14, 50, 0, 49, int(rc))]
        r = R.add(2, 60, 151, rc, left=1)
        R.present += [(44, r, 1, 40, 10, 49, int(rc)), (45, r, 41, 50, 0, 49, int(rc))]
        R.absent.append((46, r))
    out.append(R.case())
    R = _Round("short_tail_w500", ["short_tail"], [_seq(14, 2003), _seq(17, 2012), _seq(18, 1000), _seq(19, 1001)])
    for rc in (False, True):
        r = R.add(0, 1400, 2003, rc, left=7)
        R.present += [(2, r, 7, 100, 400, 499, int(rc)), (3, r, 107, 500, 0, 499, int(rc))]
        R.absent.append((4, r))  # 3 bases < 10
        r = R.add(1, 1400, 2012, rc, left=7)
        R.present += [(8, r, 107, 500, 0, 499, int(rc)), (9, r, 607, 12, 0, 11, int(rc))]
        r = R.add(2, 400, 1000, rc, left=7)
        R.present += [(10, r, 7, 100, 400, 499, int(rc)), (11, r, 107, 500, 0, 499, int(rc))]
        r = R.add(3, 400, 1001, rc, left=7)
        R.present.append((13, r, 107, 500, 0, 499, int(rc)))
        R.absent.append((14, r))
    out.append(R.case())
    return out


def _q_exact():
    """racon: a piece whose mean Phred is below q is no layer, `mean >= q` keeps it.  520 bases over [490, 1010), every
    quality 33 + 10, q = 10.0: three layers.  The same read with ONE quality byte of its first piece (aligned position 3)
    lowered by one has mean 9.9 there: that piece alone goes.  Both strands."""
    R = _Round("q_exact", ["q_exact"], [_seq(20, 1500)], q=10.0)
    for rc in (False, True):
        qual = np.full(520, 43, dtype=np.uint8)
        r = R.add(0, 490, 1010, rc, qual=qual)
        R.present += [(0, r, 0, 10, 490, 499, int(rc)), (1, r, 10, 500, 0, 499, int(rc)), (2, r, 510, 10, 0, 9, int(rc))]
        low = qual.copy()
        low[3] -= 1
        r = R.add(0, 490, 1010, rc, qual=low)
        R.present += [(1, r, 10, 500, 0, 499, int(rc)), (2, r, 510, 10, 0, 9, int(rc))]
        R.absent.append((0, r))
    return [R.case()]


def _q_oriented():
    """A reverse-strand read of 1000 bases over [250, 1250) whose STORED qualities are 5 over its first half and 20 over
    its second: aligned, the pieces of windows 0 / 1 / 2 have means 20 / 12.5 / 5, and q = 15 keeps window 0 alone.  Read
    in the stored orientation the means are 5 / 12.5 / 20 and window 2 alone would stay.  A forward read with the same
    stored bytes beside it keeps window 2."""
    R = _Round("q_oriented", ["q_oriented"], [_seq(21, 1500)], q=15.0)
    stored = np.concatenate([np.full(500, 33 + 5, np.uint8), np.full(500, 33 + 20, np.uint8)])
    r = R.add(0, 250, 1250, True, qual=stored[::-1])
    R.present.append((0, r, 0, 250, 250, 499, 1))
    R.absent += [(1, r), (2, r)]
    r = R.add(0, 250, 1250, False, qual=stored)
    R.present.append((2, r, 750, 250, 0, 249, 0))
    R.absent += [(0, r), (1, r)]
    return [R.case()]


def _q_blocks():
    """The same rule on block qualities (one byte per 64 bases, Reads.attach_quality(blocks, block_shift=6)): reads of
    1000 bases, so the last block holds 40; pieces begin and end inside a block; both strands; block values 3 .. 19 and
    q = 11 so that some pieces go and some stay.  The reference sees the per-base expansion."""
    rng = np.random.default_rng(22)
    R = _Round("q_blocks", ["q_blocks"], [_seq(23, 2000)], q=11.0)
    blocks = []
    for i in range(8):
        left, right = 30 + 7 * i, 10 + 3 * i
        t_begin = 270 + 90 * i
        b = (rng.integers(3, 20, size=16) + 33).astype(np.uint8)
        stored = np.repeat(b, 64)[:1000]
        rc = bool(i & 1)
        R.add(0, t_begin, t_begin + 1000 - left - right, rc, left=left, right=right, qual=stored[::-1] if rc else stored)
        blocks.append(b)
    R.blocks = blocks
    return [R.case()]


def _ties():
    """window_finish_kernel ranks a window's layers by (begin, job) in trips of 64 lanes.  ties_130: 130 copies of one
    read over [250, 750), both windows get 130 layers of equal begin in read order (three trips).  ties_interleaved: 130
    reads whose begin in window 0 takes five values that cycle over the read indices, strands mixed: sorted by job alone
    or by begin alone (ties in any other order) the table is another."""
    t = _seq(24, 1000)
    R = _Round("ties_130", ["ties_130"], [t])
    for r in range(130):
        R.add(0, 250, 750, False)
        R.present += [(0, r, 0, 250, 250, 499, 0), (1, r, 250, 250, 0, 249, 0)]
    S = _Round("ties_interleaved", ["ties_interleaved"], [t])
    for r in range(130):
        a = 240 + 7 * ((3 * r) % 5)
        rc = r % 3 == 1
        S.add(0, a, 760, rc, left=r % 4)
        S.present += [(0, r, r % 4, 500 - a, a, 499, int(rc)), (1, r, r % 4 + 500 - a, 260, 0, 259, int(rc))]
    return [R.case(), S.case()]


def _unused_and_degenerate():
    """Unused reads (best_t = ~0, their overlap records full of values that must not be looked at) between used ones; a
    read whose overlap has rhs_end == rhs_begin and one with lhs_end == lhs_begin (no job, no layer, but a used read of
    n_reads_used); windows 1 and 3 without a layer between windows 0, 2 and 4 that have some."""
    R = _Round("unused_and_degenerate", ["unused_and_degenerate"], [_seq(25, 2500)])
    junk = np.zeros(1, dtype=oracle.OVERLAP_DTYPE)[0]
    for f in ("lhs_begin", "lhs_end", "rhs_id", "rhs_begin", "rhs_end"):
        junk[f] = 0xFFFFFFF0
    for k, a in enumerate((50, 1050, 2050)):
        for rc in (False, True):
            r = R.add(0, a, a + 400, rc, left=5, right=9)
            R.present.append((2 * k, r, 5, 400, 50, 449, int(rc)))
        R.add_raw(_seq(30 + k, 300), junk.copy(), UNUSED)
        if k == 0:
            o = _overlap(0, 300, 0, 100, False, 0, 700, 700)
        else:
            o = _overlap(0, 300, 100, 100, k == 1, 0, 1600, 1700)
        r = R.add_raw(_seq(40 + k, 300), o, 0)
        R.absent += [(w, r) for w in range(5)]
    return [R.case()]


def _multi_target():
    """Three targets of 1203, 700 and 1500 bases (3 + 2 + 3 windows) with ids 7, 3 and 12; reads with planted edits to each
    of them in an order that mixes the targets, both strands: a layer's window is first_window[target] + its window in
    the target."""
    rng = np.random.default_rng(26)
    targets = [_seq(27, 1203), _seq(28, 700), _seq(29, 1500)]
    R = _Round("multi_target", ["multi_target"], targets, target_ids=[7, 3, 12])
    for i in range(36):
        t = (2, 0, 1)[i % 3]
        n = len(targets[t])
        a = int(rng.integers(0, n - 300))
        b = int(min(n, a + rng.integers(300, 900)))
        codes = mutate(rng, targets[t][a:b], 0.02, 0.01, 0.01)
        R.add(t, a, b, bool(rng.integers(0, 2)), codes=codes)
    return [R.case()]


def cases():
    out = (_len_rule() + _empty_window() + _one_pair() + _short_tail() + _q_exact() + _q_oriented() + _q_blocks() + _ties() +
           _unused_and_degenerate() + _multi_target())
    assert len({c["name"] for c in out}) == len(out)
    return out
