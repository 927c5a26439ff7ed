"""The three routes of edit_distance_dev behind the lane windows (raven_amd/csrc/edit_distance.hip) on crafted pairs: the
wave ring (ed_banded_kernel<4>: 64 lanes, super-blocks of 4 x 64 rows, thresholds doubled up to 32 * 4 * 63 = 8 064), the
workgroup ring (ed_wide_kernel<4>: L = 64 .. 512 lanes, one sweep, capacity 128 (L - 1)) and the unbanded striped sweep
(ed_full_kernel: stripes of 64 blocks).  The cases, tagged by class (TAGS), and the model: what the function must leave
for a pair and which kernel sites a call must have launched, from the DP distance D alone.  No GPU and nothing of csrc
is used here; tests/test_ed_ring_cases.py checks every case against the oracle's DP and the model's own claims,
tests/test_gpu_ed_ring_cases.py runs the device over them (rvn_test_edit_distance_dev).

A case: a sequence pair SEQS[case["seq"]] = (a, b, planted D) — a = the pattern (rows), b = the text (columns) in a's
orientation — placed into two reads of its own (random flank of `ab` / `bb` bases in front, `at` / `bt` behind; strand 0
stores b reverse-complemented), a threshold km (None: unbounded) and a route: route = 0, L = 0 the usual one (wide_sweep = 0); route = 1 (wide_sweep = 1)
with L = 64 / 128 / 512 the workgroup ring of that many lanes (engine option ed_wide_lanes = L), with L = 1 the ring
switched off (ed_wide_lanes = 1: the usual route after all).  Several cases share a sequence pair (placements,
strands, thresholds, routes): its DP is computed once.

Planting: a block of delta bases cut out of one side makes it a subsequence of the other, D = delta exactly, and
|n - m| = delta > 384 is what sends a small pair past the widest lane window into the wave ring with a first threshold
of delta.  s further bases replaced by a letter the other side does not have give D = delta + s exactly, also at equal
lengths (_cut_pair has the argument).  Every planted D is a claim by construction; the CPU test holds it to the DP."""
import functools
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import oracle
from raven_amd import seqio
from tests import ed_lane_model as lane

ABOVE = lane.ABOVE
INF = lane.INF
UNBOUNDED = 0xFFFFFFF0   # the threshold a call WITH thresholds passes for a pair that has none (what the lane kernel assumes without)
CAP = 32 * 4 * 63        # 8 064: the wave ring's capacity
LANE_SLOTS = 7           # the widest lane window: the one every pair of a call of at most SAMPLE pairs gets
SAMPLE = 2048            # calls up to this size are "the sample" of the lane stage: one lane launch for all
TAGS = ("thr_edge", "cap_edge", "geometry", "ring_reuse", "retire", "text_side", "bounded", "wide", "full", "batch")
DEC = np.frombuffer(b"ACGT", dtype=np.uint8)
THREADS = min(16, os.cpu_count() or 1)


def cap_wide(L):
    return 128 * (L - 1)


def kmax_rule(mx, ratio):
    """The largest x with !(1 - x / mx < ratio): the threshold rvn_path_similarity_batch sweeps a pair with (the rule of
    assemble.cc:267-281 itself, in doubles)."""
    keeps = lambda x: not (1.0 - float(x) / float(mx) < ratio)
    t = int(max(0.0, min(float(mx), (1.0 - ratio) * mx)))
    while t < mx and keeps(t + 1):
        t += 1
    while t > 0 and not keeps(t):
        t -= 1
    return t


# ---- the model -------------------------------------------------------------------------------------------------------------

def ring_lanes(route, L):
    """Lanes of the workgroup ring a call takes — route: its wide_sweep, L: the engine's ed_wide_lanes (0 / -1: the default
    of 512, 1: no workgroup ring) — or 0: the usual route."""
    if not route or L == 1:
        return 0
    return 512 if L in (0, -1) else L


def expected(n, m, D, km=INF, route=0, L=0):
    """The value edit_distance_dev must leave (km: the pair's threshold, INF / UNBOUNDED or more = none)."""
    L = ring_lanes(route, L)
    if n == 0 or m == 0:
        return n + m if n + m <= km else ABOVE
    if abs(n - m) > km:
        return ABOVE
    if km >= UNBOUNDED or D <= km:
        return D
    # D > km: the rings answer "above"; only the full sweep answers with the exact distance (path_similarity_batch's exception)
    if L:
        return ABOVE if km <= cap_wide(L) else D
    return ABOVE if (km <= CAP or D <= CAP) else D


Trace = namedtuple("Trace", "decided ks value lane")  # decided: lane / wave / wide / full; ks: the thresholds swept by the ring


def trace(n, m, D, km=INF, route=0, L=0):
    """The way of a pair through the stages, restated from the kernels' control flow: who decides it, the thresholds the
    ring sweeps on the way (the last one decides, or hands on to the full sweep), the stored value."""
    d = abs(n - m)
    L = ring_lanes(route, L)
    if L:  # ed_wide_kernel: ONE sweep, at kmax where the ring holds it, at the capacity otherwise
        cap = cap_wide(L)
        if n == 0 or m == 0 or d > km:
            return Trace("wide", (), n + m if (n == 0 or m == 0) and d <= km else ABOVE, None)
        if d > cap:
            return Trace("full", (), D, None)
        k = min(km, cap)
        if D <= k:
            return Trace("wide", (k,), D, None)
        return Trace("wide", (k,), ABOVE, None) if k >= km else Trace("full", (k,), D, None)
    outcome, value = lane.expected(n, m, D, km, LANE_SLOTS)
    if outcome not in ("no_fit", "overflow"):
        return Trace("lane", (), value, outcome)
    if d > CAP:  # no threshold of the ring holds the length difference
        return Trace("full", (), D, outcome)
    k = max(64, d)
    if km <= CAP and km > k:  # bounded: one sweep at the threshold decides
        k = km
    ks = []
    while True:
        ks.append(k)
        if D <= k:
            return Trace("wave", tuple(ks), D if D <= km else ABOVE, outcome)
        if k >= km:
            return Trace("wave", tuple(ks), ABOVE, outcome)
        if k == CAP:
            return Trace("full", tuple(ks), D, outcome)
        k = min(2 * k, CAP)


def leaves_lane(n, m, D, km=INF):
    """The lane stage hands the pair on iff the widest window overflows (tests/ed_lane_model.py)."""
    return lane.expected(n, m, D, km, LANE_SLOTS)[1] == lane.OVERFLOW_WIDE


def leaves_wave(n, m, D, km=INF):
    """Of the pairs the wave ring gets: the ones it leaves to the full sweep."""
    return abs(n - m) > CAP or (D > CAP and km > CAP)


def leaves_wide(n, m, D, km, L):
    """Of the pairs of a call by the workgroup ring of L lanes: the ones it leaves to the full sweep."""
    if n == 0 or m == 0 or abs(n - m) > km:
        return False
    return abs(n - m) > cap_wide(L) or (D > cap_wide(L) and km > cap_wide(L))


def launches(shapes, route=0, L=0):
    """{site: launches} of ONE call of edit_distance_dev on shapes = [(n, m, D, km)] (1 .. SAMPLE pairs)."""
    assert 1 <= len(shapes) <= SAMPLE
    L = ring_lanes(route, L)
    if L:
        return dict(edit_lane=0, edit_banded=0, edit_wide=1, edit_full=int(any(leaves_wide(*s, L) for s in shapes)))
    on = [s for s in shapes if leaves_lane(*s)]
    return dict(edit_lane=1, edit_banded=int(bool(on)), edit_wide=0, edit_full=int(any(leaves_wave(*s) for s in on)))


# ---- sequences -------------------------------------------------------------------------------------------------------------

def dp(a, b):
    return oracle.edit_distance(DEC[a].tobytes(), DEC[b].tobytes())


def _rand(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def _cut_pair(rng, n_long, delta, s=0, at=None, foreign=False):
    """(long, short): short = long without a block of delta bases (anywhere, delta = 0: a copy), s of its bases replaced.
    With s > 0 long is drawn from three of the four letters and the replaced bases get the fourth: such a base matches
    nothing in long, so it costs an edit of its own whatever the alignment does with the delta deletions the lengths
    demand: D = delta + s, for any positions.  (Substitutions within a four-letter sequence do NOT add up beside a cut:
    a changed base t bases from a cut of delta > 3 t random bases is free, the alignment finds it and the t bases between
    as a subsequence of what it has to delete anyway.)  foreign: the cut block itself consists of the fourth letter, so
    that nothing of short finds a partner inside it: the only alignments of cost delta run straight, gap at the cut."""
    z = int(rng.integers(0, 4))
    long_ = _rand(rng, n_long) if s == 0 and not foreign else ((z + 1 + rng.integers(0, 3, size=n_long)) & 3).astype(np.uint8)
    n_short = n_long - delta
    at = int(rng.integers(0, n_short + 1)) if at is None else at
    if foreign:
        assert s == 0
        long_[at:at + delta] = z
    short = np.concatenate([long_[:at], long_[at + delta:]])
    if s > n_short:
        raise ValueError("no room for %d substitutions in %d bases" % (s, n_short))
    short[rng.choice(n_short, size=s, replace=False)] = z
    return long_, short


SEQS = {}   # key -> (a codes, b codes in a's orientation, planted D)


def _seq(key, a, b, D):
    assert key not in SEQS
    SEQS[key] = (np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8), int(D))
    return key


def _cut_seq(key, rng, n_long, delta, s, long_rows, at=None, foreign=False):
    long_, short = _cut_pair(rng, n_long, delta, s, at, foreign)
    return _seq(key, long_ if long_rows else short, short if long_rows else long_, delta + s)


def _case(tag, name, seq, strand=1, ab=0, bb=0, at=7, bt=5, km=None, L=0, **more):
    return dict(tag=tag, name=name, seq=seq, strand=strand, ab=ab, bb=bb, at=at, bt=bt, km=km, route=int(L != 0), L=L, **more)


@functools.lru_cache(maxsize=None)
def cases():
    """Every case, in class order.  Deterministic: fixed seeds, no case depends on what ran before the module was loaded."""
    SEQS.clear()
    out = []

    # ---- thr_edge: the doubling sequence of the wave ring at its own edges
    rng = np.random.default_rng(8101)
    for i, s in enumerate((0, 1, 400, 401, 1200, 1201)):   # first threshold 400: D = k and k + 1 at 400, 800, 1600
        key = _cut_seq("thr400+%d" % s, rng, 400 + 3 * s + 300, 400, s, long_rows=i % 2 == 0)
        out.append(_case("thr_edge", key, key, strand=(i // 2 + i) & 1, ab=3 * i, bb=31 - i))
    for i, target in enumerate((512, 513)):                # equal lengths: floor 64, beyond the lane window, D = 512 / 513
        key = _cut_seq("thr_eq%d" % target, rng, 1500, 0, target, True)
        out.append(_case("thr_edge", key, key, strand=i, ab=17, bb=40))
    for i, s in enumerate((0, 1, 400)):                    # first threshold 4 100: the next is min(2 k, cap) = cap
        key = _cut_seq("thr4100+%d" % s, rng, 4100 + 2500, 4100, s, long_rows=i != 1)
        out.append(_case("thr_edge", key, key, strand=(i + 1) & 1, ab=i, bb=2 * i))

    # ---- cap_edge: D and |n - m| on both sides of the wave ring's capacity
    rng = np.random.default_rng(8102)
    i = 0
    for delta, s in ((8064, 0), (8063, 1), (8063, 2), (8065, 0)):
        for long_rows in (True, False):
            key = _cut_seq("cap%d+%d%s" % (delta, s, "r" if long_rows else "c"), rng, delta + 236, delta, s, long_rows)
            out.append(_case("cap_edge", key, key, strand=(i // 2 + i) & 1, ab=5 + i, bb=29 + i))
            i += 1

    # ---- geometry: pad mask, partial last super-block, patterns of one block; D = 400
    rng = np.random.default_rng(8103)
    for i, n in enumerate((1, 63, 64, 65, 255, 256, 257, 511, 512, 513)):
        for long_rows in (False, True):
            key = _cut_seq("geo%d%s" % (n, "r" if long_rows else "c"), rng, n + 400, 400, 0, long_rows)
            # the pattern of the very last case lies in the last read of the class's set and ends with it
            last = n == 513 and long_rows
            out.append(_case("geometry", key, key, strand=(i + long_rows) & 1, ab=(7 * i) % 32, bb=(11 * i + 3) % 32,
                             at=0 if last else 7, a_last=last))

    # ---- ring_reuse: rows beyond 64 super-blocks; a lane moves on to super-block s + 64 in mid-text
    rng = np.random.default_rng(8104)
    for i, (n, delta, s, long_rows) in enumerate(((16384, 385, 30, True), (16385, 3000, 200, True), (16448, 2000, 700, False),
                                                  (16640, 3000, 100, True), (16641, 500, 400, False))):
        key = _cut_seq("rr%d" % n, rng, n if long_rows else n + delta, delta, s, long_rows)
        out.append(_case("ring_reuse", key, key, strand=i & 1, ab=(9 * i + 1) % 32, bb=(5 * i + 31) % 32))
    out.append(_case("ring_reuse", "rr16385 reverse", "rr16385", strand=0, ab=31, bb=1))
    key = _cut_seq("rr32769", rng, 32769, 7000, 30, True)   # super-blocks 0 .. 128: a second wrap
    out.append(_case("ring_reuse", key, key, strand=0, ab=2, bb=30))

    # ---- retire: blocks that retire above the band / never enter it
    rng = np.random.default_rng(8105)
    out.append(_case("retire", "retire17000x9000", _cut_seq("retire17000x9000", rng, 17000, 8000, 10, True), strand=1, ab=4, bb=8))
    out.append(_case("retire", "retire9000x17000", _cut_seq("retire9000x17000", rng, 17000, 8000, 10, False), strand=0, ab=8, bb=4))
    out.append(_case("retire", "retire237x8300", _cut_seq("retire237x8300", rng, 8300, 8063, 0, False), strand=0, ab=0, bb=33))
    out.append(_case("retire", "retire8300x237", _cut_seq("retire8300x237", rng, 8300, 8063, 0, True), strand=1, ab=33, bb=0))
    # the cut in the first block and D = |n - m| = the capacity: behind it the path runs ON the band's edge, through the one
    # cell a block still has in its last column (columns longer) / in its first (rows longer).  A block that leaves a column
    # early or comes a column late costs this call the full sweep nobody else in it needs.  (The cut block is of a letter of
    # its own: from random bases the 54 rows between the cut and the first block boundary would find partners in it, the cell
    # beside the path would be one cheaper than the path, and the edge cell would not be needed.)
    out.append(_case("retire", "retire236x8300", _cut_seq("retire236x8300", rng, 8300, CAP, 0, False, at=10, foreign=True), strand=1, ab=6, bb=21))
    out.append(_case("retire", "retire8300x236", _cut_seq("retire8300x236", rng, 8300, CAP, 0, True, at=10, foreign=True), strand=0, ab=21, bb=6))

    # ---- text_side: TextCursor / load_peq addressing.  Text of m columns at b_begin: the residues of both ends mod 32
    rng = np.random.default_rng(8106)

    def text_pair(m):
        key = "text%d" % m
        return key if key in SEQS else _cut_seq(key, rng, m + 400, 400, 0, True)

    i = 0
    for strand in (1, 0):
        for b0 in (0, 31):
            for e in (0, 1):            # (b_begin + m) % 32
                bb = 32 + b0 if (i & 1) else b0
                m = 512 + e - b0
                out.append(_case("text_side", "text s%d b%d e%d" % (strand, b0, e), text_pair(m), strand=strand, ab=(0, 1, 31)[i % 3],
                                 bb=bb, bt=3 + i))
                i += 1
    for strand in (1, 0):               # begins one base into a word, ends one base before a word's end
        out.append(_case("text_side", "text s%d b1 e31" % strand, text_pair(510), strand=strand, ab=31 - 30 * strand, bb=33 - 32 * strand))
    for bb in (0, 1, 31):               # the reverse strand whose first word is the read's first (the cursor's look-ahead clamps at 0)
        out.append(_case("text_side", "text rc begin %d" % bb, text_pair(500 + bb), strand=0, ab=1, bb=bb, bt=0))
    i = 0
    for strand in (1, 0):               # the same on a pair whose lanes re-initialise their cursor in mid-text
        for b0 in (0, 31):
            out.append(_case("text_side", "rr16385 s%d b%d" % (strand, b0), "rr16385", strand=strand, ab=(1, 31, 0, 33)[i],
                             bb=b0 + 32 * (i & 1), bt=(0, 3, 30, 31)[i]))
            i += 1
    out.append(_case("text_side", "rr16385 rc begin 1", "rr16385", strand=0, ab=0, bb=1, bt=0))
    # the text of the very last case lies in the last read of the class's set and ends on its last base
    out.append(_case("text_side", "text ends the set", text_pair(513), strand=0, ab=31, bb=31, bt=0))

    # ---- bounded: kmax in the wave ring, on both sides of D, of |n - m| and of the capacity
    rng = np.random.default_rng(8107)
    i = 0
    for key, D, delta in (("thr400+400", 800, 400), ("rr16385", 3200, 3000)):
        for km in (D - 1, D, D + 1, delta, delta - 1, CAP):
            out.append(_case("bounded", "%s km %d" % (key, km), key, strand=i & 1, ab=i % 32, bb=(3 * i) % 32, km=km))
            i += 1
    for target, kms in ((40, (10, 39, 40, 63)), (100, (10, 63))):   # thresholds below the ring's floor of 64
        key = _cut_seq("eq%d" % target, rng, 1000, 0, target, True)
        for km in kms:
            out.append(_case("bounded", "%s km %d" % (key, km), key, strand=i & 1, ab=i % 32, bb=(3 * i) % 32, km=km))
            i += 1
    for s in (1, 2, 3):                                             # D = 8 064 / 8 065 / 8 066 with a first threshold of 8 063
        key = _cut_seq("cap8063+%db" % s, rng, 8063 + 300, 8063, s, long_rows=s != 2)
        for km in (CAP, CAP + 1, 20000):
            out.append(_case("bounded", "%s km %d" % (key, km), key, strand=i & 1, ab=i % 32, bb=(3 * i) % 32, km=km))
            i += 1

    for n in (65, 257, 513):   # D = |n - m| = km: the one sweep runs with the path on the band's edge (see retire236x8300)
        for long_rows in (False, True):
            key = _cut_seq("edge%d%s" % (n, "r" if long_rows else "c"), rng, n + 400, 400, 0, long_rows, at=10, foreign=True)
            for km in (400, 401):
                out.append(_case("bounded", "%s km %d" % (key, km), key, strand=i & 1, ab=i % 32, bb=(3 * i) % 32, km=km))
                i += 1

    # ---- wide: the workgroup ring, L lanes
    rng = np.random.default_rng(8108)
    i = 0

    def wide(name, seq, L, **kw):
        nonlocal i
        kw.setdefault("strand", i & 1)
        kw.setdefault("ab", (7 * i) % 32)
        kw.setdefault("bb", (13 * i + 31) % 32)
        out.append(_case("wide", "L%d %s" % (L, name), seq, L=L, **kw))
        i += 1

    for s in (1, 2, 3):                 # L = 128: capacity 16 256, a 244-base side
        for long_rows in (True, False):
            _cut_seq("w16255+%d%s" % (s, "r" if long_rows else "c"), rng, 16255 + 244, 16255, s, long_rows)
    for delta in (16256, 16257):
        for long_rows in (True, False):
            _cut_seq("w%d%s" % (delta, "r" if long_rows else "c"), rng, delta + 244, delta, 0, long_rows, at=10, foreign=True)
    for L in (64, 1):                   # L = 64: the wave ring's capacity; L = 1: the same members on the usual route
        for key in ("cap8064+0r", "cap8064+0c", "cap8063+1r", "cap8063+2c", "cap8065+0r", "cap8065+0c"):
            wide(key, key, L)
        for key, km in (("cap8063+1c", 8063), ("cap8063+1c", 8064), ("cap8063+2r", 8064), ("cap8063+2r", 8065), ("cap8063+2r", 8066),
                        ("cap8063+3b", 8065)):
            wide("%s km %d" % (key, km), key, L, km=km)
        for strand in (1, 0):           # n = 16 385 on 64 lanes: the ring is re-used
            wide("rr16385 s%d" % strand, "rr16385", L, strand=strand, bb=31 * strand)
        for km in (3199, 3200, 8064, 8065):
            wide("rr16385 km %d" % km, "rr16385", L, km=km)
        wide("rr16641", "rr16641", L)
        for strand, bb in ((1, 0), (1, 31), (0, 1), (0, 31), (0, 32)):   # word-offset begins of the text
            wide("text s%d b%d" % (strand, bb), "text%d" % (481 + 32 * (bb & 1)), L, strand=strand, bb=bb, ab=(0, 1, 31)[bb % 3])
        for key in ("edge257c", "edge257r"):                             # the path on the band's edge (see retire236x8300)
            wide("%s km 400" % key, key, L, km=400)
    for suffix in ("r", "c"):           # L = 128
        wide("w16256" + suffix, "w16256" + suffix, 128)
        wide("w16257" + suffix, "w16257" + suffix, 128)
        wide("w16255+1" + suffix, "w16255+1" + suffix, 128)
        wide("w16255+2" + suffix, "w16255+2" + suffix, 128)
    for key, km in (("w16255+1r", 16255), ("w16255+1r", 16256), ("w16255+1c", 16257), ("w16255+2r", 16256), ("w16255+2c", 16257),
                    ("w16255+2r", 16258), ("w16255+3r", 16257), ("w16255+3c", 16257)):
        wide("%s km %d" % (key, km), key, 128, km=km)
    for key in ("w16256r", "w16256c"):  # D = |n - m| = km = the capacity: the path on the band's edge
        wide("%s km 16256" % key, key, 128, km=16256)
    for strand in (1, 0):               # super-blocks 64 and up: work in the second wave
        wide("rr16385 s%d" % strand, "rr16385", 128, strand=strand, bb=31)
        wide("rr16641 s%d" % strand, "rr16641", 128, strand=strand, bb=1)
    wide("rr32769", "rr32769", 128, strand=0)   # 129 super-blocks on 128 lanes: lane 0 takes a second one
    for km in (3199, 3200):
        wide("rr16385 km %d" % km, "rr16385", 128, km=km)
    for strand, bb in ((1, 31), (0, 0), (0, 31)):
        wide("text s%d b%d" % (strand, bb), "text%d" % (481 + 32 * (bb & 1)), 128, strand=strand, bb=bb)
    for strand in (1, 0):               # L = 512
        wide("rr16385 s%d" % strand, "rr16385", 512, strand=strand)
        wide("text s%d" % strand, "text510", 512, strand=strand, bb=33 - 32 * strand)
    for km in (3199, 3200, 3201):
        wide("rr16385 km %d" % km, "rr16385", 512, km=km)
    wide("cap8065+0r", "cap8065+0r", 512)
    wide("w16257c", "w16257c", 512)
    # whole reads on the forward strand with the threshold of RemoveBubbles' rule: what rvn_path_similarity_batch makes of a pair
    for L in (64, 128, 512):
        for key, ratio in (("rr16385", 0.5), ("rr16641", 0.5), ("rr32769", 0.7), ("retire17000x9000", 0.5)):
            a, b, _ = SEQS[key]
            if L != 128 and key == "rr32769":
                continue
            wide("%s whole, ratio %g" % (key, ratio), key, L, strand=1, ab=0, bb=0, at=0, bt=0, ratio=ratio,
                 km=kmax_rule(max(a.shape[0], b.shape[0]), ratio))

    # ---- full: the striped sweep's geometry.  One, two and three stripes, a partly filled last stripe, m = 1
    rng = np.random.default_rng(8109)
    full = []
    for i, n in enumerate((1, 10, 64, 4096)):        # one stripe; the columns carry the cut
        key = _cut_seq("full%d" % n, rng, n + 8065 + 11 * i, 8065 + 11 * i, 0, False)
        full.append(_case("full", key, key, strand=i & 1, ab=i, bb=31 - i))
    key = _cut_seq("full4097", rng, 4097 + 8070, 8070, 0, False)   # two stripes, one block in the second
    full.append(_case("full", key, key, strand=0, ab=1, bb=1))
    i = 0
    for n in (8192, 8193, 8300):                     # two full stripes; three: both boundary rows in turn
        for m in ((100,) if n == 8192 else (1, 2, 33, 100)):
            a = _rand(rng, n)
            at = int(rng.integers(0, n - m + 1))
            key = _seq("full%dx%d" % (n, m), a, a[at:at + m].copy(), n - m)
            full.append(_case("full", key, key, strand=i & 1, ab=(5 * i) % 32, bb=(9 * i + 31) % 32))
            i += 1
    # equal length, nothing in common (one side over A / C, the other over G / T): D = 8 200, the ring sweeps its whole
    # sequence first
    key = _seq("full8200", rng.integers(0, 2, size=8200, dtype=np.uint8), rng.integers(2, 4, size=8200, dtype=np.uint8), 8200)
    full.append(_case("full", key + " forward", key, strand=1, ab=31, bb=0))
    full.append(_case("full", key + " reverse", key, strand=0, ab=0, bb=31))
    out += [full[j] for j in np.random.default_rng(81090).permutation(len(full))]   # (an order that is not sorted by size)

    # ---- batch: list collection, four pairs per workgroup.  A pool; batch_calls() picks the calls from it
    rng = np.random.default_rng(8110)
    for i, (n, delta) in enumerate(((300, 400), (700, 390), (1000, 450), (64, 500), (129, 385))):
        key = _cut_seq("batch wave %d" % i, rng, n + delta, delta, 0, i % 2 == 0)
        out.append(_case("batch", key, key, strand=i & 1, ab=i, bb=2 * i, wave=True))
    for i in range(16):
        n = 200 + 37 * i
        key = _cut_seq("batch lane %d" % i, rng, n, i % 3, i, i % 2 == 0)
        out.append(_case("batch", key, key, strand=i & 1, ab=i, bb=31 - i, wave=False))
    out.append(_case("batch", "batch empty rows", _seq("batch empty rows", np.zeros(0, np.uint8), _rand(rng, 500), 500), strand=0, wave=False))
    out.append(_case("batch", "batch empty columns", _seq("batch empty columns", _rand(rng, 90), np.zeros(0, np.uint8), 90), strand=1,
                     ab=3, bb=9, wave=False))
    for c in out:
        c.setdefault("a_last", False)
        c.setdefault("ratio", None)
    assert [c["tag"] for c in out] == sorted((c["tag"] for c in out), key=TAGS.index)
    return tuple(out)


def by_tag(tag):
    return [c for c in cases() if c["tag"] == tag]


def batch_calls():
    """{pairs of the wave ring's share: indices into by_tag("batch")}: 1, 3, 4 and 5 pairs for the wave ring (four share a
    workgroup), scattered among pairs the lane stage decides."""
    pool = by_tag("batch")
    wave = [i for i, c in enumerate(pool) if c["wave"]]
    rest = [i for i, c in enumerate(pool) if not c["wave"]]
    calls = {}
    for share in (1, 3, 4, 5):
        pick = wave[5 - share:] + rest[share:]
        calls[share] = [pick[j] for j in np.random.default_rng(8200 + share).permutation(len(pick))]
    return calls


def shape(c, D=None):
    """(n, m, D, km) of a case as the model takes it (D: the DP's, default the planted one)."""
    a, b, planted = SEQS[c["seq"]]
    return a.shape[0], b.shape[0], planted if D is None else D, INF if c["km"] is None else c["km"]


@functools.lru_cache(maxsize=None)
def distances():
    """{sequence key: DP distance}, every sequence pair once, on a thread pool (the oracle's DP runs outside the
    interpreter lock); the largest first."""
    cases()
    keys = sorted(SEQS, key=lambda k: -SEQS[k][0].shape[0] * SEQS[k][1].shape[0])
    with ThreadPoolExecutor(THREADS) as ex:
        return dict(zip(keys, ex.map(lambda k: dp(SEQS[k][0], SEQS[k][1]), keys)))


def dp_cells():
    cases()
    return sum(a.shape[0] * b.shape[0] for a, b, _ in SEQS.values())


def place(some, seed=1):
    """One packed read set for the cases `some`: per case two reads (flank + span + tail; strand 0 stores the reverse
    complement of b), the pattern's read first unless the case says a_last.  Returns (ReadSet, pairs as 8 x uint32 records,
    kmax: uint32 per pair with UNBOUNDED for the cases without a threshold, or None when no case has one)."""
    rng = np.random.default_rng(seed)
    reads, P = [], []
    for c in some:
        a, b, _ = SEQS[c["seq"]]
        stored_b = b if c["strand"] else (3 - b[::-1])
        ra = np.concatenate([_rand(rng, c["ab"]), a, _rand(rng, c["at"])])
        rb = np.concatenate([_rand(rng, c["bb"]), stored_b, _rand(rng, c["bt"])])
        if c["a_last"]:
            reads += [rb, ra]
            ia, ib = len(reads) - 1, len(reads) - 2
        else:
            reads += [ra, rb]
            ia, ib = len(reads) - 2, len(reads) - 1
        P.append((ia, c["ab"], a.shape[0], ib, c["bb"], b.shape[0], c["strand"], 0))
    rs = seqio.pack_reads(reads)
    pairs = np.array(P, dtype=np.uint32).reshape(-1, 8)
    kmax = None
    if any(c["km"] is not None for c in some):
        kmax = np.array([UNBOUNDED if c["km"] is None else c["km"] for c in some], dtype=np.uint32)
    return rs, pairs, kmax
