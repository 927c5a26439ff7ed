"""Polishing rounds whose alignments need a band wider than one wave's ring (nwpath.h: the striped sweep).

  * a small round with the ring forced down to 1 / 2 / 4 lanes (engine option nw_stripe_lanes: every alignment wider
    than that is striped, here all of them): the layer table equals the oracle's row for row, the consensus is within the
    tolerances of tests/test_gpu_polish.py;
  * the production stage on single ultra-long pairs (250 - 600 kb, the test hook's device mode): distances equal the
    exact edit-distance kernel's, at least one of them beyond one ring, and the records of such a pair equal an
    independent memory-light exact path (checked against the oracle on small pairs here);
  * a round with ultra-long reads (250 - 600 kb at ~10 % error: distances of 23 000 - 57 000, most beyond the 32 320
    rows of one ring): nothing is dropped, the short reads' layers are those of the round without the ultra-long reads, and every
    ultra-long read has layers in most of the windows it spans."""
import math
import time

import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip, seqio, synth
from tests import polish_util as pu2

pytestmark = pytest.mark.gpu


def _ed(a, b):
    return oracle.edit_distance(bytes(np.asarray(a, np.uint8) + 65), bytes(np.asarray(b, np.uint8) + 65))


def _pack(codes):
    return np.concatenate([seqio.pack_reads([np.asarray(codes, np.uint8)]).packed, np.zeros(2, np.uint64)])


def _device(t, read, rc, w=500, lanes=0):
    q = (3 - read[::-1]).astype(np.uint8) if rc else read
    return hip.test_nw_breakpoints(_pack(t), len(t), _pack(read), len(read), 0, len(t), 0, len(q), rc, w,
                                   stripe_lanes=lanes, device=True)


def _pairs_of(recs):
    got = []
    for r in recs:
        if r["first_t"] != 0xFFFFFFFF:
            got += [(int(r["first_t"]), int(r["first_q"])), (int(r["last_t"]), int(r["last_q"]))]
    return got


@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_forced_stripes_layers_bit_exact(lanes):
    # rings of at most 4 lanes: no variant but (R, G) = (1, 4) is allowed, and that one holds a band of 196 only — every
    # alignment of these 2.5-kb reads (thresholds of ~340) is striped; the stage says so on one such pair
    rng = np.random.default_rng(lanes)
    t = rng.integers(0, 4, 2500, dtype=np.uint8)
    _, _, plan, _ = _device(t, synth.mutate(rng, t, 0.04, 0.03, 0.03), 0, lanes=lanes)
    assert plan["stripe_lanes"] == lanes and plan["stripes"] > 1
    truths, drafts, targets, reads, _ = pu2.make_case(genome_len=24_000, coverage=25, read_len=2500, seed=7)
    eng = hip.Engine(15, 5)
    assert eng.set_option("nw_stripe_lanes", lanes) == 0
    cons, ratio, st = eng.polish_round(eng.upload(targets), eng.upload(reads))
    got = eng.polish_layers()
    want = oracle.polish_layers(targets, reads)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert st["n_aligned"] == st["n_reads_used"] and st["n_dropped_layers"] == 0
    ref, _ = oracle.polish_round(targets, reads)
    d = _ed(cons[0], ref[0])
    assert d <= math.ceil(0.001 * len(ref[0])), d
    assert _ed(cons[0], truths[0]) <= math.ceil(1.05 * _ed(ref[0], truths[0]))


def myers_path_pairs(tt, tq, w, ck=1024):
    """Global unit-cost alignment path of tq (columns) against tt (rows) with racon's tie order (diagonal, then query
    base only, then target base only), memory-light: Myers' bit-vectors of whole columns as Python integers, a
    checkpoint every `ck` columns, each segment recomputed when the walk enters it.  Returns (breakpoint pairs as
    oracle.nw_breakpoints gives them for t_begin = q_begin = 0, distance)."""
    tt = np.asarray(tt, np.uint8)
    tq = np.asarray(tq, np.uint8)
    n, m = len(tt), len(tq)
    full = (1 << n) - 1
    peq = [int.from_bytes(np.packbits(tt == c, bitorder="little").tobytes(), "little") for c in range(4)]
    qs = tq.tolist()

    def step(pv, mv, c):
        eq = peq[c]
        xv = eq | mv
        xh = (((eq & pv) + pv) ^ pv) | eq
        ph = (mv | ~(xh | pv)) & full
        mh = pv & xh
        ph = ((ph << 1) | 1) & full
        mh = (mh << 1) & full
        return (mh | ~(xv | ph)) & full, ph & xv

    cks = [(full, 0)]
    pv, mv = full, 0
    for j in range(1, m + 1):
        pv, mv = step(pv, mv, qs[j - 1])
        if j % ck == 0:
            cks.append((pv, mv))
    dist = m + pv.bit_count() - mv.bit_count()
    seg = {}

    def col(x):
        if x not in seg:
            seg.clear()
            c0 = (x // ck) * ck
            p, q = cks[c0 // ck]
            seg[c0] = (p, q)
            for jj in range(c0 + 1, min(m, c0 + ck + 2) + 1):
                p, q = step(p, q, qs[jj - 1])
                seg[jj] = (p, q)
        return seg[x]

    def score(i, x):
        p, q = col(x)
        msk = (1 << i) - 1
        return x + (p & msk).bit_count() - (q & msk).bit_count()

    def dv(i, x):
        p, q = col(x)
        return ((p >> (i - 1)) & 1) - ((q >> (i - 1)) & 1)

    wins = {}
    i, j = n, m
    dc = dist
    dl = score(i, j - 1) if j > 0 else 0
    ts = tt.tolist()
    while i > 0 and j > 0:
        dv1 = dv(i, j - 1)
        ddiag = dl - dv1
        if ts[i - 1] == qs[j - 1] or ddiag + 1 == dc:
            r = wins.setdefault((i - 1) // w, [None, None])
            if r[1] is None:
                r[1] = (i, j)
            r[0] = (i - 1, j - 1)
            i, j, dc = i - 1, j - 1, ddiag
            dl = score(i, j - 1) if j > 0 else 0
        elif dl + 1 == dc:
            j, dc = j - 1, dl
            dl = score(i, j - 1) if j > 0 else 0
        else:
            d = dv(i, j)
            i, dc, dl = i - 1, dc - d, dl - dv1
    pairs = []
    for k in sorted(wins):
        pairs += wins[k]
    return pairs, dist


def test_memory_light_reference_equals_the_oracle():
    rng = np.random.default_rng(5)
    for n, w, ck in [(1, 50, 64), (7, 50, 64), (200, 50, 64), (900, 64, 64), (3000, 500, 256), (2000, 7, 100)]:
        t = rng.integers(0, 4, n, dtype=np.uint8)
        q = synth.mutate(rng, t, 0.04, 0.03, 0.03)
        if len(q) == 0:
            q = t.copy()
        pairs, d = myers_path_pairs(t, q, w, ck)
        want, wd = oracle.nw_breakpoints(q, t, 0, 0, w)
        assert d == wd and pairs == [tuple(int(v) for v in p) for p in want]
    h = np.zeros(300, np.uint8)  # homopolymers: the tie rule decides
    want, _ = oracle.nw_breakpoints(h[:250], h, 0, 0, 100)
    assert myers_path_pairs(h, h[:250], 100, 32)[0] == [tuple(int(v) for v in p) for p in want]


def test_ultralong_pairs_production_stage():
    rng = np.random.default_rng(77)
    pairs = []
    for n, rc in [(250_000, 0), (360_000, 1), (600_000, 0)]:
        t = rng.integers(0, 4, n, dtype=np.uint8)
        q = synth.mutate(rng, t, 0.04, 0.03, 0.03)
        pairs.append((t, q, rc))
    # exact distances from the edit-distance kernel (unbanded): at least one beyond one ring
    rs = seqio.pack_reads([x for t, q, _ in pairs for x in (t, q)])
    ed = np.zeros(len(pairs), dtype=hip.ED_PAIR_DTYPE)
    for x, (t, q, _) in enumerate(pairs):
        ed[x] = (2 * x, 0, len(t), 2 * x + 1, 0, len(q), 1, 0)
    eng = hip.Engine(15, 5)
    want, _, _ = eng.edit_distance_batch(eng.upload(rs), ed)
    assert max(want) > 32_320, want
    beyond = []
    for x, (t, q, rc) in enumerate(pairs):
        read = (3 - q[::-1]).astype(np.uint8) if rc else q
        recs, d, plan, _ = _device(t, read, rc)
        print("pair of %d kb: distance %d, k %d, %s, %d stripes, stage %.1f ms"
              % (len(t) // 1000, d, plan["k"], "striped" if plan["stripe_lanes"] else "one ring", plan["stripes"],
                 plan["stage_ms"]))
        assert d == want[x]
        if d > 32_320:
            assert plan["stripe_lanes"] == 64 and plan["stripes"] > 1
            beyond.append((len(t), x, recs))
    # the shortest pair beyond one ring against the independent path
    _, x, recs = min(beyond)
    t, q, _ = pairs[x]
    pairs_ref, d_ref = myers_path_pairs(t, q, 500)
    assert d_ref == want[x] and _pairs_of(recs) == pairs_ref


def _reads(rng, genome, lengths, err):
    out = []
    for n in lengths:
        n = int(min(n, len(genome) - 1))
        p = int(rng.integers(0, len(genome) - n))
        r = synth.mutate(rng, genome[p:p + n], *err)
        out.append((3 - r[::-1]).astype(np.uint8) if rng.random() < 0.5 else r)
    return out


def test_ultralong_reads_round():
    rng = np.random.default_rng(2026)
    genome = synth.make_genome(1_000_000, seed=31)
    draft = synth.mutate(rng, genome, 0.01, 0.008, 0.008)
    err = (0.04, 0.03, 0.03)
    lens = []
    while sum(lens) < 12 * len(genome):
        lens.append(int(np.clip(rng.lognormal(np.log(8000), 0.5), 1000, 40_000)))
    short = _reads(rng, genome, lens, err)
    ul = _reads(rng, genome, [250_000, 300_000, 360_000, 450_000, 520_000, 600_000], err)
    targets = seqio.pack_reads([draft])

    def round_of(read_list):
        eng = hip.Engine(15, 5)
        rs = seqio.pack_reads(read_list)
        t0 = time.time()
        _, _, st = eng.polish_round(eng.upload(targets), eng.upload(rs))
        return eng.polish_layers(), st, time.time() - t0

    lay_all, st_all, s_all = round_of(short + ul)
    lay_short, st_short, s_short = round_of(short)
    print("ultra-long round: align_ms %.1f with the ultra-long reads (round %.2f s), %.1f without (round %.2f s)"
          % (st_all["align_ms"], s_all, st_short["align_ms"], s_short))
    assert st_all["n_dropped_layers"] == 0 and st_all["n_aligned"] == st_all["n_reads_used"]
    ns = len(short)
    keep = lay_all[:, 1] < ns
    assert np.array_equal(lay_all[keep], lay_short)
    w = 500
    for x, r in enumerate(ul):
        rows = lay_all[lay_all[:, 1] == ns + x]
        assert len(np.unique(rows[:, 0])) >= 0.8 * len(r) / w, (x, len(np.unique(rows[:, 0])), len(r))
