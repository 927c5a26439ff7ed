"""The lane-per-pair edit-distance kernel (raven_amd/csrc/edit_distance.hip: ed_lane_kernel<W>, W = 3 / 5 / 7 slots) and
its bounded mode against the textbook DP of the oracle, without a GPU: the per-pair body of the kernel is one
__host__ __device__ function with no cross-lane operation, and rvn_test_ed_lane calls that very function on the host.

For every pair, every window and every threshold the RAW value the kernel stores is predicted from the DP distance D and
a threshold k_W restated by brute force from the rule in the kernel's comment (tests/ed_lane_model.py; never from
ed_lane_threshold):
the exact D when D <= min(k_W, kmax), "above" when kmax decides, the window's overflow code otherwise — never a number
that is not D, and never an overflow where the window has to decide.  TextGroups (unaligned fetch, clipping at the
span's end, the reverse strand), PeqRaw (1 / 2 / 3-word loads, converted a cycle later), the moving window, the fits edge
and the three codes are what the shapes below are chosen for."""
import ctypes as C
import mmap
import os
import subprocess
import sys
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip, seqio, synth
from tests.ed_lane_model import expected, k_window  # (shared with tests/ed_ring_cases.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS = (3, 5, 7)
ABOVE = hip.ED_ABOVE
OVER = {3: hip.ED_OVERFLOW, 5: hip.ED_OVERFLOW, 7: hip.ED_OVERFLOW_WIDE}
INF = 1 << 40
THREADS = min(16, os.cpu_count() or 1)
DEC = np.frombuffer(b"ACGT", dtype=np.uint8)


def identity_kmax(n, m, identity):
    """The largest distance x that passes the reference's rule !(1. - x / max(len) < identity), in double."""
    maxlen = max(n, m)
    t, lo, hi = 0, 0, maxlen  # the rule is monotone in x
    while maxlen and lo <= hi:
        mid = (lo + hi) // 2
        if not (1. - float(mid) / float(maxlen) < identity):
            t, lo = mid, mid + 1
        else:
            hi = mid - 1
    return t


def _subs(rng, a, count):
    """`count` substitutions at positions at least 4 apart (isolated: the distance is then `count` but for rare luck)."""
    b = a.copy()
    count = max(count, 0)
    slots = rng.choice(len(a) // 6, size=count, replace=False) * 6 + rng.integers(0, 3, size=count)
    b[slots] = (b[slots] + rng.integers(1, 4, size=count)) & 3
    return b


def _cases():
    """[(a codes, b codes in a's orientation)]: the pattern and the text the DP sees."""
    rng = np.random.default_rng(20260)
    out = []
    # 1. lengths at the block / group boundaries, n and m independently (nb below, at and above W; d up to 609)
    edge = sorted({max(0, 64 * k + x) for k in range(10) for x in (-1, 0, 1, 31, 32, 33)} | {2})
    base = rng.integers(0, 4, size=700, dtype=np.uint8)
    noisy = synth.mutate(rng, base, 0.01, 0.005, 0.005)
    for n in edge:
        for m in edge:
            out.append((base[:n], noisy[:m]))
    # 2. random lengths up to ~4 kb, uniform noise 0.1 % .. 12 %
    for i in range(260):
        n = int(np.exp(rng.uniform(np.log(100), np.log(4000))))
        e = float(np.exp(rng.uniform(np.log(0.001), np.log(0.12))))
        a = rng.integers(0, 4, size=n, dtype=np.uint8)
        out.append((a, synth.mutate(rng, a, e / 2, e / 4, e / 4)))
    # 3. length differences at the slot and fits edges, both directions, the indels in one cluster or spread
    for d in (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385):
        for n in (d + 90, d + 700, d + 1500):
            a = rng.integers(0, 4, size=n, dtype=np.uint8)
            at = int(rng.integers(0, n - d + 1))
            keep = np.ones(n, bool)
            keep[rng.choice(n, size=d, replace=False)] = False
            for bb in (np.concatenate([a[:at], a[at + d:]]), a[keep]):
                bb = synth.mutate(rng, bb, 0.004, 0.0, 0.0)
                out.append((a, bb))
                out.append((bb, a))
    # 4. all indels in one cluster at the start / middle / end; balanced ones keep d = 0 and push the path to a band edge
    for g in (10, 60, 64, 100, 128, 190, 250, 380):
        for where in (0, 1, 2):
            n = int(rng.integers(g + 300, g + 1800))
            a = rng.integers(0, 4, size=n, dtype=np.uint8)
            at = (0, (n - g) // 2, n - g)[where]
            cut = np.concatenate([a[:at], a[at + g:]])
            fill = rng.integers(0, 4, size=g, dtype=np.uint8)
            bal = np.concatenate([cut, fill]) if where < 2 else np.concatenate([fill, cut])
            for bb in (cut, bal):
                out.append((a, bb))
                out.append((bb, a))
    # 5. distances at the window's threshold: D = k_W - 2 .. k_W + 2, with and without a length difference
    for W in WS:
        for d0 in (0, 10, 64, 100):
            for delta in (-2, -1, 0, 1, 2):
                n = 7 * 64 * W + d0
                a = rng.integers(0, 4, size=n, dtype=np.uint8)
                b = _subs(rng, a, k_window(n, n - d0, W) + delta - d0)
                at = int(rng.integers(0, n - d0 + 1)) // 6 * 6
                out.append((a, np.concatenate([b[:at], b[at + d0:]])))
    # 6. homopolymers and dinucleotide repeats against each other, identical spans, unrelated spans
    for n in (1, 31, 32, 33, 64, 65, 129, 300, 600):
        for m in (1, 33, 64, 127, 300, 590):
            out.append((np.zeros(n, np.uint8), np.tile(np.array([0, 1], np.uint8), m)[:m]))
            out.append((np.tile(np.array([1, 0], np.uint8), n)[:n], np.tile(np.array([0, 1], np.uint8), m)[:m]))
            out.append((np.full(n, 3, np.uint8), np.full(m, 3, np.uint8)))
    for n in (1, 32, 33, 64, 100, 513, 1000, 2000):
        a = rng.integers(0, 4, size=n, dtype=np.uint8)
        out.append((a, a.copy()))
    for i in range(30):
        out.append((rng.integers(0, 4, size=int(rng.integers(800, 1500)), dtype=np.uint8),
                    rng.integers(0, 4, size=int(rng.integers(800, 1500)), dtype=np.uint8)))
    return out


def _place(cases, seed, flush=False):
    """One read per span: flank + span + flank.  The begins run over all residues mod 32, some spans start at base 0 of
    their read, some (flush: all) end at its last base; strand 0 stores the reverse complement of b.  Returns (ReadSet,
    pairs, mask of the span bases in the packed stream)."""
    rng = np.random.default_rng(seed)
    reads, P, spans = [], [], []
    for i, (a, b) in enumerate(cases):
        strand = (i // 3 + i) & 1
        stored_b = b if strand else (3 - b[::-1])
        begins = [((i * 7 + 3) % 32 + 32 * (i % 3)) if i % 5 else 0, ((i * 11 + 5) % 32 + 32 * ((i // 3) % 3)) if i % 7 else 0]
        tails = [0 if (i % 4 == 0 or flush) else int(rng.integers(1, 45)), 0 if (i % 4 == 1 or flush) else int(rng.integers(1, 45))]
        for span, bg, tl in zip((a, stored_b), begins, tails):
            reads.append(np.concatenate([rng.integers(0, 4, size=bg, dtype=np.uint8), span.astype(np.uint8),
                                         rng.integers(0, 4, size=tl, dtype=np.uint8)]))
            spans.append((bg, len(span)))
        P.append((2 * i, begins[0], len(a), 2 * i + 1, begins[1], len(b), strand, 0))
    rs = seqio.pack_reads(reads)
    mask = np.zeros(rs.packed.shape[0] * 32, dtype=bool)
    for r, (bg, ln) in enumerate(spans):
        at = int(rs.word_offsets[r]) * 32 + bg
        mask[at:at + ln] = True
    return rs, np.array(P, dtype=hip.ED_PAIR_DTYPE), mask


def _scrambled(rs, mask, seed):
    """The packed words with every bit outside the spans replaced: neighbouring bases, the unused part of a read's last
    word and the pad word are what fetch / load_bases32 / PeqRaw read past a span."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 1 << 32, size=rs.packed.shape[0], dtype=np.uint64) << np.uint64(32) | \
        rng.integers(0, 1 << 32, size=rs.packed.shape[0], dtype=np.uint64)
    bits = np.repeat(mask, 2).reshape(-1, 64).astype(np.uint64)
    keep = np.bitwise_or.reduce(bits << np.arange(64, dtype=np.uint64)[None, :], axis=1)
    return (rs.packed & keep) | (noise & ~keep)


def _dp(case):
    return oracle.edit_distance(DEC[case[0]].tobytes(), DEC[case[1]].tobytes())


@pytest.fixture(scope="module")
def world():
    cases = _cases()
    with ThreadPoolExecutor(THREADS) as ex:
        D = list(ex.map(_dp, cases))
    rs, pairs, mask = _place(cases, seed=77)
    # kmax per pair: none, 0, 1, d - 1, d, D - 1, D, D + 1 and what the identity filter computes for 0.9 / 0.95 / 0.99
    n = pairs["lhs_len"].astype(np.int64)
    m = pairs["rhs_len"].astype(np.int64)
    d = np.abs(n - m)
    Dn = np.array(D, dtype=np.int64)
    variants = {"none": None, "0": np.zeros_like(d), "1": np.ones_like(d), "d-1": d - 1, "d": d, "D-1": Dn - 1, "D": Dn, "D+1": Dn + 1}
    for ident in (0.9, 0.95, 0.99):
        variants["id%g" % ident] = np.array([identity_kmax(int(x), int(y), ident) for x, y in zip(n, m)], dtype=np.int64)
    return dict(D=D, rs=rs, pairs=pairs, mask=mask, variants=variants)


def _want(world, W, name):
    km = world["variants"][name]
    res = []
    for i, p in enumerate(world["pairs"]):
        if km is not None and km[i] < 0:
            res.append(None)  # the variant does not exist for this pair (d - 1 of d = 0, D - 1 of D = 0)
            continue
        res.append(expected(int(p["lhs_len"]), int(p["rhs_len"]), world["D"][i], INF if km is None else int(km[i]), W))
    return res


def test_shapes_reach_every_outcome_and_the_threshold_edges(world):
    """From the oracle and this module's own k_W alone, before the kernel is looked at: every outcome occurs at least 20
    times for every window, distances sit on, just below and just above every window's threshold, every residue of the
    begins occurs, short and ragged texts occur on the reverse strand."""
    for W in WS:
        c = Counter()
        for name in world["variants"]:
            c.update(w[0] for w in _want(world, W, name) if w is not None)
        for outcome in ("empty", "d_above", "no_fit", "exact", "above", "overflow"):
            assert c[outcome] >= 20, (W, outcome, dict(c))
        near = Counter()
        for p, D in zip(world["pairs"], world["D"]):
            kw = k_window(int(p["lhs_len"]), int(p["rhs_len"]), W)
            if kw is not None and p["lhs_len"] and p["rhs_len"]:
                near[D - kw] += 1
        assert all(near[x] >= 2 for x in (-1, 0, 1)), (W, [near[x] for x in (-1, 0, 1)])
    P = world["pairs"]
    for key in ("lhs_begin", "rhs_begin"):
        assert set((P[key] % 32).tolist()) == set(range(32))
    rev = P[P["strand"] == 0]
    assert (rev["rhs_len"] < 32).sum() > 50 and ((rev["rhs_len"] % 32 != 0) & (rev["rhs_len"] > 32)).sum() > 500
    assert [k_window(100, 100, W) for W in WS] == [129, 257, 385]
    assert k_window(228, 100, 3) == 129 and k_window(229, 100, 3) is None and k_window(100, 485, 7) is None


@pytest.mark.parametrize("W", WS)
def test_lane_kernel_body_equals_the_dp_or_says_why_not(world, W):
    rs, pairs = world["rs"], world["pairs"]
    scrambled = _scrambled(rs, world["mask"], seed=5)

    def run(name):
        km = world["variants"][name]
        kmax = None if km is None else np.clip(km, 0, None).astype(np.uint32)
        return (name, hip.test_ed_lane(rs.packed, rs.word_offsets, pairs, W, kmax),
                hip.test_ed_lane(scrambled, rs.word_offsets, pairs, W, kmax))

    with ThreadPoolExecutor(THREADS) as ex:
        results = list(ex.map(run, world["variants"]))
    bad = []
    for name, got, got2 in results:
        for i, w in enumerate(_want(world, W, name)):
            if w is not None and (int(got[i]) != w[1] or int(got2[i]) != w[1]):
                bad.append((name, i, tuple(int(x) for x in pairs[i]), "D=%d" % world["D"][i], w, int(got[i]), int(got2[i])))
    assert not bad, (len(bad), bad[:12])


def test_equal_lengths_with_a_threshold_below_two():
    """Regression: spans of equal length with kmax 0 or 1 had a band with no row beside the diagonal; block 1 then came
    in after block 0 had left, took its entry bound from nothing, and the kernel stored 0 or 1 for a distance of 2 (an
    overlap of 84 .. 199 bases at --identity 0.99 was kept that the reference drops).  n = m = 65, D = 2."""
    a = np.tile(np.array([0, 1, 2, 3], np.uint8), 17)[:65]
    b = a.copy()
    b[[10, 40]] ^= 1
    assert _dp((a, b)) == 2
    rs, pairs, _ = _place([(a, b)], seed=1)
    for W in WS:
        for km, want in ((0, ABOVE), (1, ABOVE), (2, 2), (3, 2)):
            assert int(hip.test_ed_lane(rs.packed, rs.word_offsets, pairs, W, np.array([km], np.uint32))[0]) == want, (W, km)
        assert int(hip.test_ed_lane(rs.packed, rs.word_offsets, pairs[:1], W, np.array([0], np.uint32))[0]) == ABOVE
    same, p2, _ = _place([(a, a.copy())], seed=1)
    for W in WS:
        assert int(hip.test_ed_lane(same.packed, same.word_offsets, p2, W, np.array([0], np.uint32))[0]) == 0


def _guarded_copy(words, keep):
    """`words` copied so that its last word ends where a page the process may not touch begins."""
    page = mmap.PAGESIZE
    size = (words.nbytes + page - 1) // page * page + page
    mm = mmap.mmap(-1, size)
    keep.append(mm)
    addr = C.addressof(C.c_char.from_buffer(mm))
    assert C.CDLL(None).mprotect(C.c_void_p(addr + size - page), C.c_size_t(page), 0) == 0
    arr = np.frombuffer(mm, dtype=np.uint64, count=words.shape[0], offset=size - page - words.nbytes)
    arr[:] = words
    return arr


def _guarded_run():
    """Spans that end at the last base of the LAST read of the set, as the text and as the pattern, the packed words (one
    pad word behind the last read: what seqio.pack_reads provides and rvn_reads_upload guarantees) ending at an
    unreadable page: a read further out is a fault."""
    rng = np.random.default_rng(99)
    keep, done = [], 0
    for n in (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 300, 513, 545, 577, 609, 1000):
        a = rng.integers(0, 4, size=n, dtype=np.uint8)
        case = (a, synth.mutate(rng, a, 0.01, 0.005, 0.005))
        D = _dp(case)
        for copies in (1, 2, 3, 4, 6):  # the last pair of the set: both strands, several residues of the begins
            rs, pairs, _ = _place([case] * copies, seed=n + copies, flush=True)
            assert int(rs.word_offsets[-1]) + 1 == rs.packed.shape[0]
            words = _guarded_copy(rs.packed, keep)
            p = pairs[-1:].copy()
            q = p.copy()  # the same two spans with the roles exchanged: the pattern is the one in the last read
            for x, y in (("lhs_read", "rhs_read"), ("lhs_begin", "rhs_begin"), ("lhs_len", "rhs_len")):
                q[x], q[y] = p[y], p[x]
            for pr in (p, q):
                for W in WS:
                    got = int(hip.test_ed_lane(words, rs.word_offsets, pr, W)[0])
                    assert got == expected(int(pr[0]["lhs_len"]), int(pr[0]["rhs_len"]), D, INF, W)[1], (n, copies, pr, W, got, D)
                    done += 1
    return done


def test_reads_past_a_span_stay_inside_the_packed_buffer():
    """In a child process: an access beyond the pad word ends it with a signal instead of passing unnoticed."""
    script = "import sys; sys.path.insert(0, %r); from tests.test_ed_lane import _guarded_run; print('guarded ok', _guarded_run())" % ROOT
    run = subprocess.run([sys.executable, "-c", script], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "guarded ok 600" in run.stdout, (run.returncode, run.stdout[-500:], run.stderr[-2000:])
