"""Crafted reads for the sketch stage (sketch.hip: sketch_kernel, minhash_select_kernel, compact_sketch_kernel,
gather_u32_kernel, sketch_flag_queries, pack_codes_kernel; abi_shard.hip: rvn_shard_sketch_range and its pieces) and the
plain reference they are held to.

The reference is tests/refimpl.py::brute_sketch read by read; nothing here restates the winnowing.  What this module adds
is the way to the inputs that random reads never give:

* ram's hash is a bijection on 2k bits and can be inverted (`unhash`), so a k-mer with a chosen hash value can be planted
  (`plant`): about half of all values have a preimage that is the canonical strand.
* every generator asserts, from brute_sketch alone, that the read it built is what its case is named after
  (`select_profile`: R, n, the threshold T, its ties, the digit and the fill of every radix pass).
* the random draws a generator needed (a seed, some lengths) are searched once (`python -m tests.sketch_cases`) and kept in
  tests/golden/sketch_case_seeds.json; loading a case builds it from there and asserts it again, so a recorded draw that no
  longer gives the case fails loudly.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

from raven_amd import seqio
from tests import refimpl

U64 = np.uint64
TILE = 1024                      # kSketchTile
CHUNK = 256                      # entries per trip of the ordered flag pass (= kThreads)
WINDOWS = (1, 2, 5, 10, 33, 256)
KS = (2, 4, 8, 12, 13, 15, 16, 17, 23, 28, 29, 31)   # every byte width of the select, both sides of the u32 / u64 switch
QUERY_FLAG = 1 << 63
FOREIGN_FLAG = 1 << 62
SEEDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sketch_case_seeds.json")


def nbytes(k):
    return (2 * k + 7) // 8


def max_digit(k, b):
    """Largest digit of byte b of a 2k-bit value."""
    return min(255, ((1 << (2 * k)) - 1) >> (8 * b))


def digit(v, b):
    return (int(v) >> (8 * b)) & 0xFF


# ---- the hash and its inverse ------------------------------------------------------------------------------------------

def _unxorshift(y, s, bits):
    x = y
    for _ in range(bits // s + 1):
        x = y ^ (x >> s)
    return x


def unhash(v, k):
    """The key with refimpl._hash(key, 4^k - 1) == v: the three odd multipliers 2^21 - 1, 265, 21 and the factor
    1 + 2^31 inverted modulo 4^k, the three xor-shifts undone from the top."""
    bits = 2 * k
    M = 1 << bits
    x = int(v)
    assert 0 <= x < M
    x = x * pow(1 + (1 << 31), -1, M) % M
    x = _unxorshift(x, 28, bits)
    x = x * pow(21, -1, M) % M
    x = _unxorshift(x, 14, bits)
    x = x * pow(265, -1, M) % M
    x = _unxorshift(x, 24, bits)
    return (x + 1) * pow((1 << 21) - 1, -1, M) % M    # ~key + (key << 21) = key * (2^21 - 1) - 1


def kmer_codes(x, k):
    """The k-mer whose forward register (first base in the top bits) is x."""
    return np.array([(int(x) >> (2 * (k - 1 - j))) & 3 for j in range(k)], dtype=np.uint8)


def kmer_value(codes):
    v = 0
    for c in codes:
        v = (v << 2) | int(c)
    return v


def revcomp(codes):
    return (3 - np.asarray(codes, dtype=np.uint8)[::-1]).astype(np.uint8)


def is_usable(v, k):
    """Is the preimage of v the canonical strand of its k-mer (strictly smaller than its reverse complement)?"""
    x = unhash(v, k)
    return x < kmer_value(revcomp(kmer_codes(x, k)))


def plant(values, k, strands=0):
    """(k-mers, values used): for every value whose preimage is canonical the k-mer with that hash — as it is (strand 0)
    or reverse-complemented (strand 1; `strands` is one number or one per value).  The other values are left out."""
    kmers, used = [], []
    for i, v in enumerate(values):
        if not is_usable(v, k):
            continue
        c = kmer_codes(unhash(v, k), k)
        s = strands if np.isscalar(strands) else strands[i]
        kmers.append(revcomp(c) if s else c)
        used.append(int(v))
    return kmers, used


def usable_below(limit, k, count, rng=None, lo=0):
    """`count` distinct usable values in [lo, limit): the smallest ones, or a random draw."""
    out = []
    if rng is None:
        v = lo
        while len(out) < count and v < limit:
            if is_usable(v, k):
                out.append(v)
            v += 1
    else:
        seen = set()
        tries = 0
        while len(out) < count and tries < 50 * count + 1000:
            tries += 1
            v = lo + int(rng.integers(0, 1 << 62)) % max(limit - lo, 1)
            if v not in seen and is_usable(v, k):
                seen.add(v)
                out.append(v)
    assert len(out) == count, "not enough usable values in [%d, %d) at k = %d" % (lo, limit, k)
    return out


def smallest_usable(k):
    return usable_below(1 << (2 * k), k, 1)[0]


# ---- the reference -----------------------------------------------------------------------------------------------------

def raw_and_kept(codes, k, w, read_id=0):
    """(values, origins, kept): the raw sketch of one read and which of its entries Minimize(seq, minhash = true) keeps,
    both from brute_sketch (origins are unique within a read, so the kept ones are found by origin)."""
    v, o = refimpl.brute_sketch(np.asarray(codes, dtype=np.uint8), k, w, read_id, False)
    _, mo = refimpl.brute_sketch(np.asarray(codes, dtype=np.uint8), k, w, read_id, True)
    return v, o, np.isin(o, mo)


class CaseSet:
    """One read set of one (k, w) with the names of its reads and the reference of any range of it."""

    def __init__(self, name, k, w, reads, names=None, ids=None):
        self.name, self.k, self.w = name, k, w
        self.reads = [np.ascontiguousarray(r, dtype=np.uint8) for r in reads]
        self.names = list(names) if names is not None else ["%s[%d]" % (name, i) for i in range(len(reads))]
        assert len(self.names) == len(self.reads)
        self.ids = np.arange(len(reads), dtype=np.uint32) if ids is None else np.asarray(ids, dtype=np.uint32)
        self._raw = {}

    @property
    def n(self):
        return len(self.reads)

    @functools.cached_property
    def rs(self):
        return seqio.pack_reads(self.reads, ids=self.ids)

    def raw(self, i):
        if i not in self._raw:
            self._raw[i] = raw_and_kept(self.reads[i], self.k, self.w, int(self.ids[i]))
        return self._raw[i]

    def reference(self, first=0, last=None, minhash=False, flags=False):
        """(values, origins, read offsets) of reads [first, last).  flags: the raw entries with bit 63 on the kept ones."""
        last = self.n if last is None else last
        vs, os_, off = [np.zeros(0, U64)], [np.zeros(0, U64)], [0]
        for i in range(first, last):
            v, o, kept = self.raw(i)
            if flags:
                o = o | (kept.astype(U64) << U64(63))
            elif minhash:
                v, o = v[kept], o[kept]
            vs.append(v)
            os_.append(o)
            off.append(off[-1] + v.shape[0])
        return np.concatenate(vs), np.concatenate(os_), np.array(off, dtype=np.uint32)

    def n_kept(self, first=0, last=None):
        last = self.n if last is None else last
        return int(sum(int(self.raw(i)[2].sum()) for i in range(first, last)))


def compare(got, want, names=None, first=0):
    """Mismatches between two (values, origins[, read offsets]): the first difference of every field, with the read it
    falls into.  Empty list == equal in every field, order included.  `got` without offsets: they are not compared."""
    errs = []
    gv, go = np.asarray(got[0]), np.asarray(got[1])
    wv, wo, woff = np.asarray(want[0]), np.asarray(want[1]), np.asarray(want[2]).astype(np.int64)

    def where(j):
        r = min(max(int(np.searchsorted(woff, j, side="right")) - 1, 0), max(woff.shape[0] - 2, 0))
        return "read %d%s entry %d" % (first + r, " (%s)" % names[first + r] if names else "", j - int(woff[r]))

    if len(got) > 2:
        goff = np.asarray(got[2]).astype(np.int64)
        if goff.shape != woff.shape:
            errs.append("read offsets: %d entries, want %d" % (goff.shape[0], woff.shape[0]))
        else:
            d = np.nonzero(goff != woff)[0]
            if d.size:
                errs.append("read offsets differ at %d: got %s want %s" % (int(d[0]), goff[d[0]:d[0] + 3].tolist(), woff[d[0]:d[0] + 3].tolist()))
    for what, g, wt in (("values", gv, wv), ("origins", go, wo)):
        if g.shape != wt.shape:
            errs.append("%s: %d entries, want %d" % (what, g.shape[0], wt.shape[0]))
        m = min(g.shape[0], wt.shape[0])
        d = np.nonzero(g[:m].astype(U64) != wt[:m].astype(U64))[0]
        if d.size:
            j = int(d[0])
            errs.append("%s differ at %d (%s): got %#x want %#x" % (what, j, where(j), int(g[j]), int(wt[j])))
    return errs


# ---- what the select does on a read, from brute_sketch -----------------------------------------------------------------

def select_profile(codes, k, w):
    """The quantities minhash_select_kernel works with on this read: n raw entries, R = min(n, len / k), the threshold
    T = the R-th smallest value, `nxt` = the R + 1-th, `t` entries equal to T at raw indices `tie_idx` of which the first
    `rem` are kept, `decide` = the highest byte in which T and nxt differ (-1: they are equal) and per radix pass b
    (`passes[b]`): T's digit, `rem` on entry, the entries of T's prefix group with a smaller (`lt`) / smaller or equal
    (`le`) digit and the histogram of the group."""
    vals, org, kept = raw_and_kept(codes, k, w)
    n = int(vals.shape[0])
    R = min(n, len(codes) // k)
    p = dict(n=n, R=R, len_over_k=len(codes) // k, vals=vals, org=org, kept=kept, T=None, nxt=None, t=0, rem=0, decide=None,
             tie_idx=np.zeros(0, np.int64), passes={})
    if R == 0 or n == 0:
        return p
    s = sorted(int(x) for x in vals)
    T = s[R - 1]
    p["T"] = T
    p["nxt"] = s[R] if R < n else None
    p["tie_idx"] = np.nonzero(vals == U64(T))[0]
    p["t"] = int(p["tie_idx"].shape[0])
    p["below"] = sum(1 for x in s if x < T)
    p["rem"] = R - p["below"]
    p["tie_strands"] = (org[p["tie_idx"]] & U64(1)).astype(np.int64)
    if p["nxt"] is not None:
        x = T ^ p["nxt"]
        p["decide"] = (x.bit_length() - 1) // 8 if x else -1
    for b in range(nbytes(k)):
        hi = T >> (8 * (b + 1))
        group = [x for x in s if x >> (8 * (b + 1)) == hi]
        rem_b = R - sum(1 for x in s if x >> (8 * (b + 1)) < hi)
        hist = np.bincount([digit(x, b) for x in group], minlength=256)
        d = digit(T, b)
        p["passes"][b] = dict(digit=d, rem=rem_b, lt=int(hist[:d].sum()), le=int(hist[:d + 1].sum()), hist=hist)
        assert p["passes"][b]["lt"] < rem_b <= p["passes"][b]["le"]
    return p


def pal_positions(codes, k):
    """Boolean per k-mer position: is the k-mer its own reverse complement (canonical_hash returns false)?"""
    c = np.asarray(codes, dtype=np.uint8)
    P = c.shape[0] - k + 1
    if P <= 0:
        return np.zeros(0, bool)
    out = np.ones(P, bool)
    for j in range(k):
        out &= c[j:j + P] == 3 - c[k - 1 - j:k - 1 - j + P]
    return out


def runs_of(mask):
    """[(first, length)] of the runs of True."""
    m = np.concatenate([[False], np.asarray(mask, bool), [False]])
    d = np.diff(m.astype(np.int8))
    return list(zip(np.nonzero(d == 1)[0].tolist(), (np.nonzero(d == -1)[0] - np.nonzero(d == 1)[0]).tolist()))


# ---- recorded draws ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _seeds():
    with open(SEEDS_PATH) as f:
        return json.load(f)


def _draw(name):
    s = _seeds()
    assert name in s, "no recorded draw for %s: run python -m tests.sketch_cases" % name
    return s[name]


def _rng(*key):
    return np.random.default_rng([int(x) for x in key])


def _bases(rng, n):
    return rng.integers(0, 4, size=int(n), dtype=np.uint8)


# ---- family select_byte ------------------------------------------------------------------------------------------------
# Pass b of the MSD radix select separates kept from dropped where the R-th and the R + 1-th smallest raw value agree in
# every byte above b and differ in byte b.  A read of `kSelSlots` planted k-mers has R = kSelSlots, and at least one raw
# value that is not planted lies below T (R planted values cannot all be kept and leave a planted R + 1-th), so T sits
# where the read's other minimizers begin: its upper bytes are drawn at that magnitude, byte b gets the wanted digit.

SEL_W = {8: 5, 12: 2, 13: 5, 15: 5, 16: 5, 17: 10, 23: 5, 28: 10, 29: 5, 31: 5}
kSelSlots = 40


def select_specs():
    """(name, k, b, d, kind).  kind: `exact` — pass b decides, T's digit there is d and the entries up to that digit are
    exactly what is still wanted (cum + h == rem); `carry` — the same with d = 255, so the R + 1-th value opens the next
    prefix; `plus` — one entry more than wanted up to T's digit (the cut falls inside the digit: a lower pass or the tie
    pass decides); `minus` — the digit before T's is occupied and ends one short of what is wanted; `top` — T's digit in
    the first pass is the largest a 2k-bit value has there."""
    out = []
    for k in KS:
        nb = nbytes(k)
        for b in range(nb):
            top, md = b == nb - 1, max_digit(k, b)
            digits = sorted({x for x in (0, 3, 4, 252, 255) if x <= md} | {md})
            if nb == 1:  # the value is the digit: only values whose preimage is a canonical strand occur at all
                digits = [x for x in digits if is_usable(x, k)]
            for d in digits:
                kind = "top" if (top and d == md) else ("carry" if d == 255 else "exact")
                if k == 4 and kind == "top":  # T = 255 = the largest value there is: every dropped entry would be 255 too
                    continue
                out.append(("select_byte:k%d:b%d:d%d:%s" % (k, b, d, kind), k, b, d, kind))
            pm = 4 if md >= 5 else 1
            if nb == 1:  # (two neighbouring usable values)
                pairs = [x for x in range(1, md + 1) if is_usable(x, k) and is_usable(x - 1, k)]
                pm = min(pairs, key=lambda x: abs(x - pm)) if pairs else None
            for kind in ("plus", "minus"):
                if pm is None:  # (k = 2: no two neighbouring values are both usable)
                    continue
                if kind == "minus" and (k, b) in ((17, 4), (29, 7)):
                    # T alone in the second quarter of the range with every dropped minimizer in the upper half: window
                    # minima are hardly ever there, no draw was found (k = 13 has this case on a top byte of two bits,
                    # k = 16 and 28 on a full top byte)
                    continue
                out.append(("select_byte:k%d:b%d:d%d:%s" % (k, b, pm, kind), k, b, pm, kind))
    return out


def select_check(codes, k, w, b, d, kind):
    """Is this read the case (k, b, d, kind)?  From brute_sketch alone."""
    p = select_profile(codes, k, w)
    if p["T"] is None or not p["R"] < p["n"]:
        return False
    ps = p["passes"][b]
    if ps["digit"] != d:
        return False
    fill = ps["le"] - ps["rem"]
    if kind == "top":
        return d == max_digit(k, b) and b == nbytes(k) - 1
    if kind == "exact":
        return p["decide"] == b and fill == 0
    if kind == "carry":
        return p["decide"] is not None and p["decide"] > b and fill == 0
    if kind == "plus":
        return fill == 1 and (p["decide"] == -1 if b == 0 else 0 <= p["decide"] < b)
    if kind == "minus":
        return d >= 1 and p["decide"] == b and fill == 0 and ps["hist"][d - 1] >= 1 and ps["lt"] == ps["rem"] - 1
    raise ValueError(kind)


def _sel_planted(k, w, b, d, kind, seed, c):
    """(read, u): kSelSlots planted k-mers in random order and on random strands — c of them above the threshold u (the
    R + 1-th value first among them), the others at or below it.  None where the draw has no room."""
    rng = _rng(seed, k, b, d)
    M, nb = 1 << (2 * k), nbytes(k)
    low = (1 << (8 * b)) - 1
    md = max_digit(k, b)

    def rand_low(bits):
        return int(rng.integers(0, 1 << 62)) & ((1 << bits) - 1)

    def usable_in(hi_part, dg, tries=64):
        for _ in range(tries):
            v = hi_part | (dg << (8 * b)) | rand_low(8 * b)
            if v < M and is_usable(v, k):
                return v
            if b == 0:
                return None
        return None

    if b == nb - 1:
        hi = 0
    else:
        n_junk = kSelSlots * k * 2.0 / (w + 1)
        u0 = int(M * (2.5 / n_junk) * (0.6 + 0.8 * rng.random()))
        hi = (u0 >> (8 * (b + 1))) << (8 * (b + 1))
        if n_junk * w * (hi | d << (8 * b)) < 1.5 * M:   # (hardly any other minimizer would lie below: one step up)
            hi += 1 << (8 * (b + 1))
    u = usable_in(hi, d)
    if u is None:
        return None
    small, large = [u], []
    if kind == "plus":
        if b == 0:
            small.append(u)
        else:
            u2 = u + 1
            while u2 & low and not is_usable(u2, k):
                u2 += 1
            if not u2 & low:
                return None
            small.append(u2)
    if kind == "minus":
        um = usable_in(hi, d - 1)
        if um is None:
            return None
        small.append(um)
    if kind == "carry":
        base = hi + (1 << (8 * (b + 1)))
        nx = None
        for _ in range(64):
            v = base | rand_low(8 * (b + 1))
            if v < M and is_usable(v, k):
                nx = v
                break
    else:
        nx = None
        for dd in range(d + 1, min(md, d + 3) + 1):
            nx = usable_in(hi, dd)
            if nx is not None:
                break
    if nx is None or nx <= max(small):
        return None
    large.append(nx)
    n_small = kSelSlots - c - len(small)
    if c < 1 or n_small < 0 or u < 8 * n_small + 8 or M - nx < 8 * c + 8:
        return None
    taken = set(small)
    for v in usable_below(u, k, n_small + len(small), rng):
        if v not in taken and len(small) < kSelSlots - c:
            small.append(v)
            taken.add(v)
    for v in usable_below(M, k, c + 1, rng, lo=nx + 1):
        if len(large) < c:
            large.append(v)
    if len(small) + len(large) != kSelSlots:
        return None
    values = small + large
    strands = rng.integers(0, 2, size=len(values)).tolist()
    kmers, used = plant(values, k, strands)
    assert used == values
    order = rng.permutation(len(kmers))
    return np.concatenate([kmers[i] for i in order]), u


def _sel_random(k, b, d, seed):
    """(read, w): a short random read and a window length, with up to two copies of a k-mer whose value has digit d in
    byte b written into it — for the cases a read of planted k-mers cannot reach (k <= 4: the value space is smaller than
    a read's sketch; T in the upper part of the range: nearly every other minimizer lies below it)."""
    rng = _rng(seed, k, b, d, 77)
    w = int(WINDOWS[int(rng.integers(0, len(WINDOWS)))])
    n = k + w - 1 + int(rng.integers(1, (1, 2, 4, 8, 24)[int(rng.integers(0, 5))] * k))
    codes = _bases(rng, n)
    above = 2 * k - 8 * (b + 1)
    v = (int(rng.integers(0, 1 << 62)) & ((1 << max(above, 0)) - 1)) << (8 * (b + 1)) | d << (8 * b) | \
        (int(rng.integers(0, 1 << 62)) & ((1 << (8 * b)) - 1))
    copies = int(rng.integers(0, 3))
    if v < (1 << (2 * k)) and is_usable(v, k):
        kmer = plant([v], k)[0][0]
        for _ in range(copies):
            at = int(rng.integers(0, n - k + 1))
            codes[at:at + k] = kmer if rng.integers(0, 2) else revcomp(kmer)
    return codes, w


def _sel_pair(k, b, d, seed):
    """(read, 1): k + 1 bases at w = 1 — two k-mer positions, both minimizers, R = 1: T is the smaller value and the
    other one is the R + 1-th.  One of them is a planted value with digit d in byte b (the top byte, or the one below a
    top byte of two bits); the base before or behind it is drawn.  Reaches the upper digits there, where any longer read
    has too many minimizers below T."""
    rng = _rng(seed, k, b, d, 78)
    v = d << (8 * b) | (int(rng.integers(0, 1 << 62)) & ((1 << (8 * b)) - 1))
    v |= int(rng.integers(0, 1 << max(2 * k - 8 * (b + 1), 0))) << (8 * (b + 1))
    if not is_usable(v, k):
        return None
    kmer = plant([v], k, int(rng.integers(0, 2)))[0][0]
    base = np.array([rng.integers(0, 4)], dtype=np.uint8)
    return (np.concatenate([kmer, base]) if rng.integers(0, 2) else np.concatenate([base, kmer])), 1


def _sel_search(k, b, d, kind, max_seeds=4000):
    if k in SEL_W:
        w = SEL_W[k]
        for seed in range(60):
            c = 2
            for _ in range(5):
                got = _sel_planted(k, w, b, d, kind, seed, c)
                if got is None:
                    break
                codes, u = got
                if select_check(codes, k, w, b, d, kind):
                    return dict(mode="planted", seed=seed, c=c)
                p = select_profile(codes, k, w)
                cnt = int((p["vals"] <= U64(u | ((1 << (8 * b)) - 1))).sum())
                c2 = c + cnt - (p["len_over_k"] + (1 if kind == "plus" else 0))
                if c2 == c or not 1 <= c2 < kSelSlots - 3:
                    break
                c = c2
    if 2 * k - 8 * (b + 1) <= 2:
        for seed in range(max_seeds):
            got = _sel_pair(k, b, d, seed)
            if got is not None and select_check(got[0], k, got[1], b, d, kind):
                return dict(mode="pair", seed=seed)
    for seed in range(max_seeds):
        codes, w = _sel_random(k, b, d, seed)
        if select_check(codes, k, w, b, d, kind):
            return dict(mode="random", seed=seed)
    return None


def select_read(name, k, b, d, kind):
    """(read, w) of one select_byte case from its recorded draw, asserted to be the case."""
    dr = _draw(name)
    if dr["mode"] == "planted":
        w = SEL_W[k]
        codes = _sel_planted(k, w, b, d, kind, dr["seed"], dr["c"])[0]
    elif dr["mode"] == "pair":
        codes, w = _sel_pair(k, b, d, dr["seed"])
    else:
        codes, w = _sel_random(k, b, d, dr["seed"])
    assert select_check(codes, k, w, b, d, kind), name
    return codes, w


# ---- family ties -------------------------------------------------------------------------------------------------------
# t raw entries equal to T of which the first `rem` by position are kept.  Planted k-mers cannot give rem < t (a planted
# tie costs k bases, that is one unit of R each); a run of C does: every position of it has the value of C^k, each costs
# one base, all are minimizers (the run holds a whole window) and they are neighbours in the sketch.  G^k is the same
# k-mer on the other strand.  A run of A in front gives entries ABOVE T for one base each and so moves the ties' raw
# indices; random bases behind the run give entries below T (a minimizer is the smallest of its window) and units of R,
# which of the two faster depends on w: at w = 256 they raise rem, so rem can reach t.

A_, C_, G_ = 0, 1, 2
_STREAM = 32768


def run_value(k, base=C_):
    return int(refimpl._hash(np.array([kmer_value([base] * k)], dtype=U64), (1 << (2 * k)) - 1)[0])


def ties_build(k, x, l1, l2, c, seed):
    post = _bases(_rng(seed, k, 6), _STREAM)[:c]
    return np.concatenate([np.full(x, A_, np.uint8), np.full(l1, C_, np.uint8), np.full(l2, G_, np.uint8), post])


TIES = tuple((k, w, kind) for k in (15, 31) for w, kinds in (
    (5, ("rem1",)), (33, ("cut:255", "cut:256", "cut:511", "cut:512")),
    (256, ("rem_t-1", "rem_t", "carry:256", "carry:512", "strands"))) for kind in kinds)


def ties_specs():
    return [("ties:k%d:w%d:%s" % (k, w, kind), k, w, kind) for k, w, kind in TIES]


def ties_check(codes, k, w, kind):
    assert run_value(k, A_) > run_value(k)
    p = select_profile(codes, k, w)
    if p["T"] != run_value(k) or not p["R"] < p["n"]:
        return False
    t, rem, idx = p["t"], p["rem"], p["tie_idx"]
    if kind == "strands":            # kept ties on both strands, and the cut between two ties of the second strand
        st = p["tie_strands"]
        return rem < t and st[0] == 0 and st[rem - 1] == 1 and st[rem] == 1
    if not (np.diff(idx) == 1).all():   # the ties are neighbours in the sketch
        return False
    if kind == "rem1":
        return rem == 1 and t >= 3
    if kind == "rem_t-1":
        return rem == t - 1 and t >= 4
    if kind == "rem_t":
        return rem == t and t >= 4
    if kind.startswith("cut:"):      # the last tie kept sits at raw index E, the first one dropped at E + 1
        return 2 <= rem < t and int(idx[rem - 1]) == int(kind[4:]) and int(idx[rem]) == int(kind[4:]) + 1
    if kind.startswith("carry:"):    # s_run goes through rem / 256 chunks before the cut
        return int(kind[6:]) < rem < t and int(idx[0]) < CHUNK
    raise ValueError(kind)


def _ties_search(k, w, kind):
    g = 1.0 / k - 2.0 / (w + 1)      # rem per random base behind the run

    def walk(l1, l2, want, seed, x=0):    # move c until rem is what `want` makes of the profile
        c = max(int((want(None) - (x + l1 + l2) / k) / g), 0)
        seen = set()
        for _ in range(40):
            if c in seen or not 0 <= c <= 24000 - x - l1 - l2:
                return None
            seen.add(c)
            codes = ties_build(k, x, l1, l2, c, seed)
            if ties_check(codes, k, w, kind):
                return dict(x=x, l1=l1, l2=l2, c=c, seed=seed)
            p = select_profile(codes, k, w)
            if p["T"] != run_value(k):
                return None
            diff = want(p) - p["rem"]
            c += int(round(diff / g)) if abs(diff) > 2 else (k if diff > 0 else -k) if diff else 1
        return None

    for seed in range(8):
        if kind == "rem1":
            grid = [(0, l1, 0, c) for l1 in range(k + 6, 2 * k) for c in (0, 1, 2)]
        elif kind.startswith("cut:"):
            x0 = int((int(kind[4:]) + k - 1200 / k) / (1 + 1.0 / k))
            grid = [(x, l1, 0, 0) for x in range(x0 - 30, x0 + 30) for l1 in range(1200, 1200 + k, 2)]
        else:
            grid = []
            l = k + w + 4
            if kind == "rem_t":
                # (everything the random bases add lies below T: without the run of A in front nothing would be dropped)
                got = walk(l, 0, lambda p: p["t"] if p else l - k + 1, seed, x=k + w - 1)
            elif kind == "rem_t-1":
                got = walk(l, 0, lambda p: p["t"] - 1 if p else l - k, seed)
            elif kind.startswith("carry:"):
                got = walk(int(kind[6:]) + 400, 0, lambda p: int(kind[6:]) + 12, seed)
            else:
                got = walk(l + 20, l + 20, lambda p: l + 20 - k + 1 + 30, seed)
            if got:
                return got
        for x, l1, l2, c in grid:
            if ties_check(ties_build(k, x, l1, l2, c, seed), k, w, kind):
                return dict(x=x, l1=l1, l2=l2, c=c, seed=seed)
    return None


def ties_read(name, k, w, kind):
    d = _draw(name)
    codes = ties_build(k, d["x"], d["l1"], d["l2"], d["c"], d["seed"])
    assert ties_check(codes, k, w, kind), name
    return codes


# ---- family keep_all ---------------------------------------------------------------------------------------------------
# R against n: R == n and R == n + 1 (the min caps it) return before the select, R == n - 1 drops exactly the largest
# value.  Random bases give n below len / k at w = 33; a run of C behind them adds one entry per base, so any n is reached.

KEEP_KW = ((15, 33), (17, 33))     # a u32 engine and a u64 one


def keep_build(k, L, x, seed):
    return np.concatenate([_bases(_rng(seed, k, 9), _STREAM)[:L - x], np.full(x, C_, np.uint8)])


def keep_specs():
    return [("keep_all:k%d:w%d:n%d:R%+d" % (k, w, n, dr), k, w, n, dr) for k, w in KEEP_KW for n in (255, 256, 257)
            for dr in (-1, 0, 1)]


def keep_check(codes, k, w, n, dr):
    p = select_profile(codes, k, w)
    return p["n"] == n and p["len_over_k"] == n + dr and p["R"] == min(n, n + dr)


def _keep_search(k, w, n, dr):
    for seed in range(4):
        for L in range(k * (n + dr), k * (n + dr + 1)):
            for x in range(0, 120):
                if keep_check(keep_build(k, L, x, seed), k, w, n, dr):
                    return dict(L=L, x=x, seed=seed)
    return None


def keep_read(name, k, w, n, dr):
    d = _draw(name)
    codes = keep_build(k, d["L"], d["x"], d["seed"])
    assert keep_check(codes, k, w, n, dr), name
    return codes


def keep_small_reads(k, w):
    """[(name, read)]: n = 1 with R = 1 or 2 (one window; R = 0 needs len < k, which has no entry at all), and a read of
    k + w - 2 bases — R >= 1 and no full window — between two ordinary reads."""
    rng = _rng(k, w, 10)
    out = []
    for L in range(k + w - 1, k + w + 8):
        r = _bases(rng, L)
        p = select_profile(r, k, w)
        if p["n"] == 1 and not any(nm.endswith("R%d" % p["len_over_k"]) for nm, _ in out):
            out.append(("keep_all:k%d:w%d:n1:R%d" % (k, w, p["len_over_k"]), r))
    assert out, "no read with a single minimizer"
    mid = _bases(rng, k + w - 2)
    pm = select_profile(mid, k, w)
    assert pm["n"] == 0 and pm["len_over_k"] >= 1
    a, b = _bases(rng, 700), _bases(rng, 1300)
    assert select_profile(a, k, w)["n"] > 0 and select_profile(b, k, w)["n"] > 0
    return out + [("keep_all:k%d:w%d:before" % (k, w), a), ("keep_all:k%d:w%d:no_window" % (k, w), mid),
                  ("keep_all:k%d:w%d:behind" % (k, w), b)]


# ---- family palindromes (even k) ---------------------------------------------------------------------------------------
# (AT)^m is its own reverse complement around every gap between two bases, so for even k every k-mer of it is a palindrome:
# a run of r invalid positions takes r + k - 1 bases.  Two runs of two or more positions that are less than k - 1 valid
# positions apart would share two bases and be one run, except at k = 2 where AT | CG leaves the single valid position TC.

PAL_KW = ((2, 2), (4, 5), (12, 10), (16, 5), (28, 33))


def at_run(positions, k, first=0):
    """r + k - 1 bases of (AT)^m or (TA)^m."""
    return ((np.arange(positions + k - 1) + first) % 2 * 3).astype(np.uint8)


def _with_run(rng, k, before, r, behind):
    """Random bases around a run of exactly r palindromic positions that begins at position `before`; the neighbours of
    the run are redrawn until they do not lengthen it."""
    for _ in range(200):
        codes = np.concatenate([_bases(rng, before), at_run(r, k), _bases(rng, behind)])
        if (before, r) in runs_of(pal_positions(codes, k)):
            return codes
    raise AssertionError("no run of %d positions at %d" % (r, before))


def palindrome_reads(k, w):
    """[(name, read)] with every claim asserted here from pal_positions and brute_sketch."""
    assert k % 2 == 0
    rng = _rng(k, w, 11)
    out = []
    tag = "palindromes:k%d:w%d:" % (k, w)
    for r in sorted({w - 1, w, w + 1, 3 * w}):
        out.append((tag + "run%d" % r, _with_run(rng, k, 300, r, 300)))
    for q in (1023, 1024, 1025):
        out.append((tag + "first@%d" % q, _with_run(rng, k, q, w + 1, 1300)))
        out.append((tag + "last@%d" % q, _with_run(rng, k, q - w, w + 1, 1300)))
    out.append((tag + "halo", _with_run(rng, k, TILE - w, 2 * w + 1, 900)))   # left halo of tile 1, right halo of tile 0
    whole = at_run(1500 - k + 1, k)
    assert pal_positions(whole, k).all() and refimpl.brute_sketch(whole, k, w)[0].shape[0] == 0 and whole.shape[0] - k + 1 > TILE
    out.append((tag + "whole", whole))
    # a window of invalid positions and one valid one: that one is emitted whatever its value
    gap = 1 if k == 2 else k - 1
    for _ in range(200):
        cg = (1 + np.arange(w + k - 1) % 2).astype(np.uint8)
        codes = np.concatenate([_bases(rng, 200), at_run(w, k), cg, _bases(rng, 200)])
        runs = runs_of(pal_positions(codes, k))
        if (200, w) in runs and (200 + w + gap, w) in runs:
            break
    else:
        raise AssertionError("no two runs")
    pos = (refimpl.brute_sketch(codes, k, w)[1] >> U64(1)) & U64(0x7FFFFFFF)
    assert 200 + w in pos and 200 + w + gap - 1 in pos
    out.append((tag + "between%d" % gap, codes))
    # (ACGT)^m: every second position is a palindrome, the others are one k-mer on alternating strands
    alt = np.tile(np.array([0, 1, 2, 3], np.uint8), 300)
    pal = pal_positions(alt, k)
    v, o = refimpl.brute_sketch(alt, k, w)
    assert pal[::2].all() != pal[1::2].all() and np.unique(v).shape[0] == 1 and set((o & U64(1)).tolist()) == {0, 1}
    out.append((tag + "alternating", alt))
    return out


# ---- family tile_edges -------------------------------------------------------------------------------------------------

EDGE_KW = ((15, 5), (15, 33), (16, 10), (31, 256))


def _planted_at(rng, k, w, n, at, v):
    """A random read of n bases with the k-mer of value v at the positions `at`; v is asserted to be below every other
    value of the read, so it is the minimum of every window that holds it, and to be in the sketch at those positions."""
    kmer = plant([v], k)[0][0]
    for _ in range(50):
        codes = _bases(rng, n)
        for p in at:
            codes[p:p + k] = kmer
        vals, org = refimpl.brute_sketch(codes, k, 1)          # w = 1: every valid position
        pos = ((org >> U64(1)) & U64(0x7FFFFFFF)).astype(np.int64)
        if sorted(pos[vals == U64(v)].tolist()) == sorted(at) and (vals >= U64(v)).all():
            rv, ro = refimpl.brute_sketch(codes, k, w)
            rp = ((ro >> U64(1)) & U64(0x7FFFFFFF)).astype(np.int64)
            assert all(p in rp for p in at)
            return codes
    raise AssertionError("planted value not the minimum")


def tile_edge_reads(k, w):
    rng = _rng(k, w, 12)
    v0 = smallest_usable(k)
    tag = "tile_edges:k%d:w%d:" % (k, w)
    n = 2 * TILE + 300 + k
    out = []
    for p in sorted({TILE - 1, TILE, TILE - 1 + w - 1, TILE - w + 1}):
        out.append((tag + "v0@%d" % p, _planted_at(rng, k, w, n, [p], v0)))
    out.append((tag + "v0@last", _planted_at(rng, k, w, n, [n - k], v0)))
    out.append((tag + "v0@0", _planted_at(rng, k, w, n, [0], v0)))
    lo = TILE - 1 - (k - 1) // 2 if w > k else TILE - 3          # both sides of the edge; inside one window where w > k
    out.append((tag + "equal_across", _planted_at(rng, k, w, n, [lo, lo + k], v0)))
    assert lo < TILE <= lo + k
    for last in sorted({1, w - 1, w} - {0}):                       # positions in the last tile
        out.append((tag + "last_tile%d" % last, _bases(rng, TILE + last + k - 1)))
    for P in (TILE, 2 * TILE, 2 * TILE + 1):
        out.append((tag + "P%d" % P, _bases(rng, P + k - 1)))
    return out


# ---- family words ------------------------------------------------------------------------------------------------------

WORDS_KW = ((15, 5), (31, 10))
WORD_IDS = (7, 3, (1 << 30) - 1)


def words_set(k, w):
    """Read lengths 0, 1 and 31 modulo 32, a planted k-mer at bit 0 of a word and one that ends on a word's last bit, the
    same reads again behind reads of other lengths, the last read ending on a word boundary, ids that are no indices."""
    rng = _rng(k, w, 13)
    v0, v1 = usable_below(1 << (2 * k), k, 2)
    base = []
    for L in (320, 321, 351):
        at = [96, 160 - k]                                   # bases 96 .. : word 3 bit 0;  ... 159: last bit of word 4
        codes = _bases(rng, L)
        codes[at[0]:at[0] + k] = plant([v0], k)[0][0]
        codes[at[1]:at[1] + k] = plant([v1], k, 1)[0][0]
        vals, org = refimpl.brute_sketch(codes, k, w)
        pos = ((org >> U64(1)) & U64(0x7FFFFFFF)).astype(np.int64).tolist()
        assert at[0] in pos and at[1] in pos and (2 * at[0]) % 64 == 0 and (2 * (at[1] + k)) % 64 == 0
        base.append(codes)
    reads = base + [_bases(rng, 45)] + base + [_bases(rng, 1000)] + base[:1] + [_bases(rng, 33), _bases(rng, 32 * 70)]
    names = ["words:k%d:w%d:%d" % (k, w, i) for i in range(len(reads))]
    ids = [WORD_IDS[i % 3] if i < 3 else 1000 + 17 * i for i in range(len(reads))]
    cs = CaseSet("words:k%d:w%d" % (k, w), k, w, reads, names, ids)
    off = cs.rs.word_offsets
    assert {int(r.shape[0]) % 32 for r in base} == {0, 1, 31} and reads[-1].shape[0] % 32 == 0
    assert all(int(off[i]) % (TILE // 32) for i in (4, 5, 6, 8))   # the copies start inside a tile's worth of words
    return cs


# ---- family ranges -----------------------------------------------------------------------------------------------------

RANGES_KW = ((15, 5), (16, 5))


def ranges_set(k, w):
    """About 40 reads whose len / k differs from neighbour to neighbour, among them reads of 0, 1, k - 1 and k + w - 2
    bases (no tiles), singly, in a row of three, first and last."""
    rng = _rng(k, w, 14)
    short = [0, 1, k - 1, k + w - 2]
    lens = [k + w - 2]
    for i in range(36):
        lens.append(int(rng.integers(k + w - 1, 2700)))
        if i in (4, 11, 20):
            lens.append(short[(i // 4) % 4])
        if i == 15:
            lens += [0, k - 1, 1]
    lens.append(k - 1)
    reads = [_bases(rng, n) for n in lens]
    cs = CaseSet("ranges:k%d:w%d" % (k, w), k, w, reads)
    q = [n // k for n in lens]
    assert all(a != b for a, b in zip(q, q[1:]) if a and b)
    assert any(n > TILE + k + w for n in lens) and any(n > 2 * TILE + k for n in lens)
    return cs


def has_tiles(cs, i):
    return cs.reads[i].shape[0] >= cs.k + cs.w - 1


def ranges_of(cs):
    """[(first, last)]: the whole set, every single read, the empty range at every read, and around every stretch of
    reads without tiles: beginning / ending on it, just before it and just behind it, and the stretch alone."""
    n = cs.n
    out = [(0, n)] + [(i, i + 1) for i in range(n)] + [(i, i) for i in range(0, n + 1, 7)]
    for s, ln in runs_of([not has_tiles(cs, i) for i in range(n)]):
        e = s + ln
        out.append((s, e))
        for f in {max(s - 1, 0), s, min(s + 1, e), e}:
            for l in {min(e + 1, n), e, max(e - 1, s), s, min(e + 3, n)}:
                if f <= l:
                    out.append((max(f - 2, 0) if f == l else f, l))
        out += [(max(s - 3, 0), s), (max(s - 3, 0), s + 1), (e - 1, min(e + 2, n)), (e, min(e + 2, n))]
    return sorted(set(out))


# ---- pack_codes --------------------------------------------------------------------------------------------------------

def pack_codes_arrays():
    """{name: list of one-byte code arrays} for rvn_reads_upload_codes; values carry bits above the low two."""
    rng = _rng(15)
    lens = [0, 1, 31, 32, 33, 63, 64, 65, 1000]

    def arr(n):
        return rng.integers(0, 256, size=n, dtype=np.uint8)

    big = [0] + [int(x) for x in rng.choice(lens[1:], size=150)] + [0, 0, 0] + [int(x) for x in rng.choice(lens[1:], size=146)] + [0]
    return {"empty_set": [], "one_empty_read": [arr(0)], "lengths": [arr(n) for n in lens],
            "empty_first_middle_last": [arr(n) for n in big],
            "only_empty": [arr(0), arr(0), arr(0)], "one_word": [arr(32)], "words_33": [arr(33), arr(0), arr(31)]}


def pack_codes_reference(arrays):
    return seqio.pack_reads([np.asarray(a, dtype=np.uint8) & 3 for a in arrays])


# ---- all sets ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def family_sets(family):
    """The CaseSets of one family, built from the recorded draws with every generator's assertion run."""
    groups = {}

    def add(k, w, name, read):
        groups.setdefault((k, w), []).append((name, read))

    if family == "select_byte":
        for name, k, b, d, kind in select_specs():
            read, w = select_read(name, k, b, d, kind)
            add(k, w, name, read)
    elif family == "ties":
        for name, k, w, kind in ties_specs():
            add(k, w, name, ties_read(name, k, w, kind))
    elif family == "keep_all":
        for name, k, w, n, dr in keep_specs():
            add(k, w, name, keep_read(name, k, w, n, dr))
        for k, w in ((15, 5), (17, 33)):
            for name, read in keep_small_reads(k, w):
                add(k, w, name, read)
    elif family == "palindromes":
        for k, w in PAL_KW:
            for name, read in palindrome_reads(k, w):
                add(k, w, name, read)
    elif family == "tile_edges":
        for k, w in EDGE_KW:
            for name, read in tile_edge_reads(k, w):
                add(k, w, name, read)
    elif family == "words":
        return tuple(words_set(k, w) for k, w in WORDS_KW)
    elif family == "ranges":
        return tuple(ranges_set(k, w) for k, w in RANGES_KW)
    else:
        raise ValueError(family)
    return tuple(CaseSet("%s:k%d:w%d" % (family, k, w), k, w, [r for _, r in g], [nm for nm, _ in g])
                 for (k, w), g in sorted(groups.items()))


FAMILIES = ("select_byte", "ties", "keep_all", "palindromes", "tile_edges", "words", "ranges")
FLAG_FAMILIES = ("select_byte", "ties", "keep_all", "ranges")


def all_sets(families=FAMILIES):
    return [cs for f in families for cs in family_sets(f)]


def search_all(path=SEEDS_PATH):
    """Find every draw again and write the table (minutes; the tests only read it)."""
    out = {}
    for name, k, b, d, kind in select_specs():
        out[name] = _sel_search(k, b, d, kind)
    for name, k, w, kind in ties_specs():
        out[name] = _ties_search(k, w, kind)
    for name, k, w, n, dr in keep_specs():
        out[name] = _keep_search(k, w, n, dr)
    missing = [nm for nm, v in out.items() if v is None]
    with open(path, "w") as f:
        json.dump({nm: v for nm, v in out.items() if v is not None}, f, indent=0, sort_keys=True)
        f.write("\n")
    assert not missing, missing
    return out


if __name__ == "__main__":
    print("%d draws written" % len(search_all()))
