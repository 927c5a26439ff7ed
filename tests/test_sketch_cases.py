"""The crafted reads of the sketch stage (tests/sketch_cases.py) on the CPU: the hash inverse against refimpl._hash and
against the product's canonical_hash (kmer.h through rvn_test_canonical, both value widths); every generator's assertion,
run from brute_sketch alone; oracle.Engine.sketch equal to the reference on every read of every family, raw and minhash,
values and origins; and the comparison helper shown to notice the faults a select or a compaction could make."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip, seqio
from tests import refimpl
from tests import sketch_cases as sc

U64 = np.uint64


@pytest.mark.parametrize("k", sc.KS + (5,))
def test_unhash_inverts_the_restated_hash(k):
    mask = (1 << (2 * k)) - 1
    rng = np.random.default_rng(k)
    vals = [0, 1, mask, mask - 1] + [int(x) & mask for x in rng.integers(0, 1 << 62, size=300)]
    keys = np.array([sc.unhash(v, k) for v in vals], dtype=U64)
    assert refimpl._hash(keys, mask).tolist() == vals
    assert len(set(keys.tolist())) == len(set(vals))


@pytest.mark.parametrize("k", sc.KS)
def test_planted_kmers_hash_to_their_values_in_the_products_code(k):
    """plant() against canonical_hash<u32> / <u64>: value, strand, and `false` for nothing that was planted."""
    L = hip.test_lib()
    mask = (1 << (2 * k)) - 1
    rng = np.random.default_rng(100 + k)
    want = sorted({int(x) & mask for x in rng.integers(0, 1 << 62, size=120)} | set(range(min(mask + 1, 40))))
    strands = [int(x) for x in rng.integers(0, 2, size=len(want))]
    kmers, used = sc.plant(want, k, strands)
    assert 0.25 * len(want) < len(used) < 0.75 * len(want) or k <= 2      # about half of all values are usable
    st = [s for v, s in zip(want, strands) if v in set(used)]
    for kmer, v, s in zip(kmers, used, st):
        words = np.concatenate([seqio.pack_codes(np.concatenate([np.zeros(3, np.uint8), kmer])), np.zeros(2, U64)])
        for use32 in ((0, 1) if 2 * k < 32 else (0,)):
            val, strand = C.c_uint64(0), C.c_uint32(0)
            assert L.rvn_test_canonical(words.ctypes.data_as(C.c_void_p), 3, k, use32, C.byref(val), C.byref(strand)) == 1
            assert (val.value, strand.value) == (v, s), (k, v, use32)


def test_select_specs_cover_every_byte_of_every_width():
    specs = sc.select_specs()
    assert {(k, b) for _, k, b, _, _ in specs} == {(k, b) for k in sc.KS for b in range(sc.nbytes(k))}
    assert {sc.nbytes(k) for k in sc.KS} == set(range(1, 9))
    for k in sc.KS:
        if sc.nbytes(k) > 1:   # (one byte: the digits that are a usable value)
            for b in range(sc.nbytes(k)):
                have = {d for _, kk, bb, d, _ in specs if (kk, bb) == (k, b)}
                assert {d for d in (0, 3, 4, 252, 255) if d <= sc.max_digit(k, b)} <= have
    assert {kind for *_, kind in specs} == {"exact", "carry", "plus", "minus", "top"}


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_generators_build_what_the_cases_are_named_after(family):
    """family_sets runs every generator's assertion (select_check, ties_check, keep_check and the ones inside the
    palindrome, edge, word and range builders); here: sizes, names, and that no set is empty."""
    sets = sc.family_sets(family)
    assert sets
    names = [n for cs in sets for n in cs.names]
    assert len(names) == len(set(names))
    for cs in sets:
        assert 0 < cs.n < 300 and cs.w in sc.WINDOWS
        assert max(r.shape[0] for r in cs.reads) < 25_000
    if family == "select_byte":
        assert sorted(names) == sorted(n for n, *_ in sc.select_specs())
        assert {cs.w for cs in sets} >= {1, 5, 10}
    if family == "ties":
        assert sorted(names) == sorted(n for n, *_ in sc.ties_specs())
    if family == "tile_edges":
        assert (31, 256) in {(cs.k, cs.w) for cs in sets}


def test_every_window_length_and_every_k_is_used():
    sets = sc.all_sets()
    assert {cs.w for cs in sets} == set(sc.WINDOWS)
    assert {cs.k for cs in sets} == set(sc.KS)


def test_ranges_hold_what_the_family_names():
    for cs in sc.family_sets("ranges"):
        rg = sc.ranges_of(cs)
        tiles = [sc.has_tiles(cs, i) for i in range(cs.n)]
        assert (0, cs.n) in rg and all((i, i + 1) in rg for i in range(cs.n)) and (0, 0) in rg
        assert any(f < l and not any(tiles[f:l]) and l - f == 3 for f, l in rg)           # only reads without tiles
        assert any(f < l and not tiles[f] and tiles[l - 1] for f, l in rg)                # begins on one
        assert any(f < l and tiles[f] and not tiles[l - 1] for f, l in rg)                # ends on one
        assert any(0 < f < l and not tiles[f - 1] and tiles[f] for f, l in rg)            # begins just behind one
        assert any(f < l < cs.n and not tiles[l] and tiles[l - 1] for f, l in rg)         # ends just before one
        assert not tiles[0] and not tiles[-1]
        assert {cs.reads[i].shape[0] for i in range(cs.n) if not tiles[i]} == {0, 1, cs.k - 1, cs.k + cs.w - 2}


def test_pack_codes_arrays_hold_what_the_family_names():
    arrs = sc.pack_codes_arrays()
    big = arrs["empty_first_middle_last"]
    lens = [len(a) for a in big]
    assert len(big) > 256 and lens[0] == 0 and lens[-1] == 0 and any(lens[i:i + 3] == [0, 0, 0] and lens[i - 1] and lens[i + 3]
                                                                     for i in range(1, len(lens) - 3))
    assert {0, 1, 31, 32, 33, 63, 64, 65, 1000} == {len(a) for a in arrs["lengths"]} == set(lens)
    assert arrs["empty_set"] == [] and [len(a) for a in arrs["one_empty_read"]] == [0]
    assert any((a > 3).any() for a in big)
    ref = sc.pack_codes_reference(arrs["lengths"])
    for i, a in enumerate(arrs["lengths"]):
        assert np.array_equal(ref.codes(i), a & 3)


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_oracle_equals_the_reference(family):
    for cs in sc.family_sets(family):
        eng = oracle.Engine(cs.k, cs.w)
        for mh in (False, True):
            parts = [eng.sketch(cs.rs, i, mh) for i in range(cs.n)]
            off = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in parts])])
            got = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), off)
            assert sc.compare(got, cs.reference(0, cs.n, mh), cs.names) == [], (cs.name, mh)


def test_the_reference_of_a_range_is_the_slice_of_the_whole():
    cs = sc.family_sets("ranges")[0]
    v, o, off = cs.reference(0, cs.n, True)
    for f, l in sc.ranges_of(cs):
        rv, ro, roff = cs.reference(f, l, True)
        assert np.array_equal(rv, v[off[f]:off[l]]) and np.array_equal(ro, o[off[f]:off[l]])
        assert np.array_equal(roff.astype(np.int64), off[f:l + 1].astype(np.int64) - int(off[f]))
    assert ((o >> U64(32)) == np.repeat(np.arange(cs.n, dtype=U64), np.diff(off.astype(np.int64)))).all()


def test_ids_land_in_bits_32_to_61_only():
    cs = sc.family_sets("words")[0]
    _, o, off = cs.reference()
    assert set(cs.ids[:3].tolist()) == set(sc.WORD_IDS)
    for i in range(cs.n):
        part = o[off[i]:off[i + 1]]
        assert part.shape[0] and ((part >> U64(32)) == U64(int(cs.ids[i]))).all()
        assert (((part & U64(0xFFFFFFFF)) >> U64(1)) < U64(cs.reads[i].shape[0])).all()


# ---- the comparison notices what a wrong kernel would do ----------------------------------------------------------------

def _tie_set():
    cs = next(c for c in sc.family_sets("ties") if (c.k, c.w) == (15, 33))
    i = cs.names.index("ties:k15:w33:cut:255")
    return cs, i


def test_compare_notices_seeded_faults():
    cs, i = _tie_set()
    raw = cs.reference(0, cs.n, False)
    mh = cs.reference(0, cs.n, True)
    fl = cs.reference(0, cs.n, flags=True)
    for want in (raw, mh, fl):
        assert sc.compare(want, want, cs.names) == [] and sc.compare(want[:2], want, cs.names) == []
    v, o, off = (x.copy() for x in mh)
    j = int(off[i]) + 7

    def shifted(off, at, by):
        out = off.astype(np.int64).copy()
        out[at:] += by
        return out

    faults = {
        "dropped": (np.delete(v, j), np.delete(o, j), shifted(off, i + 1, -1)),
        "added": (np.insert(v, j, v[j]), np.insert(o, j, o[j] - U64(2)), shifted(off, i + 1, 1)),
        "strand": (v, o ^ (np.arange(o.shape[0]) == j).astype(U64), off),
        "swapped": (np.concatenate([v[:j], v[j:j + 2][::-1], v[j + 2:]]), np.concatenate([o[:j], o[j:j + 2][::-1], o[j + 2:]]), off),
        "offsets": (v, o, np.concatenate([off[:1], off[:-1]])),
    }
    # the wrong one of two equal T values: the later position instead of the earlier
    rv, ro, kept = cs.raw(i)
    p = sc.select_profile(cs.reads[i], cs.k, cs.w)
    last_kept, first_dropped = int(p["tie_idx"][p["rem"] - 1]), int(p["tie_idx"][p["rem"]])
    assert kept[last_kept] and not kept[first_dropped] and rv[last_kept] == rv[first_dropped]
    wrong = kept.copy()
    wrong[last_kept], wrong[first_dropped] = False, True
    a, b = int(off[i]), int(off[i + 1])
    faults["later_tie"] = (np.concatenate([v[:a], rv[wrong], v[b:]]), np.concatenate([o[:a], ro[wrong], o[b:]]), off)
    assert np.array_equal(faults["later_tie"][0], v)                      # the values cannot tell
    for name, got in faults.items():
        errs = sc.compare(got, mh, cs.names)
        assert errs, name
        if name not in ("offsets",):
            assert any(cs.names[i] in e for e in errs) or name in ("dropped", "added"), (name, errs)
    # flags
    fv, fo, foff = fl
    fa, fb = int(foff[i]), int(foff[i + 1])
    flagged = np.nonzero(fo[fa:fb] >> U64(63))[0] + fa
    unflagged = np.nonzero((fo[fa:fb] >> U64(63)) == 0)[0] + fa
    assert flagged.size and unflagged.size
    for name, at, bit in (("missing_flag", flagged[-1], 63), ("flag_too_many", unflagged[0], 63), ("foreign_on_member", flagged[0], 62)):
        bad = fo.copy()
        bad[at] ^= U64(1 << bit)
        assert sc.compare((fv, bad), fl, cs.names), name
    assert int((fo >> U64(63)).sum()) == cs.n_kept() == mh[0].shape[0]
