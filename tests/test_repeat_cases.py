"""The crafted cases of ResolveRepeatInducedOverlaps (tests/repeat_cases.py) on the CPU: on every case RepeatRef (plain
Python from the reference), the restatement program (tests/host/repeats_reference.cpp, the oracle's FindSlopes) and the
host build of the device's own repeats.h / overlap_rules.h (tests/host/repeats_pile.cpp) agree field for field; the
hand-derived marks the cases carry as claims hold; and every case is what its tags say, read from RepeatRef's trace
(first-sweep runs, slope pairs, raw counts, medians and removals per iteration)."""
import numpy as np
import pytest

from tests import repeat_cases as rc
from tests import repeats_util as ru


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("repeat_programs")
    return ru.build_reference(d), ru.build_pile_program(d)


def test_repeat_ref_uses_the_device_record_layout():
    assert rc.OVERLAP_DTYPE == ru.hip.OVERLAP_DTYPE


@pytest.mark.parametrize("name", rc.names())
def test_three_statements_agree(name, programs, tmp_path):
    want, _ = rc.reference(name)
    inp = rc.stage_input(rc.by_name(name))
    for exe, tag in zip(programs, ("restatement", "repeats_h")):
        got, _ = ru.run_program(exe, inp, tmp_path, tag)
        ru.assert_same(got, want)


def test_all_piles_of_family_a_in_one_call_are_the_single_piles_side_by_side(programs, tmp_path):
    union, parts = rc.family_a_union()
    want, _ = rc.reference("A:union")
    got, _ = ru.run_program(programs[1], rc.stage_input(union), tmp_path, "union")
    ru.assert_same(got, want)
    names = [c["name"] for c in parts]
    assert names[:3] == ["A:len:4096", "A:len:0", "A:len:4097"]
    regions = np.concatenate([rc.reference(n)[0]["regions"] for n in names])
    assert np.array_equal(want["regions"], regions)
    assert np.array_equal(want["is_repetitive"], np.concatenate([rc.reference(n)[0]["is_repetitive"] for n in names]))


# ---- claims ------------------------------------------------------------------------------------------------------------

def _regions(out, p):
    roff = out["region_offsets"]
    return [tuple(r) for r in out["regions"][int(roff[p]):int(roff[p + 1])].tolist()]


def _matches(rec, want):
    return all(rec[k] == v for k, v in want.items())


@pytest.mark.parametrize("name", rc.names())
def test_claims_hold(name):
    case = rc.by_name(name)
    out, ref = rc.reference(name)
    cl = case["claims"]
    for p, want in cl.get("regions", {}).items():
        assert _regions(out, p) == [tuple(w) for w in want], p
    for p, want in cl.get("is_repetitive", {}).items():
        assert out["is_repetitive"][p] == want, p
    for k in ("iterations", "components", "removed"):
        if k in cl:
            assert out[k] == cl[k], k
    if "removed_per_iteration" in cl:
        assert ref.removed_per_iteration == cl["removed_per_iteration"]
    if "survivors" in cl:
        assert np.array_equal(out["overlaps"], case["overlaps"][cl["survivors"]])
        assert list(cl["survivors"]) == sorted(cl["survivors"])
    for p, want in cl.get("runs", {}).items():
        assert set(want) <= set(ref.trace[p].first_sweep), (want, ref.trace[p].first_sweep)
    for p, want in cl.get("raw", {}).items():
        assert len(ref.trace[p].raw) == want, (p, len(ref.trace[p].raw))
    for p, want in cl.get("slopes", {}).items():
        assert len(ref.trace[p].slopes) == want
    for p, want in cl.get("median_used", {}).items():
        assert ref.medians_used[0][p] == want, p
    for p, want in cl.get("median_per_iteration", {}).items():
        assert [used[p] for used in ref.medians_used] == want
    for p, want in cl.get("pair", {}).items():
        assert any(_matches(rec, want) for rec in ref.trace[p].pairs), ref.trace[p].pairs
    if "types" in cl:
        assert [rc.overlap_type(tuple(int(x) for x in o), case["begin"].tolist(), case["end"].tolist())
                for o in case["overlaps"].tolist()] == cl["types"]


# ---- tags: every case is what its tags say ---------------------------------------------------------------------------------

def _twin(case):
    """the case one step across the boundary: same tags, and the inputs differ in one median or one coverage cell"""
    other = rc.by_name(case["claims"]["flips_with"])
    assert other["claims"]["flips_with"] == case["name"] and other["tags"] == case["tags"]
    a, b = rc.stage_input(case), rc.stage_input(other)
    dm = int((a.median != b.median).sum())
    dc = int((a.coverage != b.coverage).sum()) if a.coverage.shape == b.coverage.shape else -1
    assert (dm, dc) in ((1, 0), (0, 1)), (dm, dc)
    ra, rb = _regions(rc.reference(case["name"])[0], 0), _regions(rc.reference(other["name"])[0], 0)
    assert (len(ra), len(rb)) in ((0, 1), (1, 0))  # they differ in exactly the one region
    return other, dm


def _pairs(ref, p=0):
    return ref.trace[p].pairs


def _span(rec):
    return ((rec["down"][0] >> 1) + rec["down"][1]) // 2 - ((rec["up"][0] >> 1) + rec["up"][1]) // 2


def _cells(case, p=0):
    return len(case["coverage"][p])


def _merge_once(src):
    """MergeRegions without its rescan"""
    dst, merged = [], [False] * len(src)
    for i in range(len(src)):
        if merged[i]:
            continue
        f, s = src[i]
        for j in range(i + 1, len(src)):
            if not merged[j] and f < src[j][1] and s > src[j][0]:
                merged[j] = True
                f, s = min(f, src[j][0]), max(s, src[j][1])
        dst.append([f, s])
    return dst


def _on_pile0(case):
    """(index, begin cell, end cell) of every overlap as pile 0 sees it (the lhs coordinates when it is the lhs)"""
    out = []
    for i, o in enumerate(case["overlaps"].tolist()):
        if o[0] == 0:
            out.append((i, o[1] >> 4, o[2] >> 4))
        elif o[3] == 0:
            out.append((i, o[4] >> 4, o[5] >> 4))
    return out


def _pile0_geometry(case, out):
    b_, e_ = int(case["begin"][0]) >> 4, int(case["end"][0]) >> 4
    return b_, e_, int(0.1 * (e_ - b_)), _regions(out, 0)


def t_plateau(case, out, ref):
    assert len(_pairs(ref)) == 1 and _pairs(ref)[0]["accepted"] and len(ref.trace[0].raw) == 1


def t_median_flip(case, out, ref):
    _, dm = _twin(case)
    assert dm == 1 and all(r["found_peak"] for r in _pairs(ref))


def t_validity(case, out, ref):
    _, dm = _twin(case)
    rec = _pairs(ref)[0]
    assert dm == 0 and rec["span_ok"] and rec["found_peak"]
    assert abs(rec["num_valid"] - 0.9 * (rec["interior"] + 1)) < 1  # one dip from the boundary


def t_span(case, out, ref):
    assert len(_pairs(ref)) == 1
    rec, limit = _pairs(ref)[0], 0.84 * _cells(case)
    assert rec["span_ok"] == (_span(rec) <= limit) and rec["accepted"] == rec["span_ok"]
    if "flips_with" in case["claims"]:
        _twin(case)
        assert abs(_span(rec) - limit) < 1


def t_found_peak(case, out, ref):
    assert any(r["span_ok"] and r["interior"] > 0 and not r["found_peak"] and
               r["num_valid"] >= 0.9 * (r["interior"] + 1) for r in _pairs(ref))


def t_clamp(case, out, ref):
    assert int(case["coverage"][0].max()) == 65535 or int(case["median"][0]) in (0, 65535)


def t_spike(case, out, ref):
    assert min(r["interior"] for r in _pairs(ref) if r["span_ok"]) == 1


def t_non_adjacent(case, out, ref):
    slopes = ref.trace[0].slopes
    ups = [s for s in slopes if s[0] & 1]
    downs = [s for s in slopes if not s[0] & 1]
    rec = next(r for r in _pairs(ref) if r["up"] == ups[0] and r["down"] == downs[-1])
    assert slopes.index(downs[-1]) - slopes.index(ups[0]) > 1 and rec["span_ok"]
    assert rec["accepted"] == case["claims"]["non_adjacent"][0]
    assert sum(r["accepted"] for r in _pairs(ref)) >= 2


def t_first_try_full(case, out, ref):
    assert len(ref.trace[0].raw) == rc.FIRST_TRY


def t_retry(case, out, ref):
    raws = [len(ref.trace[p].raw) for p in range(len(case["coverage"]))]
    assert max(raws) > rc.FIRST_TRY
    if len(raws) > 1:  # several retry piles with different room, a pile that fits between them
        assert len({r for r in raws if r > rc.FIRST_TRY}) >= 2 and min(raws) <= rc.FIRST_TRY


def t_kmer_push(case, out, ref):
    bare = rc.new_regions(case["coverage"][0].tolist(), [], 0, _cells(case), int(case["median"][0]))
    assert len(bare.raw) == rc.FIRST_TRY and len(ref.trace[0].raw) == rc.FIRST_TRY + 1


def t_kmer_group(case, out, ref):
    assert int(case["kmers"][0].sum()) in (rc.GROUP, rc.GROUP + 1)
    assert (len(ref.trace[0].kmer_groups) == 1) == (int(case["kmers"][0].sum()) > rc.GROUP)


def t_kmer_gap(case, out, ref):
    gaps = set(np.diff(np.flatnonzero(case["kmers"][0])).tolist())
    assert gaps in ({rc.W_KMER}, {rc.W_KMER + 1}) and (len(ref.trace[0].kmer_groups) == 1) == (gaps == {rc.W_KMER})


def t_kmers_empty(case, out, ref):
    assert any(len(k) == 0 and _regions(out, p) for p, k in enumerate(case["kmers"]))


def t_kmer_edge(case, out, ref):
    k = case["kmers"][0]
    assert len(k) == _cells(case) + 1 and k[0] and k[-1]
    assert ref.trace[0].kmer_groups[0][0] == 0 and ref.trace[0].kmer_groups[-1][1] == _cells(case)


def t_touch(case, out, ref):
    (a, b), final = ref.trace[0].raw, _regions(out, 0)
    touching = a[1] == b[0] or b[1] == a[0]
    by_one = a[1] == b[0] + 1 or b[1] == a[0] + 1
    assert touching != by_one and len(final) == (2 if touching else 1)


def t_rescan(case, out, ref):
    raw = [list(r) for r in ref.trace[0].raw]
    assert len(rc.merge_regions(raw)) == 1 and len(_merge_once(raw)) == 2


def t_kmer_plateau(case, out, ref):
    assert ref.trace[0].kmer_groups and any(r["accepted"] for r in _pairs(ref)) and len(_regions(out, 0)) == 1


def t_clip(case, out, ref):
    b_, e_ = int(case["begin"][0]) >> 4, int(case["end"][0]) >> 4
    (f, s), raw = _regions(out, 0)[0], ref.trace[0].raw[0]
    assert (f >> 1 == b_ and raw[0] < b_) or (s == e_ and raw[1] > e_)


def t_outside(case, out, ref):
    f, s = _regions(out, 0)[0]
    assert (f >> 1) > s  # the inverted pair is kept


def t_length(case, out, ref):
    assert _cells(case) in rc.LENGTHS and case["name"] == "A:len:%d" % _cells(case)


def t_lds_split(case, out, ref):
    assert abs(_cells(case) - rc.LDS_CELLS) <= 1 and _regions(out, 0)


def t_chunk_boundary(case, out, ref):
    (first, last), = case["claims"]["runs"][0]
    first >>= 1
    what = case["name"].rsplit(":", 1)[1]
    assert {"lane0": first % rc.CHUNK == 0, "lane63": last % rc.CHUNK == rc.CHUNK - 1,
            "cross": last // rc.CHUNK - first // rc.CHUNK == 1, "cross2": last // rc.CHUNK - first // rc.CHUNK == 2}[what]


def t_one_cell_gap(case, out, ref):
    a, b = case["claims"]["runs"][0]
    assert (a[0] & 1) == (b[0] & 1) and (b[0] >> 1) - a[1] == 2 and a[1] + 1 in (63, 64, 65)


def t_scan_boundary(case, out, ref):
    rec = _pairs(ref)[0]
    lo_, hi_ = rec["up"][1] + 1, rec["down"][0] >> 1
    assert rec["span_ok"] and (lo_ % rc.CHUNK == 0 or hi_ % rc.CHUNK == 0)
    assert {"begin64": lo_ % 64 == 0 and hi_ % 64, "end64": hi_ % 64 == 0 and lo_ % 64}.get(
        case["name"].split(":")[2], lo_ % 64 == 0 and hi_ % 64 == 0)


def t_pile_end(case, out, ref):
    runs = ref.trace[0].first_sweep
    assert any(not r[0] & 1 and (r[0] >> 1) < rc.W_SLOPE for r in runs)
    assert any(r[0] & 1 and r[1] >= _cells(case) - rc.W_SLOPE for r in runs)


def _first_components(ref):
    return ref.components_per_iteration[0]


def t_component_size(case, out, ref):
    size = int(case["name"].rsplit(":", 1)[1])
    assert all(len(c) == size for c in _first_components(ref) if 0 in c or 1 in c)


def t_ties(case, out, ref):
    for comp in _first_components(ref):
        m = sorted(int(case["median"][j]) for j in comp)
        k = len(m) // 2
        assert m[k] in (m[k - 1], m[(k + 1) % len(m)]) and m[0] != m[-1]


def t_extremes(case, out, ref):
    assert any({0, 65535} <= {int(case["median"][j]) for j in c} for c in _first_components(ref))


def t_invalid_member(case, out, ref):
    members = {j for c in _first_components(ref) for j in c}
    inv = np.flatnonzero(case["invalid"]).tolist()
    assert any(j in members and _regions(out, j) for j in inv) and any(j not in members for j in inv)
    assert all(j in members for j in range(len(case["invalid"])) if not case["invalid"][j])


def t_no_join(case, out, ref):
    assert case["claims"]["types"] == [0, 1, 2] and out["components"] == len(case["coverage"])


def t_self_overlap(case, out, ref):
    assert all(o[0] == o[3] for o in case["overlaps"].tolist()) and min(case["claims"]["types"]) > 2


def t_sort_bits(case, out, ref):
    n = len(case["coverage"])
    members = {j for c in _first_components(ref) for j in c}
    assert n in (255, 256, 257) and 0 < len(members) < n and 0 in members


def t_union_find(case, out, ref):
    n = len(case["coverage"])
    assert n >= 40 and [len(c) for c in _first_components(ref)] == [n] and len(case["overlaps"]) >= n - 1


def t_intersection(case, out, ref):
    _, _, _, (region,) = _pile0_geometry(case, out)
    seen = _on_pile0(case)
    assert any(b == region[1] for _, b, e in seen) and any(b == region[1] - 1 for _, b, e in seen)
    assert any(e == region[0] >> 1 for _, b, e in seen) and any(e == (region[0] >> 1) + 1 for _, b, e in seen)


def t_left_branch(case, out, ref):
    b_, e_, offset, (region,) = _pile0_geometry(case, out)
    assert 0.1 * (e_ - b_) != offset and (region[0] >> 1) - (b_ + offset) in (-1, 0)


def t_balance(case, out, ref):
    b_, e_, _, _ = _pile0_geometry(case, out)
    assert any((b - b_) - (e_ - e) in (-1, 0) for _, b, e in _on_pile0(case))


def t_fuzz(case, out, ref):
    _, _, _, regions = _pile0_geometry(case, out)
    seen = _on_pile0(case)
    assert any(e - r[1] in (rc.FUZZ - 1, rc.FUZZ) or (r[0] >> 1) - b in (rc.FUZZ - 1, rc.FUZZ)
               for _, b, e in seen for r in regions)


def t_right_branch(case, out, ref):
    b_, e_, offset, (region,) = _pile0_geometry(case, out)
    assert region[1] > e_ - offset and not (region[0] >> 1) < b_ + offset


def t_both_ends(case, out, ref):
    b_, e_, offset, (region,) = _pile0_geometry(case, out)
    assert (region[0] >> 1) < b_ + offset and region[1] > e_ - offset


def t_rhs_role(case, out, ref):
    assert any(o[3] == 0 and o[0] != 0 for o in case["overlaps"].tolist())


def t_self_coordinates(case, out, ref):
    assert any(o[0] == o[3] == 0 and (o[1], o[2]) != (o[4], o[5]) for o in case["overlaps"].tolist())


def t_two_regions(case, out, ref):
    assert sorted(r[0] & 1 for r in _regions(out, 0)) == [0, 1]


def t_roles(case, out, ref):
    ovl, kept = case["overlaps"].tolist(), case["claims"]["survivors"]
    assert all(ovl[i][3] == 0 for i in kept) and all(ovl[i][0] == 0 for i in range(len(ovl)) if i not in kept)


def t_order(case, out, ref):
    kept = case["claims"]["survivors"]
    assert min(set(range(len(case["overlaps"]))) - set(kept)) < min(kept)  # the condemned one stands first


def t_wrap(case, out, ref):
    # begins before begin_ (or, the control, exactly at a begin_ > 0), or ends after end_
    b, e = int(case["begin"][0]), int(case["end"][0])
    gone = case["claims"]["removed"]
    assert any((o[1] < b and not gone) or (o[1] == b > 0 and gone) or o[2] > e
               for o in case["overlaps"].tolist() if o[0] == 0)


def t_replicated(case, out, ref):
    m = len(case["overlaps"])
    assert m >= (70000 if case["name"] == "C:replicated" else 70000 // 16) and 0 < len(out["overlaps"]) < m


def t_split(case, out, ref):
    comps = ref.components_per_iteration
    meds = case["claims"]["median_per_iteration"][0]
    assert len(comps[1]) > len(comps[0]) and meds[0] != meds[1]
    assert bool(case["claims"]["regions"][0]) == (meds[1] <= 50)


def t_orphan(case, out, ref):
    p = int(np.flatnonzero(case["invalid"])[0])
    comps = ref.components_per_iteration
    assert any(p in c for c in comps[0]) and not any(p in c for c in comps[-1])
    assert out["is_repetitive"][p] == 1 and not _regions(out, p)


def t_cascade(case, out, ref):
    assert sum(1 for r in ref.removed_per_iteration if r) >= 3
    meds = case["claims"]["median_per_iteration"][0]
    assert meds[0] > meds[1] > meds[2]


def t_all_removed(case, out, ref):
    assert len(case["overlaps"]) > 0 and len(out["overlaps"]) == 0 and ref.removed_per_iteration[0] == len(case["overlaps"])


def t_empty(case, out, ref):
    assert len(case["overlaps"]) == 0 and (len(case["coverage"]) == 0) == case["name"].endswith("n0")


TAG_CHECKS = {
    "plateau": t_plateau, "median flip": t_median_flip, "validity rule": t_validity, "span rule": t_span,
    "found_peak": t_found_peak, "clamp": t_clamp, "spike": t_spike, "non-adjacent pair": t_non_adjacent,
    "first try full": t_first_try_full, "retry": t_retry, "kmer push": t_kmer_push, "kmer group": t_kmer_group,
    "kmer gap": t_kmer_gap, "kmers empty": t_kmers_empty, "kmer edge": t_kmer_edge, "touch": t_touch,
    "rescan": t_rescan, "kmer+plateau": t_kmer_plateau, "clip": t_clip, "outside": t_outside, "length": t_length,
    "lds split": t_lds_split, "chunk boundary": t_chunk_boundary, "one-cell gap": t_one_cell_gap,
    "scan boundary": t_scan_boundary, "pile end": t_pile_end,
    "component size": t_component_size, "ties": t_ties, "extreme medians": t_extremes,
    "invalid member": t_invalid_member, "no join": t_no_join, "self overlap": t_self_overlap, "sort bits": t_sort_bits,
    "union-find": t_union_find,
    "intersection": t_intersection, "left branch": t_left_branch, "balance": t_balance, "fuzz": t_fuzz,
    "right branch": t_right_branch, "both ends": t_both_ends, "rhs role": t_rhs_role,
    "self coordinates": t_self_coordinates, "two regions": t_two_regions, "roles": t_roles, "order": t_order,
    "wrap": t_wrap, "replicated": t_replicated,
    "split": t_split, "orphan": t_orphan, "cascade": t_cascade, "all removed": t_all_removed, "empty": t_empty,
}


@pytest.mark.parametrize("name", rc.names())
def test_case_is_what_its_tags_say(name):
    case = rc.by_name(name)
    out, ref = rc.reference(name)
    assert case["tags"] and case["family"] in rc.FAMILIES
    for tag in case["tags"]:
        TAG_CHECKS[tag](case, out, ref)


# what each family has to hold at the least: tag -> number of cases
REQUIRED = {
    "plateau": 1, "median flip": 2, "validity rule": 2, "span rule": 3, "found_peak": 1, "clamp": 5, "spike": 1,
    "non-adjacent pair": 3, "first try full": 1, "retry": 4, "kmer push": 1, "kmer group": 2, "kmer gap": 2,
    "kmers empty": 2, "kmer edge": 1, "touch": 4, "rescan": 1, "kmer+plateau": 2, "clip": 2, "outside": 2,
    "length": len(rc.LENGTHS), "lds split": 3, "chunk boundary": 8, "one-cell gap": 6, "scan boundary": 4, "pile end": 1,
    "component size": 5, "ties": 1, "extreme medians": 1, "invalid member": 1, "no join": 1, "self overlap": 1,
    "sort bits": 3, "union-find": 6,
    "intersection": 1, "left branch": 2, "balance": 2, "fuzz": 5, "right branch": 2, "both ends": 2, "rhs role": 2,
    "self coordinates": 2, "two regions": 1, "roles": 1, "order": 1, "wrap": 3, "replicated": 2,
    "split": 2, "orphan": 1, "cascade": 1, "all removed": 1, "empty": 2,
}


def test_every_tag_is_used_and_every_family_has_its_classes():
    assert set(TAG_CHECKS) == set(rc.TAGS) == set(REQUIRED)
    used = {}
    for c in rc.cases():
        assert c["name"].startswith(c["family"] + ":")
        for t in c["tags"]:
            used[t] = used.get(t, 0) + 1
    for tag, least in REQUIRED.items():
        assert used.get(tag, 0) >= least, (tag, used.get(tag, 0))
    assert {rc.by_name("A:len:%d" % n)["name"] for n in rc.LENGTHS}
    assert np.array_equal(rc.by_name("A:len:4096")["coverage"][0], rc.by_name("A:len:4097")["coverage"][0][:4096])


def test_the_small_replica_is_the_large_one_cut_short():
    big, small = rc.by_name("C:replicated"), rc.by_name("C:replicated:small")
    m = len(small["overlaps"])
    assert np.array_equal(big["overlaps"][:m], small["overlaps"]) and m * 16 >= len(big["overlaps"])
    kept_big, kept_small = rc.reference("C:replicated")[0]["overlaps"], rc.reference("C:replicated:small")[0]["overlaps"]
    assert np.array_equal(kept_big[:len(kept_small)], kept_small)
