"""No GPU: the plain reference of the second pass (tests/pass2_cases.py) against the oracle, piece by piece and as a whole,
and every claim of every crafted case against the reference's output.  tests/test_gpu_pass2_cases.py runs the same cases
on the device."""
import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip, seqio, synth
from tests import pass2_cases as pc

DT = pc.DT


def _crafted():
    return [c for c in pc.cases() if c["family"] != "subset"]


def _rows(case):
    return [tuple(int(v) for v in o) for b in case["batches"] for e in b["maps"] for o in np.asarray(e[1]).tolist()]


def test_every_family_has_cases_and_every_claim_holds_on_the_reference():
    assert {c["family"] for c in pc.cases()} == set(pc.FAMILIES)
    for case in pc.cases():
        pc.assert_defined(case)
    checked = 0
    for case in _crafted():
        checked += pc.check_claims(case, pc.reference(case["name"]))
    assert checked > 300
    # the kmax pair is kept and the kmax + 1 pair dropped for every identity and span length
    seen = set()
    for case in _crafted():
        for p in case["claims"].get("pairs", []):
            if p["distance"] in (p["kmax"], p["kmax"] + 1):
                seen.add((case["identity"], p["maxlen"], p["distance"] - p["kmax"]))
    for identity in pc.IDENTITIES:
        for span in pc.SPANS:
            assert (identity, span, 0) in seen and (identity, span, 1) in seen, (identity, span)
    heads = {h for c in _crafted() for h in c["claims"].get("heads", [])}
    assert {0, 255, 256, 257, 4095, 4096, 4097} <= heads


def _rules_python(ovl, begin, end, invalid):
    out, ok, ty = ovl.copy(), np.zeros(ovl.shape[0], np.uint8), np.zeros(ovl.shape[0], np.uint32)
    for i, o in enumerate(ovl.tolist()):
        u = pc.overlap_update(tuple(int(v) for v in o), begin, end, invalid)
        if u is not None:
            out[i] = u
            ok[i] = 1
            ty[i] = pc.overlap_type(u, begin, end)
    return out, ok, ty


def _random_overlaps(n, seed):
    """Overlaps around regions drawn so that every branch of OverlapUpdate and every type is taken."""
    rng = np.random.default_rng(seed)
    piles = 64
    begin = rng.integers(0, 300, piles).astype(np.uint32)
    end = (begin + rng.integers(0, 1500, piles)).astype(np.uint32)
    invalid = (rng.random(piles) < 0.05).astype(np.uint8)
    o = np.zeros(n, dtype=DT)
    o["lhs_id"], o["rhs_id"] = rng.integers(0, piles, n), rng.integers(0, piles, n)
    for side in ("lhs", "rhs"):
        b, e = begin[o[side + "_id"]].astype(np.int64), end[o[side + "_id"]].astype(np.int64)
        lo = np.maximum(b + rng.integers(-150, 150, n), 0)
        hi = np.maximum(e + rng.integers(-150, 150, n), 0)
        snap = rng.random(n)
        lo = np.where(snap < 0.1, b, np.where(snap < 0.15, e, lo))
        hi = np.where((snap > 0.8) & (snap < 0.9), e, np.where(snap > 0.95, b, hi))
        o[side + "_begin"], o[side + "_end"] = np.minimum(lo, hi), np.maximum(lo, hi)
    o["strand"] = rng.integers(0, 2, n)
    return o, begin, end, invalid


def test_the_rules_equal_the_oracle_and_the_host_side_of_overlap_rules_h():
    lists = [(pc._ovl(_rows(c)), c["begin"], c["end"], c["invalid"]) for c in _crafted() if c["family"] == "rules"]
    lists.append(_random_overlaps(20_000, 5))
    types = set()
    for ovl, begin, end, invalid in lists:
        got = _rules_python(ovl, begin.tolist(), end.tolist(), invalid.tolist())
        for other in (oracle.overlap_update_and_type(ovl, begin, end, invalid),
                      hip.test_overlap_update_and_type(ovl.astype(hip.OVERLAP_DTYPE), begin, end, invalid)):
            assert np.array_equal(got[1], other[1])
            assert np.array_equal(got[0][got[1] == 1], other[0][got[1] == 1].astype(DT))
            assert np.array_equal(got[2][got[1] == 1], other[2][got[1] == 1])
        types |= set(got[2][got[1] == 1].tolist())
    assert types == {0, 1, 2, 3, 4}


def test_add_kmers_equals_the_oracle_on_the_kmers_cases():
    marked = 0
    for case in _crafted():
        if case["family"] != "kmers":
            continue
        rs = seqio.pack_reads(case["reads"])
        for b in case["batches"]:
            for qid, _, filtered, _ in b["maps"]:
                want = oracle.pile_add_kmers(rs, qid, filtered, case["kmer_len"])
                got = pc.add_kmers(case["reads"][qid], filtered, case["kmer_len"])
                assert np.array_equal(got, want), (case["name"], qid)
                marked += int(got.sum())
        for kmer, stage, label in case["claims"]["lc"]:
            assert pc.lc_passes(kmer, case["kmer_len"]) == (stage is None), label
    assert marked > 20


def test_edit_distance_equals_the_oracle_on_the_identity_pairs():
    n = 0
    for case in _crafted():
        for p in case["claims"].get("pairs", []):
            u = pc.overlap_update(p["overlap"], case["begin"].tolist(), case["end"].tolist(), case["invalid"].tolist())
            lhs, rhs = pc.score_spans(u, case["reads"])
            assert max(len(lhs), len(rhs)) == p["maxlen"]
            assert oracle.edit_distance(lhs.tobytes(), rhs.tobytes()) == p["distance"], (case["name"], p)
            assert pc.edit_distance(lhs, rhs) == p["distance"], (case["name"], p)
            n += 1
    assert n > 150
    rng = np.random.default_rng(3)
    for _ in range(50):
        a, b = pc._random_read(rng, int(rng.integers(0, 200))), pc._random_read(rng, int(rng.integers(0, 200)))
        assert pc.edit_distance(a, b) == oracle.edit_distance(a.tobytes(), b.tobytes())


@pytest.mark.parametrize("layout", ["plain", "gaps"])
def test_identity_filter_ref_equals_the_oracle(layout):
    kept = dropped = 0
    for case in _crafted():
        if case["family"] != "identity":
            continue
        L = pc.identity_lists(case, layout)
        rs = seqio.pack_reads(L["reads"])
        want_o, want_off = oracle.identity_filter(rs, L["overlaps"], L["offsets"], L["begin"], L["end"], L["invalid"],
                                                  case["identity"])
        got_o, got_off = pc.identity_filter_ref(L["overlaps"], L["offsets"], L["reads"], L["begin"].tolist(), L["end"].tolist(),
                                                L["invalid"].tolist(), case["identity"])
        assert np.array_equal(got_off, want_off) and np.array_equal(got_o, want_o), case["name"]
        kept += got_o.shape[0]
        dropped += L["overlaps"].shape[0] - got_o.shape[0]
    assert kept > 20 and dropped > 20


def _drive(reads, begin, end, invalid, freq, identity, batch_bases, k=15):
    """Pass2Ref driven batch by batch from the oracle engine's Minimize / Filter / Map (construct.cc:361-383)."""
    ref = pc.Pass2Ref([len(r) for r in reads], begin, end, invalid)
    if ref.s:
        V = seqio.pack_reads([reads[i] for i in ref.order[:ref.s]], ids=np.array(ref.order[:ref.s], dtype=np.uint32))
        eng = oracle.Engine(k, pc.W)
        for j, last in ref.index_batches(batch_bases):
            eng.minimize(V, j, last, minhash=False)
            eng.filter(freq)
            maps = []
            for q in range(last):
                m = eng.map(V, q, True, True, False)
                maps.append((ref.order[q], m["overlaps"], m["filtered"]))
            ref.batch(maps, identity, reads, k)
    ref.finish()
    return ref


def _equal_to_oracle(ref, want):
    got = ref.state()
    assert np.array_equal(got["overlaps"], want["overlaps"])
    assert np.array_equal(got["contained"], want["contained"])
    off = got["kmers_offsets"].astype(np.int64)
    for i in range(ref.n):
        assert np.array_equal(got["kmers"][off[i]:off[i + 1]], want["kmers"][i]), i


@pytest.mark.parametrize("identity", [0.0, 0.78])
@pytest.mark.parametrize("batch_bases", [1 << 30, 150_000])
def test_pass2ref_equals_the_oracle_pass_on_a_repeat_genome(batch_bases, identity):
    """60 kb with a repeat at 14x, reads of 2.5 kb; at identity 0.78 the Python DP scores every overlap Map reports."""
    rng = np.random.default_rng(3)
    g = synth.make_genome(60_000, seed=3)
    rep = g[1000:2500].copy()
    for c in range(1, 6):
        g[1000 + c * 10_000:2500 + c * 10_000] = synth.mutate(rng, rep, 0.01, 0.0, 0.0)[:1500]
    rs, _ = synth.make_reads(g, 14, 2500, seed=4)
    reads = [rs.codes(i) for i in range(rs.n)]
    begin = np.full(rs.n, 48, np.uint32)
    end = (((rs.lengths >> 4) << 4) - 48).astype(np.uint32)
    invalid = (np.random.default_rng(8).random(rs.n) < 0.15).astype(np.uint8)
    ref = _drive(reads, begin, end, invalid, 0.01, identity, batch_bases)
    assert len(ref.index_batches(batch_bases)) == (1 if batch_bases == 1 << 30 else 5)
    want = oracle.second_pass(15, 5, rs, begin, end, invalid, freq=0.01, identity=identity, batch_bases=batch_bases)
    _equal_to_oracle(ref, want)
    assert want["overlaps"].shape[0] > 50 and want["contained"].sum() > 0 and sum(int(k.sum()) for k in want["kmers"]) > 0


@pytest.mark.parametrize("identity", [0.0, 0.78])
@pytest.mark.parametrize("name", pc.names("subset"))
def test_pass2ref_equals_the_oracle_pass_on_the_subset_read_sets(name, identity):
    case = pc.by_name(name)
    rs = seqio.pack_reads(case["reads"])
    ref = _drive(case["reads"], case["begin"], case["end"], case["invalid"], case["freq"], identity, case["batch_bases"])
    want = oracle.second_pass(15, 5, rs, case["begin"], case["end"], case["invalid"], freq=case["freq"], identity=identity,
                              batch_bases=case["batch_bases"])
    _equal_to_oracle(ref, want)
    if identity == 0.0:  # (the claims are stated for the unfiltered pass, as in tests/test_gpu_pass2_cases.py)
        pc.check_claims(case, ref.state())
    batches = ref.index_batches(case["batch_bases"])
    if name.endswith("one_read_batches"):
        # (a read of no bases does not close a batch: it shares the next read's)
        assert all(b - a <= 2 for a, b in batches) and sum(b - a == 1 for a, b in batches) > 50
    if "last_batch" in case["claims"]:
        assert len(batches) == 2 and batches[-1][1] - batches[-1][0] == 1


def test_pass2ref_with_the_identity_filter_equals_the_oracle_pass():
    """Identity 0.78 on the first reads of the subset set (the Python DP decides every overlap), in one and in several batches."""
    reads = pc._subset_reads()[:40]
    n = len(reads)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    begin, end = np.zeros(n, np.uint32), ((lens >> 4) << 4).astype(np.uint32)
    invalid = (np.arange(n) % 7 == 3).astype(np.uint8)
    rs = seqio.pack_reads(reads)
    n_kept = []
    for identity in (0.0, 0.78):
        for batch_bases in (1 << 30, 20_000):
            ref = _drive(reads, begin, end, invalid, 0.01, identity, batch_bases)
            want = oracle.second_pass(15, 5, rs, begin, end, invalid, freq=0.01, identity=identity, batch_bases=batch_bases)
            _equal_to_oracle(ref, want)
            n_kept.append(want["overlaps"].shape[0])
    assert n_kept[0] > 0
