"""The second mapping pass on the device (raven_amd/csrc/pass2.hip) on the crafted cases of tests/pass2_cases.py: every
rules, dedup, finish, identity and kmers case through rvn_test_second_pass (second_pass_prepare, the part of
second_pass_batch behind Map once per batch, second_pass_finish — Map's output comes from the case), the identity cases also
through Engine.filter_overlaps_by_identity, the subset read sets through Engine.find_overlaps_and_repetitive_regions.
Overlaps (all eight fields, the order), containment flags, k-mer cells and offsets must equal the plain reference
(Pass2Ref, identity_filter_ref; held to the oracle by tests/test_pass2_cases.py) or the oracle's pass.  Integers, no
tolerance."""
import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip, seqio
from tests import pass2_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = hip.Engine(15, pc.W)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hook_engines():
    """One engine of the test library per k (a handle belongs to the library that made it)."""
    made = {}

    def get(k):
        if k not in made:
            made[k] = hip.HookEngine(k)
        return made[k]

    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("name", pc.names("rules", "dedup", "finish", "identity", "kmers"))
def test_crafted_batches_equal_the_reference(hook_engines, name):
    case, want = pc.by_name(name), pc.reference(name)
    he = hook_engines(case["k"])
    rs = seqio.pack_reads(case["reads"])
    rd = he.upload(rs)
    try:
        got = he.second_pass(rd, rs.n, case["begin"], case["end"], case["invalid"], case["identity"], case["kmer_len"],
                             [pc.device_batch(case, b) for b in case["batches"]])
    finally:
        he.reads_destroy(rd)
    d = pc.diff_state(got, want)
    assert d is None, "%s: %s" % (name, d)
    pc.check_claims(case, got)


@pytest.mark.parametrize("layout", ["plain", "gaps"])
@pytest.mark.parametrize("name", pc.names("identity"))
def test_identity_filter_of_lists_equals_the_reference(eng, name, layout):
    case = pc.by_name(name)
    L = pc.identity_lists(case, layout)
    rd = eng.upload(seqio.pack_reads(L["reads"]))
    try:
        got_o, got_off = eng.filter_overlaps_by_identity(rd, L["overlaps"].astype(hip.OVERLAP_DTYPE), L["offsets"], L["begin"],
                                                         L["end"], L["invalid"], case["identity"])
    finally:
        rd.close()
    want_o, want_off = pc.identity_filter_ref(L["overlaps"], L["offsets"], L["reads"], L["begin"].tolist(), L["end"].tolist(),
                                              L["invalid"].tolist(), case["identity"])
    assert np.array_equal(got_off, want_off), "%s: offsets %s, expected %s" % (name, got_off.tolist(), want_off.tolist())
    bad = np.flatnonzero(got_o != want_o.astype(hip.OVERLAP_DTYPE))
    assert bad.size == 0, "%s: entry %d is %s, expected %s" % (name, bad[0], got_o[bad[0]].tolist(), want_o[bad[0]].tolist())
    kept = {(int(o["lhs_id"]), int(o["rhs_id"])) for o in want_o}
    assert 0 < len(kept) < L["overlaps"].shape[0]


@pytest.fixture(scope="module")
def subset_reads(eng):
    rs = seqio.pack_reads(pc._subset_reads())
    rd = eng.upload(rs)
    yield rs, rd
    rd.close()


@pytest.mark.parametrize("identity", [0.0, 0.78])
@pytest.mark.parametrize("name", pc.names("subset"))
def test_subset_read_sets_equal_the_oracle_pass(eng, subset_reads, name, identity):
    case = pc.by_name(name)
    rs, rd = subset_reads
    got = eng.find_overlaps_and_repetitive_regions(rd, case["begin"], case["end"], case["invalid"], freq=case["freq"],
                                                   identity=identity, batch_bases=case["batch_bases"])
    want = oracle.second_pass(15, pc.W, rs, case["begin"], case["end"], case["invalid"], freq=case["freq"], identity=identity,
                              batch_bases=case["batch_bases"])
    koff = np.zeros(rs.n + 1, dtype=np.uint64)
    np.cumsum([len(k) for k in want["kmers"]], out=koff[1:])
    flat = lambda ks: np.concatenate([np.asarray(k, dtype=np.uint8) for k in ks]) if len(ks) else np.zeros(0, np.uint8)
    goff = np.zeros(rs.n + 1, dtype=np.uint64)
    np.cumsum([len(k) for k in got["kmers"]], out=goff[1:])
    d = pc.diff_state(dict(overlaps=got["overlaps"], contained=got["contained"], kmers=flat(got["kmers"]), kmers_offsets=goff),
                      dict(overlaps=want["overlaps"], contained=want["contained"], kmers=flat(want["kmers"]), kmers_offsets=koff))
    assert d is None, "%s at identity %g: %s" % (name, identity, d)
    if identity == 0.0:
        pc.check_claims(case, dict(overlaps=got["overlaps"], contained=got["contained"], kmers=flat(got["kmers"]),
                                   kmers_offsets=goff))


def test_the_hook_refuses_what_a_kernel_would_index_with(hook_engines):
    case = pc.by_name("kmers:k15")
    he = hook_engines(15)
    rs = seqio.pack_reads(case["reads"])
    rd = he.upload(rs)
    try:
        qf, ql, org, off, flt, ovl = pc.device_batch(case, case["batches"][0])
        args = lambda b: (rd, rs.n, case["begin"], case["end"], case["invalid"], 0.0, 15, [b])
        bad_off = off.copy()
        bad_off[1], bad_off[2] = bad_off[2] + 1, bad_off[1]
        bad_org = org.copy()
        bad_org[0] = (int(bad_org[0]) >> 32 << 32) | (len(case["reads"][1]) << 1)
        bad_ovl = np.array([(0, 0, 100, rs.n, 0, 100, 0, 1)], dtype=hip.OVERLAP_DTYPE)
        far_off = off.copy()  # an offset beyond n_query: refused before it indexes anything
        far_off[1] = 10 ** 6
        # (the last one: an overlap in a batch without a query read it could come from)
        for bad in ((qf, ql, org, bad_off, flt, ovl), (qf, ql, org, far_off, flt, ovl), (qf, ql, bad_org, off, flt, ovl),
                    (qf, ql, org, off, flt, bad_ovl), (qf, ql + 1, org, np.append(off, off[-1]), flt, ovl),
                    (2, 2, org[:0], np.zeros(1, np.uint32), flt[:0], np.array([(0, 0, 100, 1, 0, 100, 0, 1)], hip.OVERLAP_DTYPE))):
            with pytest.raises(ValueError):
                he.second_pass(*args(bad))
        with pytest.raises(ValueError):
            he.second_pass(rd, rs.n, case["begin"], case["end"] + 4096, case["invalid"], 0.0, 15, [])
    finally:
        he.reads_destroy(rd)
