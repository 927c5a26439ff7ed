"""raven::ResolveContainedReads and raven::ResolveChimericSequences on the device (raven_amd/csrc/resolve.hip) against the
single-threaded restatement (tests/host/resolve_reference.cpp): the resident form on a first pass (rvn_pass1_resolve),
the host-array form (rvn_resolve_contained_and_chimeric), the phases one by one, generated piles that take every branch
of ClearChimericRegions, hand-built cases, the hand-off to the second pass, and the C++ facade.  Every comparison is
for equality."""
import subprocess

import numpy as np
import pytest

from oracle import oracle
from raven_amd import hip
from tests import resolve_util as U
from tests.test_gpu_facade import _build, _write_reads
from tests.test_gpu_stages import _chimeric_reads, _hash

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("resolve_ref")
    return U.build_reference(d), d


@pytest.fixture(scope="module")
def eng():
    return hip.Engine(15, 5)


def _first_pass(eng, rs):
    reads = eng.upload(rs)
    return reads, eng.find_overlaps_and_create_piles(reads, freq=0.001, kmax=32, use_minhash=False)


def _input_of_pass(p, rs):
    """The arguments of the host-array form from the entry points that exist beside it: TrimAndAnnotatePiles on the
    pass, then its lists, coverage and chimeric regions fetched."""
    b, e, med, inv = p.trim_and_annotate(4)
    regions = p.find_chimeric_regions(inv)
    cov, coff = p.piles()
    ovl, off = p.overlaps()
    return U.StageInput.from_csr(ovl, off, cov, coff, regions, b, e, med, inv.astype(np.uint8), reads=rs)


def _reads_for(identity):
    # with the identity filter the restatement aligns every overlap with a quadratic DP: shorter reads there
    return _chimeric_reads(301, 5000 if identity == 0 else 3000)


@pytest.mark.parametrize("identity", [0.0, 0.78])
def test_resident_form_matches_the_restatement(eng, ref, identity):
    exe, d = ref
    rs = _reads_for(identity)
    reads, p = _first_pass(eng, rs)
    inp = _input_of_pass(p, rs)
    want1 = U.run_program(exe, inp, d, "res1", phases=1, identity=identity)
    want3 = U.run_program(exe, inp, d, "res3", phases=3, identity=identity)
    assert want3["invalid"].sum() > 5 and (1 - want3["invalid"]).sum() > 10 and want3["contained"].sum() > 3
    assert want1["overlaps"].shape[0] > 100
    got1 = p.resolve(reads, identity=identity, phases=1)
    U.assert_same(got1, want1, coverage=False)  # the lists and offsets after ResolveContainedReads
    got3 = p.resolve(None, phases=2)
    # (the stats of a pass accumulate over its phases, as one call's do)
    U.assert_same(got3, want3, coverage=False)
    cov, coff = p.piles()
    assert np.array_equal(coff, inp.coverage_offsets) and np.array_equal(cov, want3["coverage"])
    # one call for both phases on a fresh pass that has not been trimmed
    reads2, p2 = _first_pass(eng, rs)
    got = p2.resolve(reads2, identity=identity, phases=3)
    U.assert_same(got, want3, coverage=False)
    assert np.array_equal(p2.piles()[0], want3["coverage"])
    # a phase runs once per pass
    with pytest.raises(ValueError):
        p2.resolve(None, phases=2)
    p.close()
    p2.close()


def test_resident_and_host_array_forms_agree(eng, ref):
    rs = _reads_for(0.0)
    reads, p = _first_pass(eng, rs)
    inp = _input_of_pass(p, rs)
    for phases in (1, 2, 3):
        reads_k, pk = _first_pass(eng, rs)
        a = pk.resolve(reads_k, phases=phases)
        b = inp.device(eng, phases=phases)
        U.assert_same(a, b, coverage=False)
        assert np.array_equal(pk.piles()[0], b["coverage"])
        pk.close()
    # with the identity filter, on the shorter reads
    rs = _reads_for(0.78)
    reads, p = _first_pass(eng, rs)
    inp = _input_of_pass(p, rs)
    a = p.resolve(reads, identity=0.78, phases=3)
    b = inp.device(eng, phases=3, identity=0.78, reads=reads)
    U.assert_same(a, b, coverage=False)
    assert np.array_equal(p.piles()[0], b["coverage"]) and a["stats"]["dropped_by_filter"] > 0
    p.close()


def test_generated_piles_with_lists_take_every_branch_on_the_device(eng, ref):
    exe, d = ref
    rng = np.random.default_rng(77)
    n = 3000
    cov, regions, begin, end, median = U.chimeric_piles(rng, n, region_free=0.3)
    lists = U.overlap_lists(rng, begin, end, None)
    inp = U.StageInput(lists, cov, regions, begin, end, median, np.zeros(n, np.uint8))
    want1 = U.run_program(exe, inp, d, "gen1", phases=1)
    want = U.run_program(exe, inp, d, "gen3", phases=3)
    got = inp.device(eng, phases=3)
    U.assert_same(got, want)
    U.assert_same(inp.device(eng, phases=1), want1)
    # phase 2 drops overlaps and marks contained piles, and every outcome of ClearChimericRegions occurs
    st = got["stats"]
    assert st["dropped_by_update"][1] > 100 and st["contained"][0] > 100 and st["contained"][1] > 100
    counts = U.count_outcomes(inp, got, skip=want1["invalid"])
    print(counts, st)
    for k in U.OUTCOMES:
        assert counts[k] >= 10, (k, counts)
    # the pile-only input of the CPU test (no lists): the header on the device's lane 0 equals its host build
    cov, regions, begin, end, median = U.chimeric_piles(np.random.default_rng(2024), n)
    inp = U.StageInput([np.zeros(0, hip.OVERLAP_DTYPE)] * n, cov, regions, begin, end, median, np.zeros(n, np.uint8))
    U.assert_same(inp.device(eng, phases=2), U.run_program(exe, inp, d, "gen2", phases=2))


def _small(n=4, cells=300, level=30):
    z = np.zeros(0, hip.OVERLAP_DTYPE)
    return dict(lists=[z] * n, coverage=[np.full(cells, level, np.uint16) for _ in range(n)], regions=[[] for _ in range(n)],
                begin=[0] * n, end=[cells - 1] * n, median=[level] * n, invalid=np.zeros(n, np.uint8))


def test_hand_built_cases(eng, ref):
    exe, d = ref
    # no overlaps at all
    inp = U.StageInput(**_small())
    U.assert_same(inp.device(eng), U.run_program(exe, inp, d, "h0"))
    # every pile invalid: no non-zero median, the state comes back unchanged (lists included)
    a = _small()
    a["invalid"] = np.ones(4, np.uint8)
    a["median"] = [0] * 4
    a["lists"] = [np.array([(0, 0, 2000, 1, 0, 2000, 5, 1)], hip.OVERLAP_DTYPE)] + a["lists"][1:]
    inp = U.StageInput(**a)
    got = inp.device(eng, phases=2)
    U.assert_same(got, U.run_program(exe, inp, d, "h1", phases=2))
    assert got["median"] == 0 and got["overlaps"].shape[0] == 1 and np.array_equal(got["coverage"], inp.coverage)
    assert np.array_equal(got["begin"], inp.begin) and got["invalid"].all()
    # a pile with 40 regions, every other one with a dip
    a = _small(n=2, cells=2000)
    regs = [(40 * k + 10, 40 * k + 20) for k in range(40)]
    for k in range(0, 40, 2):
        a["coverage"][0][40 * k + 15] = 2
    a["regions"][0] = regs
    inp = U.StageInput(**a)
    want = U.run_program(exe, inp, d, "h2")
    got = inp.device(eng)
    U.assert_same(got, want)
    assert int(got["region_offsets"][1]) == 20 and got["chimeric"][0] == 1
    # a list entry whose lhs_id is not its list's index; an id out of range
    a = _small()
    a["lists"] = [np.array([(1, 0, 2000, 2, 0, 2000, 5, 1)], hip.OVERLAP_DTYPE)] + a["lists"][1:]
    with pytest.raises(ValueError, match="lhs_id"):
        U.StageInput(**a).device(eng)
    a["lists"] = [np.array([(0, 0, 2000, 9, 0, 2000, 5, 1)], hip.OVERLAP_DTYPE)] + a["lists"][1:]
    with pytest.raises(ValueError, match="unknown pile"):
        U.StageInput(**a).device(eng)
    # the identity filter without the reads
    with pytest.raises(ValueError, match="reads"):
        U.StageInput(**_small()).device(eng, identity=0.5)
    rs = _reads_for(0.78)
    reads, p = _first_pass(eng, rs)
    with pytest.raises(ValueError, match="reads"):
        p.resolve(None, identity=0.78)
    p.close()


def test_second_pass_takes_the_resolved_state(eng, ref):
    """The hand-off to stage -4: FindOverlapsAndRepetetiveRegions fed with the device's resolved state equals the
    oracle's second pass fed with the restatement's."""
    exe, d = ref
    rs = _reads_for(0.0)
    reads, p = _first_pass(eng, rs)
    inp = _input_of_pass(p, rs)
    want = U.run_program(exe, inp, d, "handoff")
    got = p.resolve(None)
    p2 = eng.find_overlaps_and_repetitive_regions(reads, got["begin"] << 4, got["end"] << 4, got["invalid"], freq=0.001,
                                                  kmer_len=15)
    o2 = oracle.second_pass(15, 5, rs, want["begin"] << 4, want["end"] << 4, want["invalid"], freq=0.001, kmer_len=15)
    assert o2["overlaps"].shape[0] > 20 and np.array_equal(p2["overlaps"], o2["overlaps"])
    assert np.array_equal(p2["contained"], o2["contained"])
    for i in range(rs.n):
        assert np.array_equal(p2["kmers"][i], o2["kmers"][i]), i
    p.close()


@pytest.mark.parametrize("resident", [0, 1])
def test_facade_in_construct_graph_order(tmp_path, ref, resident):
    """tests/cpp/resolve_stage_test.cpp: FindOverlapsAndCreatePiles, TrimAndAnnotatePiles, ResolveContainedReads,
    ResolveChimericSequences through the facade; the pile dump and the list sizes after each function."""
    exe, d = ref
    prog = _build(tmp_path, "resolve_stage_test")
    rs = _reads_for(0.0)
    path = _write_reads(tmp_path, rs)
    r = subprocess.run([prog, path, "0", str(resident)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    inp = U.oracle_trimmed_input(rs)
    want = {"C": U.run_program(exe, inp, d, "fc1_%d" % resident, phases=1), "D": U.run_program(exe, inp, d, "fc3_%d" % resident, phases=3)}
    for tag in ("C", "D"):
        w = want[tag]
        exp = []
        for i in range(rs.n):
            lo, hi = int(inp.coverage_offsets[i]), int(inp.coverage_offsets[i + 1])
            exp.append("%s %d %d %d %d %d %d %d %d %d %d" % (
                tag, i, w["begin"][i], w["end"][i], inp.median[i], w["invalid"][i], w["contained"][i], w["chimeric"][i],
                int(w["region_offsets"][i + 1]) - int(w["region_offsets"][i]), _hash(w["coverage"][lo:hi]),
                int(w["offsets"][i + 1]) - int(w["offsets"][i])))
        assert [ln for ln in lines if ln.startswith(tag + " ")] == exp, tag
    assert "resolved overlaps %d" % want["C"]["overlaps"].shape[0] in lines
    assert lines[-1] == "lists 0"  # construct.cc:310
