"""raven::ResolveContainedReads / ResolveChimericSequences (RavenLib/src/construct.cc:154-314) without a GPU:
  * raven_amd/csrc/chimeric.h — Pile::ClearChimericRegions + UpdateValidRegion as the device's lane 0 runs them — built
    for the host (tests/host/resolve_pile.cpp) against the restatement (tests/host/resolve_reference.cpp) on generated
    piles that take every branch;
  * the restatement against the Python statement of the same stage in tests/test_gpu_stages.py (_oracle_stages), which
    the construct-stage test already trusts: one yardstick pinned to the other."""
import numpy as np
import pytest

from tests import resolve_util as U

N_PILES = 3000
MIN_COUNT = 50


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("resolve_host")
    return U.build_reference(d), U.build_pile_program(d), d


def _piles_input(seed, n):
    rng = np.random.default_rng(seed)
    cov, regions, begin, end, median = U.chimeric_piles(rng, n)
    return U.StageInput([np.zeros(0, U.hip.OVERLAP_DTYPE)] * n, cov, regions, begin, end, median, np.zeros(n, np.uint8))


def test_generated_piles_take_every_branch_of_the_restatement(programs):
    ref, _, d = programs
    inp = _piles_input(2024, N_PILES)
    want = U.run_program(ref, inp, d, "branches", mode="piles")
    counts = U.count_outcomes(inp, want)
    print(counts)
    for k in U.OUTCOMES:
        assert counts[k] >= MIN_COUNT, (k, counts)


@pytest.mark.parametrize("seed", [2024, 7, 99])
def test_chimeric_header_matches_the_restatement(programs, seed):
    ref, pile, d = programs
    inp = _piles_input(seed, N_PILES)
    want = U.run_program(ref, inp, d, "ref%d" % seed, mode="piles")
    got = U.run_program(pile, inp, d, "hdr%d" % seed, mode=None)
    U.assert_same(got, want, stats=False)
    assert got["stats"]["cut"] == want["stats"]["cut"] and got["stats"]["invalidated"] == want["stats"]["invalidated"]
    assert want["stats"]["cut"] > 1000 and want["stats"]["invalidated"] >= MIN_COUNT


def test_chimeric_header_on_edge_piles(programs):
    """No region at all, a region that is the whole valid region, regions that touch its ends, a valid region shorter
    than 78 cells, adjacent resolved regions, a median of 0 and of 65535."""
    ref, pile, d = programs
    z = np.zeros(0, U.hip.OVERLAP_DTYPE)
    cov = [np.full(300, 30, np.uint16) for _ in range(8)]
    cov[2][100:110] = 3
    cov[3][0:5] = 1
    cov[3][295:300] = 1
    cov[5][50:60] = 2
    cov[5][61:70] = 2
    regions = [[], [(0, 299)], [(100, 109)], [(0, 4), (295, 299)], [(10, 20)], [(50, 60), (61, 70)], [(5, 9)], [(5, 9)]]
    begin = [0, 0, 0, 0, 100, 0, 0, 0]
    end = [300, 299, 300, 299, 150, 300, 300, 300]
    median = [40, 40, 40, 40, 40, 40, 0, 65535]
    inp = U.StageInput([z] * 8, cov, regions, begin, end, median, np.zeros(8, np.uint8))
    want = U.run_program(ref, inp, d, "edge_ref", mode="piles")
    got = U.run_program(pile, inp, d, "edge_hdr", mode=None)
    U.assert_same(got, want, stats=False)
    assert want["invalid"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    assert (int(want["begin"][2]), int(want["end"][2])) == (109, 300) and want["chimeric"][2] == 1
    assert want["chimeric"][6] == 0 and want["chimeric"][7] == 1


def test_restatement_matches_the_python_statement_of_stage_minus_5(programs):
    """tests/test_gpu_stages.py::_oracle_stages states the same stage in Python with the oracle's primitives; on its read
    set the pile state after ResolveChimericSequences is the restatement's."""
    from tests.test_gpu_stages import _chimeric_reads, _oracle_stages
    ref, _, d = programs
    rs = _chimeric_reads(301, 5000)
    inp = U.oracle_trimmed_input(rs)
    got = U.run_program(ref, inp, d, "stages", phases=3, identity=0.0)
    stated = _oracle_stages(rs, 0.0)
    want = stated["B"]
    assert len(want) == rs.n
    for i, (idx, b, e, med, inv, con, chi, nreg, data) in enumerate(want):
        assert idx == i
        assert (int(got["begin"][i]), int(got["end"][i]), int(got["invalid"][i]), int(got["contained"][i]),
                int(got["chimeric"][i])) == (b, e, inv, con, chi), i
        assert int(got["region_offsets"][i + 1]) - int(got["region_offsets"][i]) == nreg, i
        assert int(inp.median[i]) == med
        lo, hi = int(inp.coverage_offsets[i]), int(inp.coverage_offsets[i + 1])
        assert np.array_equal(got["coverage"][lo:hi], data), i
    assert got["overlaps"].shape[0] == 0 and not got["offsets"].any()
    # the lists after ResolveContainedReads alone: as many as the Python statement keeps
    got1 = U.run_program(ref, inp, d, "stages1", phases=1, identity=0.0)
    assert got1["overlaps"].shape[0] == stated["resolved"]
    assert got["invalid"].sum() > 5 and (1 - got["invalid"]).sum() > 10 and got["contained"].sum() > 3

