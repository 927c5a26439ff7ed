"""raven::EdgeSimilarity of include/raven_hip/graph_repr.hpp (tests/cpp/edge_similarity_test.cpp, g++ against doubles whose
node sequence counts its accesses) against the restatement (tests/host/edge_similarity_reference.cpp) on the same graphs:
every score equal by bit pattern, no node sequence ever read.  One process per graph."""
import os
import subprocess

import numpy as np
import pytest

from tests import edge_sim_util as eu
from tests.graph_util import ROOT, Reader

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("edge_similarity_facade")
    exe = str(d / "edge_similarity_test")
    lib = os.path.join(ROOT, "raven_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "edge_similarity_test.cpp"), "-L", lib, "-lraven_hip",
                           "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return eu.build_reference(d), exe, d


def _same(programs, case, tag, with_tiling):
    ref, exe, d = programs
    want = eu.reference(ref, case, d, tag)
    src, dst, til = str(d / (tag + ".fin")), str(d / (tag + ".fout")), str(d / (tag + ".til"))
    with open(src, "wb") as f:
        f.write(eu.reference_blob(case))
    args = [exe, src, dst]
    if with_tiling:
        soff, rd, bg, ln, st = case.tiling_arrays()
        with open(til, "wb") as f:
            f.write(b"".join([case.reads_blob(), np.uint32(case.n_nodes).tobytes(), soff.tobytes(), rd.tobytes(), bg.tobytes(),
                              ln.tobytes(), st.tobytes()]))
        args.append(til)
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = Reader(open(dst, "rb").read())
    score = rd.take(np.float64, len(case.table.tail))
    assert int(rd.one(np.uint64)) == 0 and rd.done()  # the accessor's count
    assert np.array_equal(eu.bits(score), eu.bits(want["score"]))
    return want


def test_the_hand_derived_graph(programs):
    case, hand = eu.hand_case()
    case.table.hole()
    want = _same(programs, case, "hand", with_tiling=False)
    assert want["score"][0] == 1.0 and want["score"][2] == 0.9 and np.isnan(want["score"][[8, 12]]).all()


def test_a_generated_graph_of_both_routes(programs):
    rng = np.random.default_rng(1)
    case = eu.overlap_case(rng, [int(x) for x in rng.integers(20, 1500, size=30)], 0.12, multi="mixed", flip=True)
    want = _same(programs, case, "generated", with_tiling=True)
    assert len(set(want["score"].tolist())) > 40
