"""The op sink of the alignment-path walker (raven_amd/csrc/nwpath.h: NwWalkerT<Cells, NwRunSink>) without a GPU: the
walker + sink compiled for the host (tests/host/nw_ops.cpp) over a Cells that answers from a plain DP matrix, against a
traceback written here with the same tie rule (tests/nw_ops_util.py).  Every case runs with windows of 7 and of 500 target
bases: the walker cuts match runs at window, block and strip ends, the sink has to hand back maximal runs."""
import os
import subprocess

import numpy as np
import pytest

from tests import nw_ops_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = (7, 500)


def _mutate(rng, s, rate):
    out = []
    for c in s:
        r = rng.random()
        if r < rate / 3:
            out.append((c + 1 + rng.integers(0, 3)) % 4)
        elif r < 2 * rate / 3:
            out.extend([c, rng.integers(0, 4)])
        elif r < rate:
            pass
        else:
            out.append(c)
    return np.array(out, dtype=np.uint8)


def _cases():
    rng = np.random.default_rng(20)
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    cases = {}
    a = rnd(200)
    cases["identical_200"] = (a, a.copy())
    for n in (1, 31, 32, 33, 63, 64, 65):
        b = rnd(n)
        cases["len_%d" % n] = (_mutate(rng, b, 0.15) if n > 1 else b.copy(), b)
        cases["len_%d_vs_other" % n] = (rnd(max(1, n - 1)), b)
    b = rnd(300)
    cases["insertion_50"] = (np.concatenate((b[:120], rnd(50), b[120:])), b)
    cases["deletion_50"] = (np.concatenate((b[:120], b[170:])), b)
    cases["homopolymer"] = (np.zeros(90, np.uint8), np.zeros(130, np.uint8))
    hp = np.concatenate((rnd(40), np.full(60, 2, np.uint8), rnd(40)))
    cases["homopolymer_inside"] = (np.concatenate((hp[:50], hp[57:])), hp)
    tr = np.tile(np.array([0, 1], np.uint8), 80)
    cases["tandem_2"] = (tr[:-14], tr)
    cases["tandem_2_noisy"] = (_mutate(rng, tr, 0.1), tr)
    cases["unrelated_300_2000"] = (rnd(300), rnd(2000))
    cases["unrelated_2000_300"] = (rnd(2000), rnd(300))
    cases["ont_like_700"] = (_mutate(rng, rnd(700), 0.1), None)
    q, _ = cases["ont_like_700"]
    cases["ont_like_700"] = (_mutate(rng, q, 0.1), q)
    return cases


CASES = _cases()


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    """{(case, w): (status, distance, runs)} of one run of the host program over every case and window length"""
    tmp = tmp_path_factory.mktemp("nw_ops")
    exe = str(tmp / "nw_ops")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I",
                           os.path.join(ROOT, "raven_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "nw_ops.cpp")])
    text = lambda c: "".join("ACGT"[x] for x in c)
    keys = [(name, w) for name in CASES for w in WINDOWS]
    src = str(tmp / "cases.txt")
    with open(src, "w") as f:
        for name, w in keys:
            q, t = CASES[name]
            f.write("%d %s %s\n" % (w, text(t), text(q)))
    lines = subprocess.check_output([exe, src], text=True).splitlines()
    assert len(lines) == len(keys)
    out = {}
    for key, line in zip(keys, lines):
        v = [int(x) for x in line.split()]
        assert v[2] == len(v) - 3, (key, line)
        out[key] = (v[0], v[1], np.array(v[3:], dtype=np.uint32))
    return out


@pytest.fixture(scope="module")
def reference():
    return {name: U.dp_runs(q, t) for name, (q, t) in CASES.items()}


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_walker_runs_equal_traceback(walked, reference, name, w):
    status, d, runs = walked[(name, w)]
    want_d, want = reference[name]
    q, t = CASES[name]
    assert status == 0
    assert d == want_d
    assert len(runs) <= 2 * d + 1
    U.check_runs(runs, q, t, d)
    assert np.array_equal(runs, want), (runs[:8], want[:8])


def test_identical_is_one_run(walked):
    for w in WINDOWS:
        status, d, runs = walked[("identical_200", w)]
        assert (status, d, runs.tolist()) == (0, 0, [200 << 2])


def test_reference_breakpoints_match_oracle(reference):
    """the yardstick of the GPU test's second check, pinned here: breakpoints derived from runs = the oracle's"""
    from oracle import oracle
    for name in ("ont_like_700", "insertion_50", "unrelated_300_2000", "homopolymer_inside"):
        q, t = CASES[name]
        _, runs = reference[name]
        for w in WINDOWS:
            want, _ = oracle.nw_breakpoints(q, t, 5, 3, w)
            assert np.array_equal(U.breakpoints_from_runs(runs, 5, 3, 3 + len(t), w), want), (name, w)
