"""The rest of the overlap phase over a device group (rvn_group_find_overlaps_and_repetitive_regions,
rvn_group_filter_overlaps_by_identity; raven_amd/csrc/group.hip) against the single-engine calls on the same input, with
1, 2 and 3 virtual ranks on the one GPU of the test box.  Every case runs in a child process under a time limit (a group
call that never returned would otherwise hold the whole suite): `python -m tests.test_gpu_group_pass2 <case> <args>`."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _run(*args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_group_pass2"] + [str(a) for a in args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("n_ranks", [1, 2, 3])
def test_group_second_pass_is_byte_identical_to_the_single_engine(n_ranks):
    out = _run("second_pass", n_ranks)
    assert out.count("identical") == 4, out  # identity {0, 0.78} x batch_bases {2^30, 120 kb}


def test_group_second_pass_equals_the_oracle():
    assert "oracle identical" in _run("oracle", 2)


@pytest.mark.parametrize("n_ranks", [1, 2, 3])
def test_group_identity_filter_is_byte_identical_to_the_single_engine(n_ranks):
    assert _run("identity", n_ranks).count("identical") == 3, n_ranks  # identity 0, 0.7, 0.9


def test_group_second_pass_degenerate_inputs():
    assert "degenerate ok" in _run("degenerate")


def test_group_facades_equal_the_single_device_templates(tmp_path):
    """pass 1 -> TrimAndAnnotatePiles -> FilterOverlapsByIdentity -> FindOverlapsAndRepetetiveRegions over a
    raven::DeviceGroup (include/raven_hip/multi_gpu.hpp) against the single-device facades, pile for pile."""
    from raven_amd import synth
    from tests.test_gpu_facade import _build, _write_reads
    from tests.test_gpu_pass2 import _repeat_genome
    exe = _build(tmp_path, "group_pass2_test")
    rs, _ = synth.make_reads(_repeat_genome(150_000, seed=71), 16, 5000, seed=72)
    rpath = _write_reads(tmp_path, rs)
    for n_ranks, identity, batch in [(2, 0.78, 1 << 30), (3, 0.0, 300_000)]:
        r = subprocess.run([exe, rpath, str(n_ranks), str(identity), str(batch)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.strip().split("\n")
        t = lines[0].split()
        assert t[:2] == ["ranks", str(n_ranks)] and t[4] == "0" and t[6] == "0" and int(t[8]) > 0, lines[0]
        f = lines[1].split()
        assert f[2] == "0" and int(f[4]) > 2000, lines[1]
        if identity:
            assert int(f[6]) < int(f[4]), lines[1]  # the filter dropped something
        p = lines[2].split()
        assert int(p[2]) > 100 and int(p[4]) > 0 and p[6] == "0" and p[8] == "0", lines[2]


def test_group_hifi_overlap_phase_on_two_ranks():
    """configs[4]'s shape (HiFi 15 kb reads, 40x, --identity 0.95) at 20 Mb: identity filter and second pass over two
    ranks, bit-identical to the single engine."""
    out = _run("hifi", 2, timeout=1200)
    assert "filter identical" in out and "pass2 identical" in out, out


# ---- the cases (child process) ----------------------------------------------------------------------------------------

def _same(got, want, n):
    assert np.array_equal(got["contained"], want["contained"])
    assert got["overlaps"].shape == want["overlaps"].shape, (got["overlaps"].shape, want["overlaps"].shape)
    assert np.array_equal(got["overlaps"], want["overlaps"])
    for i in range(n):
        assert np.array_equal(got["kmers"][i], want["kmers"][i]), i


def _batch_ends(valid_lengths, batch_bases):
    """Ends of the second pass's index batches over the valid reads (construct.cc:324-359: a batch closes at batch_bases)."""
    ends, acc = [], 0
    for i, x in enumerate(valid_lengths):
        acc += int(x)
        if i == len(valid_lengths) - 1 or acc >= batch_bases:
            ends.append(i + 1)
            acc = 0
    return ends


def _rank_cuts(valid_lengths, ends, world):
    """The group's ranges of the valid reads (group.hip): balanced by length x batches a read is mapped against."""
    batch_of = np.searchsorted(np.asarray(ends), np.arange(len(valid_lengths)), side="right")
    work = valid_lengths.astype(np.float64) * (len(ends) - batch_of)
    cum = np.concatenate([[0.0], np.cumsum(work)])
    cuts = [0] + [int(np.searchsorted(cum, cum[-1] * h / world, side="left")) for h in range(1, world)] + [len(valid_lengths)]
    return list(np.maximum.accumulate(cuts))


def _repeat_reads():
    from raven_amd import hip, synth
    from tests.test_gpu_pass2 import _pass1_regions, _repeat_genome
    g = _repeat_genome(60_000, seed=3)
    rs, _ = synth.make_reads(g, 14, 2500, seed=4)
    eng = hip.Engine(15, 5)
    rd = eng.upload(rs)
    begin, end, invalid = _pass1_regions(eng, rd)
    rng = np.random.default_rng(8)
    invalid = (invalid | (rng.random(rs.n) < 0.15)).astype(np.uint8)
    return rs, eng, rd, begin, end, invalid


def _case_second_pass(n_ranks):
    from raven_amd import hip
    rs, eng, rd, begin, end, invalid = _repeat_reads()
    grp = hip.Group([0] * n_ranks)
    # the small batch size cuts the VALID reads into several batches, one of whose ends falls strictly inside a rank's range
    vl = rs.lengths[invalid == 0]
    ends = _batch_ends(vl, 120_000)
    assert len(ends) >= 3
    if n_ranks > 1:
        cuts = _rank_cuts(vl, ends, n_ranks)
        assert any(lo < e < hi for e in ends[:-1] for lo, hi in zip(cuts[:-1], cuts[1:])), (ends, cuts)
    for identity in (0.0, 0.78):
        for batch in (1 << 30, 120_000):
            want = eng.find_overlaps_and_repetitive_regions(rd, begin, end, invalid, freq=0.01, identity=identity,
                                                            batch_bases=batch)
            got = grp.find_overlaps_and_repetitive_regions(rs, begin, end, invalid, freq=0.01, identity=identity,
                                                           batch_bases=batch)
            _same(got, want, rs.n)
            assert got["overlaps"].shape[0] > 50 and got["contained"].sum() > 0
            assert sum(int(k.sum()) for k in got["kmers"]) > 0
            print("identity %g batch %d overlaps %d identical" % (identity, batch, got["overlaps"].shape[0]))
    grp.close()


def _case_oracle(n_ranks):
    from oracle import oracle
    from raven_amd import hip
    rs, eng, rd, begin, end, invalid = _repeat_reads()
    grp = hip.Group([0] * n_ranks)
    got = grp.find_overlaps_and_repetitive_regions(rs, begin, end, invalid, freq=0.01, identity=0.78, batch_bases=120_000)
    want = oracle.second_pass(15, 5, rs, begin, end, invalid, freq=0.01, identity=0.78, batch_bases=120_000)
    want["overlaps"] = want["overlaps"].astype(hip.OVERLAP_DTYPE)
    _same(got, want, rs.n)
    print("oracle identical")


def _case_identity(n_ranks):
    from raven_amd import hip, synth
    g = synth.make_genome(50_000, seed=21)
    rs, _ = synth.make_reads(g, 12, 2500, seed=22)
    eng = hip.Engine(15, 5)
    rd = eng.upload(rs)
    p = eng.find_overlaps_and_create_piles(rd)
    ovl, off = p.overlaps()
    begin, end, median, invalid = p.trim_and_annotate(4)
    p.close()
    begin, end = (begin.astype(np.uint32) << 4), (end.astype(np.uint32) << 4)
    grp = hip.Group([0] * n_ranks)
    for identity in (0.0, 0.7, 0.9):
        want_o, want_off = eng.filter_overlaps_by_identity(rd, ovl, off, begin, end, invalid, identity)
        got_o, got_off = grp.filter_overlaps_by_identity(rs, ovl, off, begin, end, invalid, identity)
        assert np.array_equal(got_off, want_off) and np.array_equal(got_o, want_o)
        assert got_o.shape[0] <= ovl.shape[0] and (identity > 0.85 or got_o.shape[0] > 0)
        print("identity %g kept %d of %d identical" % (identity, got_o.shape[0], ovl.shape[0]))
    grp.close()


def _case_degenerate():
    from oracle import oracle
    from raven_amd import hip, synth
    g = synth.make_genome(30_000, seed=9)
    rs, _ = synth.make_reads(g, 10, 2000, seed=10)
    eng = hip.Engine(15, 5)
    rd = eng.upload(rs)
    full_b = np.zeros(rs.n, np.uint32)
    full_e = ((rs.lengths >> 4) << 4).astype(np.uint32)
    grp3, grp5 = hip.Group([0] * 3), hip.Group([0] * 5)

    def both(grp, inv, **kw):
        want = eng.find_overlaps_and_repetitive_regions(rd, full_b, full_e, inv, **kw)
        got = grp.find_overlaps_and_repetitive_regions(rs, full_b, full_e, inv, **kw)
        _same(got, want, rs.n)
        return got

    # every pile invalid: nothing to map, no rank has a valid read
    got = both(grp3, np.ones(rs.n, np.uint8))
    assert got["overlaps"].shape[0] == 0 and all(len(k) == 0 for k in got["kmers"])
    # every pile valid: the reference's `s == 0` (construct.cc:343-349) maps nothing
    got = both(grp3, np.zeros(rs.n, np.uint8))
    assert got["overlaps"].shape[0] == 0 and got["contained"].sum() == 0
    want = oracle.second_pass(15, 5, rs, full_b, full_e, np.zeros(rs.n, np.uint8))
    assert want["overlaps"].shape[0] == 0
    # one invalid pile: the whole pass, cut over the ranks
    inv = np.zeros(rs.n, np.uint8)
    inv[rs.n // 2] = 1
    assert both(grp3, inv)["overlaps"].shape[0] > 0
    # more ranks than valid reads (five ranks, three valid reads): two ranks map nothing
    inv = np.ones(rs.n, np.uint8)
    inv[[3, 40, 41]] = 0
    both(grp5, inv)
    # four valid reads over five ranks, with the identity filter on
    inv = np.ones(rs.n, np.uint8)
    inv[[5, 6, 7, 8]] = 0
    both(grp5, inv, identity=0.5)
    # an empty read set
    empty = types.SimpleNamespace(n=0, packed=np.zeros(1, np.uint64), word_offsets=np.zeros(1, np.uint64),
                                  lengths=np.zeros(0, np.uint32))
    got = grp3.find_overlaps_and_repetitive_regions(empty, np.zeros(0, np.uint32), np.zeros(0, np.uint32),
                                                    np.zeros(0, np.uint8))
    assert got["overlaps"].shape[0] == 0 and got["contained"].shape[0] == 0 and got["kmers"] == []
    o, off = grp3.filter_overlaps_by_identity(empty, np.zeros(0, hip.OVERLAP_DTYPE), np.zeros(1, np.uint32),
                                              np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8), 0.9)
    assert o.shape[0] == 0 and off.tolist() == [0]
    # a bad argument is refused before any rank starts, and the group stays usable
    with pytest.raises(ValueError):  # RVN_EINVAL
        grp3.find_overlaps_and_repetitive_regions(rs, full_b, full_e, inv, kmer_len=33)
    both(grp3, inv)
    grp3.close()
    grp5.close()
    print("degenerate ok")


def _case_hifi(n_ranks):
    from oracle import oracle
    from raven_amd import hip
    from tests.test_gpu_fullsize import _make
    g, rs, truth = _make(20_000_000, 40, 15000, "normal", (0.001, 0.002, 0.002), 0x5EED0021)
    eng = hip.Engine(15, 5)
    rd = eng.upload(rs)
    p = eng.find_overlaps_and_create_piles(rd)
    ovl, off = p.overlaps()
    begin, end, median, invalid = p.trim_and_annotate(4)
    p.close()
    begin, end = (begin.astype(np.uint32) << 4), (end.astype(np.uint32) << 4)
    grp = hip.Group([0] * n_ranks)
    want_o, want_off = eng.filter_overlaps_by_identity(rd, ovl, off, begin, end, invalid, 0.95)
    got_o, got_off = grp.filter_overlaps_by_identity(rs, ovl, off, begin, end, invalid, 0.95)
    assert np.array_equal(got_off, want_off) and np.array_equal(got_o, want_o)
    assert 0.9 * ovl.shape[0] < got_o.shape[0] <= ovl.shape[0]
    print("filter identical: %d of %d kept" % (got_o.shape[0], ovl.shape[0]))
    upd, ok, ty = oracle.overlap_update_and_type(want_o.astype(oracle.OVERLAP_DTYPE), begin, end, invalid.astype(np.uint8))
    contained = np.zeros(rs.n, bool)
    contained[upd["lhs_id"][(ok == 1) & (ty == 1)]] = True
    contained[upd["rhs_id"][(ok == 1) & (ty == 2)]] = True
    inv2 = (invalid | contained).astype(np.uint8)
    want = eng.find_overlaps_and_repetitive_regions(rd, begin, end, inv2, freq=0.001, kmer_len=15, identity=0.95)
    got = grp.find_overlaps_and_repetitive_regions(rs, begin, end, inv2, freq=0.001, kmer_len=15, identity=0.95)
    _same(got, want, rs.n)
    assert got["overlaps"].shape[0] > 1000
    print("pass2 identical: %d overlaps, %d reads newly contained" % (got["overlaps"].shape[0], got["contained"].sum()))
    grp.close()


if __name__ == "__main__":
    case, rest = sys.argv[1], [int(a) for a in sys.argv[2:]]
    globals()["_case_" + case](*rest)
