"""The scratch-release paths of the engine (rvn_engine_release_scratch, the option release_always, what a failed polishing
round leaves behind): every state group hands its device buffers back AND forgets what it knew about their contents, and
whatever runs afterwards computes what it computed before.

Small shapes throughout; no_arena=1 wherever release_always is set, so that no test starts an arena on a shared device."""
import os

import numpy as np
import pytest

from raven_amd import hip
from tests import polish_util

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAMBDA_FASTQ = os.path.join(GOLDEN, "ERA476754.fastq.gz")


@pytest.fixture(scope="module")
def case():
    """(targets, reads) of one small polishing round, shared and never changed."""
    _, _, targets, reads, _ = polish_util.make_case(genome_len=20_000, coverage=20, read_len=3000)
    return targets, reads


def _round(eng, td, rd):
    cons, _, _ = eng.polish_round(td, rd)
    return [c.copy() for c in cons], eng.polish_layers()


def _same_round(a, b):
    assert np.array_equal(a[1], b[1]), "window layers differ"
    assert len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0])), "consensus differs"


def _pass1(eng, rd):
    p = eng.find_overlaps_and_create_piles(rd)
    try:
        return p.piles() + p.overlaps()
    finally:
        p.close()


def test_polishing_round_repeats_byte_for_byte_across_a_release(case):
    eng = hip.Engine(15, 5)
    td, rd = eng.upload(case[0]), eng.upload(case[1])
    first = _round(eng, td, rd)
    assert first[1].shape[0] > 0 and len(first[0][0]) > 0
    eng.release_scratch()
    _same_round(first, _round(eng, td, rd))


def test_pass1_across_forced_releases_equals_an_engine_that_never_releases(lambda_reads, case):
    """release_always: every stage entry hands the scratch back — the first pass's to the polishing round, the round's to the
    second pass."""
    plain = hip.Engine(15, 5)
    want = _pass1(plain, plain.upload(lambda_reads))
    assert want[2].shape[0] > 0
    eng = hip.Engine(15, 5)
    eng.set_option("no_arena", 1)
    eng.set_option("release_always", 1)
    rd = eng.upload(lambda_reads)
    before = _pass1(eng, rd)
    _round(eng, eng.upload(case[0]), eng.upload(case[1]))
    after = _pass1(eng, rd)
    for got in (before, after):
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_nothing_is_left_after_a_release(lambda_reads, case):
    """Input text, sketches, index, Map result, the round's tables and every stage's scratch: all of it goes back, none of
    it is the loaded read set's."""
    eng = hip.Engine(15, 5)
    loaded = eng.load(LAMBDA_FASTQ)
    eng.minimize(loaded)
    eng.map_batch(loaded, 0, min(loaded.n, 64))
    _round(eng, eng.upload(case[0]), eng.upload(case[1]))
    assert hip.test_engine_scratch_bytes(eng) > 0
    eng.release_scratch()
    assert hip.test_engine_scratch_bytes(eng) == 0
    packed, woff, lens, _, _, _ = loaded.fetch()
    assert np.array_equal(lens, lambda_reads.lengths) and np.array_equal(woff, lambda_reads.word_offsets)
    assert np.array_equal(packed, lambda_reads.packed[: int(lambda_reads.word_offsets[-1])])


def test_descriptors_are_reset_with_their_buffers(lambda_reads, case):
    eng = hip.Engine(15, 5)
    cons, layers = _round(eng, eng.upload(case[0]), eng.upload(case[1]))
    assert layers.shape[0] > 0
    eng.polish_output_as_reads([len(c) for c in cons]).close()
    n = eng.shard_sketch_count(eng.upload(lambda_reads))
    assert n > 0
    eng.release_scratch()
    assert eng.polish_layers().shape[0] == 0
    with pytest.raises((ValueError, hip.RavenHipError)):
        eng.polish_output_as_reads([len(c) for c in cons])
    # the sketch is gone and so is its count: the host-pointer fetch has nothing to copy and writes nothing
    sentinel = 0xA5A5A5A5A5A5A5A5
    values, origins = np.full(n, sentinel, dtype=np.uint64), np.full(n, sentinel, dtype=np.uint64)
    assert hip.lib().rvn_shard_sketch_fetch(eng._h, hip._p(values), hip._p(origins)) == hip.RVN_OK
    assert (values == sentinel).all() and (origins == sentinel).all()


def test_a_failed_round_invalidates_the_resident_consensus(case):
    """A round that fails behind the point where it starts to overwrite the stitched consensus (here: the caller's buffer is
    too small for target 0) must not leave the previous round's offsets over the new bytes: rvn_polish_output_as_reads
    refuses until a further complete round has run."""
    eng = hip.Engine(15, 5)
    td, rd = eng.upload(case[0]), eng.upload(case[1])
    cons, _ = _round(eng, td, rd)
    eng.polish_output_as_reads([len(c) for c in cons]).close()
    nt = td.n
    ooff = np.zeros(nt + 1, dtype=np.uint64)
    np.cumsum(2 * case[0].lengths.astype(np.uint64) + 1024, out=ooff[1:])
    ooff[1:] -= ooff[1] - 8  # target 0 gets eight bytes
    out, out_len = np.zeros(int(ooff[-1]) + 1, dtype=np.uint8), np.zeros(nt, dtype=np.uint32)
    ratio, stats = np.zeros(nt, dtype=np.float64), np.zeros(16, dtype=np.uint64)
    rc = hip.lib().rvn_polish_round(eng._h, td._h, rd._h, None, None, 0.0, 0.3, 500, 1, 3, -5, -4, hip._p(out), hip._p(ooff),
                                    hip._p(out_len), hip._p(ratio), hip._p(stats))
    assert rc == hip.RVN_EINVAL
    with pytest.raises((ValueError, hip.RavenHipError)):
        eng.polish_output_as_reads([len(c) for c in cons])
    cons2, _ = _round(eng, td, rd)
    a = eng.upload_codes(cons2).fetch()
    b = eng.polish_output_as_reads([len(c) for c in cons2]).fetch()
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
