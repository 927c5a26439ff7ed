"""GPU: compact_overlap_list (pass2.hip), the one keep-flags -> survivors step of the overlap phase's device stages
(kept_slots = exclusive_scan_u8_u32 + the count read back, compact_overlaps = the scatter, DevBuf::swap), on its own through
rvn_test_compact_overlap_list of libraven_hip_test.so.  Sizes around the scan's tile (256 threads x 16 items), every keep
pattern once alone and once followed by a second application on the same three buffers, so that list and spare change
places in both directions.  Everything is compared with numpy for equality, order and every byte of a record included.
"""
import numpy as np
import pytest

from raven_amd import hip

pytestmark = pytest.mark.gpu

TILE = 4096  # items per block of the scan
SIZES = [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
PATTERNS = ["all", "none", "every_second", "random"]


@pytest.fixture(scope="module")
def gpu():
    if hip.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return True


def _overlaps(n, seed):
    """n records whose 32 bytes are all random: a survivor in the wrong place or a torn copy cannot go unnoticed."""
    words = np.random.default_rng(seed).integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    return np.ascontiguousarray(words).view(hip.OVERLAP_DTYPE).reshape(n)


def _keep(pattern, n, seed):
    if pattern == "all":
        return np.ones(n, np.uint8)
    if pattern == "none":
        return np.zeros(n, np.uint8)
    if pattern == "every_second":
        return (np.arange(n) % 2 == 0).astype(np.uint8)
    return np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)


def _scan(keep):
    return np.concatenate(([0], np.cumsum(keep, dtype=np.uint64))).astype(np.uint32)


def _same(got, want):
    return got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_compact_overlap_list(gpu, n, pattern):
    assert hip.OVERLAP_DTYPE.itemsize == 32
    ovl = _overlaps(n, seed=1000 + n)
    keep1 = _keep(pattern, n, seed=n)
    want1 = ovl[keep1 == 1]
    # one application
    got, slot = hip.test_compact_overlap_list(ovl, keep1)
    assert got.shape[0] == int(keep1.sum())
    assert _same(got, want1)
    assert np.array_equal(slot, _scan(keep1))
    # ... and a second one on its survivors: every third stays
    keep2 = (np.arange(want1.shape[0]) % 3 == 0).astype(np.uint8)
    got, slot = hip.test_compact_overlap_list(ovl, keep1, keep2)
    assert got.shape[0] == int(keep2.sum())
    assert _same(got, want1[keep2 == 1])
    assert np.array_equal(slot, _scan(keep2))
