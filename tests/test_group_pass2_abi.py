"""The C ABI of the overlap phase's second half over a device group (include/raven_hip.h:
rvn_group_find_overlaps_and_repetitive_regions, rvn_group_filter_overlaps_by_identity) without a GPU: both calls are
exported, refuse bad arguments before they touch the group, and a group cannot be made without a device."""
import ctypes as C

import numpy as np
import pytest

from raven_amd import hip

NEW = ["rvn_group_find_overlaps_and_repetitive_regions", "rvn_group_filter_overlaps_by_identity"]


def test_new_group_calls_are_exported_and_declared():
    L = hip.lib()
    for name in NEW:
        assert hasattr(L, name) and name in hip.SYMBOLS
        assert hasattr(hip.test_lib(), name)


def _reads():
    lengths = np.array([40, 33], np.uint32)
    woff = np.array([0, 2, 4], np.uint64)
    return np.zeros(5, np.uint64), woff, lengths


def test_null_group_or_arrays_are_refused():
    L = hip.lib()
    packed, woff, lengths = _reads()
    b, e, inv = np.zeros(2, np.uint32), np.full(2, 32, np.uint32), np.zeros(2, np.uint8)
    out = C.c_void_p()
    p = hip._p
    # NULL group
    assert L.rvn_group_find_overlaps_and_repetitive_regions(None, p(packed), p(woff), p(lengths), 2, p(b), p(e), p(inv), 0.001,
                                                            15, 0.0, 1 << 30, C.byref(out)) == hip.RVN_EINVAL
    assert "NULL argument" in L.rvn_last_error().decode()
    off = np.zeros(3, np.uint32)
    assert L.rvn_group_filter_overlaps_by_identity(None, p(packed), p(woff), p(lengths), 2, None, p(off), p(b), p(e), p(inv),
                                                   0.9) == hip.RVN_EINVAL
    # NULL arrays (the arguments are checked before the group is looked at: a stand-in handle is never dereferenced)
    fake = C.create_string_buffer(64)
    g = C.cast(fake, C.c_void_p)
    for args in [(None, p(woff), p(lengths)), (p(packed), None, p(lengths)), (p(packed), p(woff), None)]:
        assert L.rvn_group_find_overlaps_and_repetitive_regions(g, *args, 2, p(b), p(e), p(inv), 0.001, 15, 0.0, 1 << 30,
                                                                C.byref(out)) == hip.RVN_EINVAL
        assert L.rvn_group_filter_overlaps_by_identity(g, *args, 2, None, p(off), p(b), p(e), p(inv), 0.9) == hip.RVN_EINVAL
    assert L.rvn_group_find_overlaps_and_repetitive_regions(g, p(packed), p(woff), p(lengths), 2, None, p(e), p(inv), 0.001,
                                                            15, 0.0, 1 << 30, C.byref(out)) == hip.RVN_EINVAL
    assert L.rvn_group_find_overlaps_and_repetitive_regions(g, p(packed), p(woff), p(lengths), 2, p(b), p(e), p(inv), 0.001,
                                                            15, 0.0, 1 << 30, None) == hip.RVN_EINVAL
    assert L.rvn_group_filter_overlaps_by_identity(g, p(packed), p(woff), p(lengths), 2, None, None, p(b), p(e), p(inv),
                                                   0.9) == hip.RVN_EINVAL
    # overlaps announced by the offsets but not passed
    off_one = np.array([0, 1, 1], np.uint32)
    assert L.rvn_group_filter_overlaps_by_identity(g, p(packed), p(woff), p(lengths), 2, None, p(off_one), p(b), p(e), p(inv),
                                                   0.9) == hip.RVN_EINVAL
    # out-of-range parameters and inconsistent read arrays
    for freq, k, batch in [(1.5, 15, 1 << 30), (0.001, 0, 1 << 30), (0.001, 33, 1 << 30), (0.001, 15, 0)]:
        assert L.rvn_group_find_overlaps_and_repetitive_regions(g, p(packed), p(woff), p(lengths), 2, p(b), p(e), p(inv), freq,
                                                                k, 0.0, batch, C.byref(out)) == hip.RVN_EINVAL
    short = np.array([0, 1, 4], np.uint64)  # read 0 has 40 bases: two words, not one
    assert L.rvn_group_find_overlaps_and_repetitive_regions(g, p(packed), p(short), p(lengths), 2, p(b), p(e), p(inv), 0.001,
                                                            15, 0.0, 1 << 30, C.byref(out)) == hip.RVN_EINVAL
    ovl = np.zeros(1, hip.OVERLAP_DTYPE)
    ovl["rhs_id"] = 7  # no such read
    assert L.rvn_group_filter_overlaps_by_identity(g, p(packed), p(woff), p(lengths), 2, p(ovl), p(off_one), p(b), p(e),
                                                   p(inv), 0.9) == hip.RVN_EINVAL
    assert "unknown read" in L.rvn_last_error().decode()


def test_group_fails_loudly_without_gpu():
    if hip.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(hip.RavenHipError) as ei:
        hip.Group([0, 0])
    assert "no HIP device" in str(ei.value) or "device" in str(ei.value).lower()
