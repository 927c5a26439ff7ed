"""The crafted windows of tests/poa_cases.py on the GPU, through Engine.poa_consensus_batch: every kernel of the window
consensus chain — rows on lanes with 32 columns (poa4.hip, mode 9), 64 / 128 / 256 columns (poa2.hip, modes 2 / 3 / 4),
full matrix (poa.hip, mode 1) and the chain itself (mode 0) — must put every window on the side of its limits the case
states: status byte, reason of a hand-on, and the oracle's consensus byte for byte (the backbone where a window cannot
be polished).  tests/test_poa_cases.py holds the generators to their names and the emulated first attempt to the same
outcomes on the CPU.  The only outcome left open is a `band` window in a band WIDER than the one it is clearly outside of:
where a walk counts as near a band's edge is a heuristic of the kernels, so such a window may be polished (then exactly) or
handed on."""
import numpy as np
import pytest

from raven_amd import hip

from . import poa_cases as pc
from .test_poa_cases import check_first_attempt

pytestmark = pytest.mark.gpu

CASES = pc.cases()
MAIN = [c for c in CASES if not c["alone"] and c["trim"]]       # one batch: backbones of 1 .. 200 bases
NO_TRIM = [c for c in CASES if not c["alone"] and not c["trim"]]
NODES = {b: [c for c in CASES if c["family"] == "nodes" and len(c["window"]["layers"][0]) == b] for b in (85, 100)}
LENGTH = [c for c in CASES if c["family"] == "length" and c["alone"]]
BATCHES = [MAIN, NO_TRIM, NODES[85], NODES[100], LENGTH]
WIDTH = {2: 64, 3: 128, 4: 256}


def _run(eng, cases):
    cons, status, _ = eng.poa_consensus_batch([c["window"] for c in cases], trim=cases[0]["trim"])
    return cons, status


def _byte(status):
    return [int(s) & 0xFF for s in status]


def _check_final(case, cons, status):
    assert (int(status) & 0xFF) == case["final"], (case["name"], hex(int(status)))
    assert np.array_equal(cons, pc.expected(case)), case["name"]


def test_first_attempt_alone():
    """Mode 9: what the emulator is held to on the CPU, from the kernel itself."""
    eng = hip.Engine()
    eng.poa_set_mode(9)
    for batch in BATCHES:
        cons, status = _run(eng, batch)
        for c, out, st in zip(batch, cons, status):
            check_first_attempt(c, out, st)


@pytest.mark.parametrize("mode", [2, 3, 4], ids=["64_columns", "128_columns", "256_columns"])
def test_one_band_width_alone(mode):
    """A window within the graph limits of poa2.hip whose path stays within 12 columns of the straight guide (every case
    but the `band` family's `beyond` ones: the claims the CPU suite asserts) is polished, exactly, by every width — the
    kernel hands on a walk within two columns of a band's edge, and half of the narrowest band is 32.  A window clearly
    outside a width is handed on by it and by every narrower one.  An in-edge of 33 computed rows is beyond the 64-column
    kernel's ring (status 7, the 128-column kernel's job) and nobody else's.  A layer of up to kPoa2MaxSeq = 896 bases is
    the banded kernels' own (polished, exactly); one base more is status 4 and the backbone from each of them."""
    eng = hip.Engine()
    eng.poa_set_mode(mode)
    for batch in BATCHES:
        cons, status = _run(eng, batch)
        for c, out, st in zip(batch, cons, status):
            b = int(st) & 0xFF
            if c["final"] != 1:  # beyond a graph limit: the status of the limit and the backbone, from every kernel
                assert b == c["final"] and np.array_equal(out, pc.expected(c)), (c["name"], hex(int(st)))
            elif max(len(x) for x in c["window"]["layers"]) > pc.P2_MAX_SEQ:
                assert b == 4 and np.array_equal(out, c["window"]["layers"][0]), (c["name"], hex(int(st)))
            elif c["family"] == "band" and c["band"]:
                if c["band"] >= WIDTH[mode]:
                    assert b == 8, (c["name"], hex(int(st)))
                else:  # (the documented exception: a wider band may still call the walk near its edge)
                    assert b in (1, 8), (c["name"], hex(int(st)))
                    if b == 1:
                        assert np.array_equal(out, pc.expected(c)), c["name"]
            elif c["name"] == "in_edge_ranks:plain_%d" % (pc.P2_RING + 1) and mode == 2:
                assert b == 7, (c["name"], hex(int(st)))
            else:
                assert b == 1 and np.array_equal(out, pc.expected(c)), (c["name"], hex(int(st)))


def test_full_matrix_alone():
    """Mode 1: every window of up to 1024 bases is exact; the limits of the graph and of the length are reported."""
    eng = hip.Engine()
    eng.poa_set_mode(1)
    for batch in BATCHES:
        cons, status = _run(eng, batch)
        for c, out, st in zip(batch, cons, status):
            _check_final(c, out, st)


@pytest.mark.parametrize("rows_min", [0, -1], ids=["rows_on_lanes_first", "default"])
def test_the_chain(rows_min):
    """Mode 0: every window ends with its stated status and bytes, and the chain's counters are what the kernels alone
    predict: handed on by the 32 columns = mode 9's status 8; through the 128 columns = mode 2's status 8 and 7; beyond them
    = mode 3's status 8 and the windows beyond a graph limit.  Of the `length` batch exactly the four windows of more than
    896 bases leave the banded kernels."""
    eng = hip.Engine()
    alone = {}
    for mode in (9, 2, 3):
        eng.poa_set_mode(mode)
        alone[mode] = np.asarray(_byte(_run(eng, MAIN)[1]))
    eng.poa_set_mode(0)
    eng.set_option("poa_rows_min_windows", rows_min)
    for batch in BATCHES:
        cons, status = _run(eng, batch)
        for c, out, st in zip(batch, cons, status):
            _check_final(c, out, st)
        if batch is MAIN:
            limits = sum(c["final"] in (2, 3, 4) for c in MAIN)
            assert eng.poa_narrow_windows() == (int(np.sum(alone[9] == 8)) if rows_min == 0 else 0)
            assert eng.poa_wide_windows() == int(np.sum((alone[2] == 8) | (alone[2] == 7)))
            assert eng.poa_fallback_windows() == int(np.sum(alone[3] == 8)) + limits
            assert int(np.sum(alone[2] == 7)) == 1 and int(np.sum(alone[3] == 8)) >= 2 and limits == 1
        if batch is LENGTH:
            # 895 and 896 bases are the first kernel's; 897, 1023, 1024 and 1025 are status 4 there and go straight to the
            # full-matrix kernel (which polishes the first three): no band is tried again for them
            beyond_banded = sum(len(c["window"]["layers"][0]) > pc.P2_MAX_SEQ for c in LENGTH)
            assert beyond_banded == 4
            assert (eng.poa_narrow_windows(), eng.poa_wide_windows(), eng.poa_fallback_windows()) == (0, 0, beyond_banded)


def test_groups_give_the_bytes_of_the_windows_alone():
    """The same windows as batches of 1, 3, 4, 5 and 9, a hand-on at each place of a group of four, a window that cannot be
    polished among polishable ones: window for window the bytes and the status of the window run alone (and what the case
    states), from the first attempt and from the chain."""
    eng = hip.Engine()
    eng.set_option("poa_rows_min_windows", 0)
    for mode in (9, 0):
        eng.poa_set_mode(mode)
        for name, members in pc.groups():
            cs = [pc.by_name(n) for n in members]
            cons, status = _run(eng, cs)
            for k, (c, out, st) in enumerate(zip(cs, cons, status)):
                if mode == 9:
                    check_first_attempt(c, out, st)
                else:
                    _check_final(c, out, st)
                one, st1 = _run(eng, [c])
                assert _byte(st1)[0] == _byte([st])[0] and np.array_equal(one[0], out), (name, k, c["name"])
