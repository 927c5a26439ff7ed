"""raven::ResolveRepeatInducedOverlaps on the device (rvn_resolve_repeat_induced_overlaps, raven_amd/csrc/repeats.hip)
over the crafted cases of tests/repeat_cases.py, against RepeatRef, the plain Python statement of the reference that
tests/test_repeat_cases.py holds to the restatement program and to the host build of repeats.h: every field, order
included, integers, no tolerance.  One test per case, so that a failure names the class it belongs to; all piles of
family A in one call; and one engine over a large, a small and the large case again."""
import numpy as np
import pytest

from raven_amd import hip
from tests import repeat_cases as rc
from tests import repeats_util as ru

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    eng = hip.Engine(15, 5)
    yield eng
    eng.close()


@pytest.mark.parametrize("name", rc.names())
def test_case_matches_the_reference(name, engine):
    got = rc.stage_input(rc.by_name(name)).device(engine)
    ru.assert_same(got, rc.reference(name)[0])


def test_all_piles_of_family_a_in_one_call(engine):
    """Slots, retry slots and scratch of neighbouring piles do not interfere: the piles of 4096 and 4097 cells around
    the 0-cell pile in front, several piles beyond the first try behind them."""
    union, parts = rc.family_a_union()
    assert [len(c) for c in union["coverage"][:3]] == [4096, 0, 4097]
    got = rc.stage_input(union).device(engine)
    want = rc.reference("A:union")[0]
    ru.assert_same(got, want)
    assert want["components"] == len(union["coverage"]) and want["regions"].shape[0] > 40


def _bytes(res):
    return [np.ascontiguousarray(res[k]).tobytes() for k in ("overlaps", "regions", "region_offsets", "is_repetitive")] + \
        [res["iterations"], res["components"], res["removed"]]


def test_one_engine_over_a_large_a_small_and_the_large_case_again(engine):
    large, small = rc.stage_input(rc.by_name("C:replicated")), rc.stage_input(rc.by_name("C:mark:weak+setter"))
    first = large.device(engine)
    between = small.device(engine)
    again = large.device(engine)
    ru.assert_same(first, rc.reference("C:replicated")[0])
    ru.assert_same(between, rc.reference("C:mark:weak+setter")[0])
    assert _bytes(first) == _bytes(again)
