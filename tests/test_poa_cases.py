"""The crafted windows of tests/poa_cases.py on the CPU: every window is first held to what its generator names it after
(by oracle.poa_window_stats: the oracle says which graph a layer meets, no kernel is asked), the oracle's two statements
of the consensus — spoa's rules, and the device's row order with the smallest-node-id end rule — must give the same bytes
on it, and then the rows-on-lanes kernel (raven_amd/csrc/poa4.hip, stepped through by the host wavefront emulator, both
schedules) must report exactly the outcome the case states: the status byte, for a hand-on the reason in bits 24-27,
for a polished window the oracle's consensus byte for byte, for an unpolishable one the backbone.  No case accepts two
outcomes.  The GPU side of the same cases is tests/test_gpu_poa_limits.py."""
import numpy as np
import pytest

from raven_amd import hip

from . import poa_cases as pc

CASES = pc.cases()
IDS = [c["name"] for c in CASES]


def outcome(status):
    """(status byte, reason of a hand-on) of a status word."""
    s = int(status)
    return (s & 0xFF, (s >> 24) & 15 if (s & 0xFF) == 8 else 0)


def check_first_attempt(case, cons, status):
    assert outcome(status) == tuple(case["poa4"]), (case["name"], hex(int(status)))
    if case["poa4"][0] == 1:
        assert np.array_equal(cons, pc.expected(case)), case["name"]
    elif case["poa4"][0] != 8:
        assert np.array_equal(cons, case["window"]["layers"][0]), case["name"]


def test_every_family_has_its_cases():
    """Every family of the issue is there, and every limit that has a case at all has one inside (or at) it and one beyond."""
    fams = {c["family"] for c in CASES} | {"groups"}
    assert fams == set(pc.FAMILIES)
    sides = {}
    for c in CASES:
        sides.setdefault(c["limit"], set()).add(c["side"])
        if "also" in c:
            sides.setdefault(c["also"][0], set()).add(c["also"][1])
    for limit, s in sides.items():
        if limit in ("consensus", "end rule", "lbk > rho"):  # (no hand-on behind them: every case polishes)
            continue
        assert "beyond" in s and (s & {"inside", "at"}), (limit, s)
    assert len(pc.groups()) >= 9


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_generator_builds_what_it_is_named_after(case):
    st = pc.stats(case["window"])
    assert st["agree"], "the oracle's two statements differ on " + case["name"]
    assert pc.claims_hold(case, st) == []


# (layers of 900 bases take the emulator its longest: the `length` family goes through the persistent schedule alone)
RUNS = [(c, v) for c in CASES for v in (4, 5) if v == 5 or c["family"] != "length"]


@pytest.mark.parametrize("case,variant", RUNS, ids=["%s-%s" % (c["name"], "per_round" if v == 4 else "persistent") for c, v in RUNS])
def test_first_attempt_reports_the_stated_outcome(case, variant):
    cons, status = hip.poa_banded_emulate([case["window"]], trim=case["trim"], variant=variant)
    check_first_attempt(case, cons[0], status[0])


def test_trim_cases_have_the_stated_lengths():
    """The coverage trim at its rule: ends covered by exactly (layers - 1) / 2 sequences stay, one fewer and they go."""
    for c in CASES:
        if "length" in c:
            assert len(pc.expected(c)) == c["length"], c["name"]


def test_end_rule_case_depends_on_the_end_rule():
    """The case named after the end-node rule is one where the rule decides: the oracle with the LARGEST node id among equal
    scores gives other bytes than the stated consensus."""
    from oracle import oracle
    for c in CASES:
        if c.get("end_rule"):
            other = oracle.poa_window(c["window"]["layers"], device_order=True, end_tie=2)[0]
            assert not np.array_equal(other, pc.expected(c))


@pytest.mark.parametrize("group", pc.groups(), ids=[g[0] for g in pc.groups()])
def test_groups_give_the_bytes_of_the_windows_alone(group):
    """A wave carries four windows: whatever shares a wave with a window — a hand-on at any of the four places, a window
    that cannot be polished — each window comes back as it does alone."""
    cs = [pc.by_name(n) for n in group[1]]
    cons, status = hip.poa_banded_emulate([c["window"] for c in cs], variant=5)
    for c, out, st in zip(cs, cons, status):
        check_first_attempt(c, out, st)
