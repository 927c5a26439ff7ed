"""tests/align_cases.py held on the CPU: the generators are what their names say (from dp_runs alone), the predicted plan of
every attempt is nwplan.h's (the host program of tests/test_nw_plan.py), the comparison helper notices each defect it is
there for, and the small cases go through the CPU stepper of the sweep and the walk (hip.test_nw_breakpoints) — so that a
failure of tests/test_gpu_align_cases.py can be placed on one side of the stepper."""
import subprocess

import numpy as np
import pytest

from raven_amd import hip, seqio
from tests import align_cases as A
from tests import nw_ops_util as U
from tests import test_nw_plan as P


# ---- the generators ------------------------------------------------------------------------------------------------------
def test_threshold_cases_are_what_they_are_named():
    cases = A.threshold_cases()
    assert sorted(c.meta["dist"] for c in cases if c.name.startswith("thr_mismatch")) == [15, 16, 17, 32, 33, 64, 65]
    for c in cases:
        d, runs = A.reference(c)
        assert d == c.meta["dist"], c
        assert 120 <= max(c.n, c.m) <= 400
        k0 = A.threshold(0.0, c.n, c.m)
        assert k0 == max(16, abs(c.n - c.m))
        if "touch" in c.meta:  # the reference path runs on the outermost diagonal of the first band, which holds it
            lo, hi = P.band(c.n, c.m, k0)
            diag = A.diagonals(runs)
            assert d == k0
            assert (diag[0] == -lo) if c.meta["touch"] < 0 else (diag[1] == hi), (c, diag, lo, hi)
    by = {c.name: c for c in cases}
    assert P.band(216, 200, 16) == (0, 16) and P.band(200, 216, 16) == (16, 0)  # k == |n - m|: one side of width 0
    assert (by["thr_rows_16_more"].n, by["thr_rows_16_more"].m) == (216, 200)
    assert A.threshold(0.0, by["thr_rows_40_more"].n, by["thr_rows_40_more"].m) == 40
    far = by["thr_all_mismatch_200"]
    att = A.attempts(far.n, far.m, 200, 0.0)
    assert [a[3] for a in att] == [16, 32, 64, 128, 256] and att[-1][:2] == (1, 8)
    # 16 isolated mismatches; 8 inserted at the very start + 8 deleted at the very end and its mirror image
    assert len(A.reference(by["thr_mismatch_16"])[1]) == 33
    assert [int(r) & 3 for r in A.reference(by["thr_on_minus_lo"])[1][[0, -1]]] == [U.OP_I, U.OP_D]
    assert [int(r) & 3 for r in A.reference(by["thr_on_plus_hi"])[1][[0, -1]]] == [U.OP_D, U.OP_I]


def test_ring_edge_cases_are_the_edges_of_their_variants():
    cases = A.ring_edge_cases()
    assert len(cases) == 8 * 3 * 2
    for c in cases:
        R, G = c.meta["variant"]
        lvl = c.meta["level"]
        k = A.threshold(A.RATE_LARGE, c.n, c.m)
        assert k == c.n + c.m and P.plan(c.n, c.m, k, 64, 1 << 62)[:3] == (R, G, 0)
        d = c.n - c.m
        step = 2  # (n + m and n - m have one parity)
        if c.meta["edge"] == "high":  # the ring is full; the next pair of this n - m is the next variant's
            assert c.meta["lanes"] == G
            nxt = P.plan(c.n + 1, c.m + 1, k + step, 64, 1 << 62)
            assert nxt[:2] == (P.VARIANTS[lvl + 1] if lvl < 7 else (8, 64)) and (lvl < 7 or nxt[2] == 64)
        elif lvl > 0:
            prev = P.plan(c.n - 1, c.m - 1, k - step, 64, 1 << 62)
            assert prev[:2] == P.VARIANTS[lvl - 1], c
            if R == 1:
                assert c.meta["lanes"] == P.VARIANTS[lvl - 1][1] + 1  # one lane more than the ring before holds
        assert (d > 0, d < 0, d == 0) == (c.name.endswith("d37"), c.name.endswith("d-37"), c.name.endswith("d0"))
    no_dp = [c.name for c in list(cases) + list(A.ring_below_cases()) if c.cells > A.DP_MAX_CELLS]
    assert sorted(no_dp) == sorted(A.NO_DP_CASES) and len(no_dp) <= 4
    for c in A.ring_below_cases():
        assert A.threshold(c.meta["rate"], c.n, c.m) == c.meta["k"]
        assert P.plan(c.n, c.m, c.meta["k"], 64, 1 << 62)[:2] == c.meta["variant"]


@pytest.mark.parametrize("G", (4, 8, 16, 32))
def test_bundle_pools(G):
    pool = A.bundle_pool(G)
    NG = 64 // G
    assert len(pool) >= 2 * NG + 1
    for c in pool:
        assert P.plan(c.n, c.m, A.threshold(A.RATE_LARGE, c.n, c.m), 64, 1 << 62)[:3] == (1, G, 0), c
    first = pool[:max(NG, 2)]
    assert min(c.m for c in first) == 1 and max(c.m for c in first) == max(c.m for c in pool)  # one bundle: 1 .. most columns
    assert pool[0].n == 1 and P.plan(1, pool[0].m + 1, pool[0].m + 2, 64, 1 << 62)[:2] != (1, G)  # (no more columns fit)
    assert {(c.m + (c.n + 63) // 64) % 32 for c in pool} >= {0, 1, 15, 16, 17, 31}
    assert any(c.n == 1 and c.m > 1 for c in pool) and any(c.m == 1 for c in pool)
    assert any(len(set(c.q.tolist()) | set(c.t.tolist())) == 1 and c.m > 1 for c in pool)  # the homopolymer pair
    if G == 4:
        assert any(c.n == 1 and c.m == 1 for c in pool)
    sizes = [len(b) for _, b in A.bundle_batches(G)]
    assert sorted(set(sizes)) == sorted({1, NG - 1, NG, NG + 1, 2 * NG + 1} - {0})


def test_slot_cases_fill_their_slots():
    full, ordinary = A.slot_cases()
    for key, k in (("x16", 16), ("x32", 32), ("id16", 16), ("id32", 32)):
        d, runs = A.reference(full[key])
        assert d == k and len(runs) == 2 * k + 1 and len(runs) + 1 == 2 * k + 2  # runs + the count word = nw_slot_words(k)
        assert runs[0] & 3 == U.OP_EQ and runs[-1] & 3 == U.OP_EQ
        edits = runs[1::2]
        assert ((edits >> 2) == 1).all()  # every edit isolated
        if key.startswith("id"):
            assert [int(e) & 3 for e in edits] == [U.OP_I, U.OP_D] * (k // 2)
        assert [a[3] for a in A.attempts(full[key].n, full[key].m, d, 0.0)] == ([16] if k == 16 else [16, 32])


def test_path_kernel_cases_have_the_named_run_counts():
    cases = A.path_kernel_cases()
    assert sorted(c.meta["runs"] for c in cases if c.name.startswith("path_runs")) == [1, 3, 63, 64, 65, 255, 256, 257, 513]
    for c in cases:
        assert len(A.reference(c)[1]) == c.meta["runs"], c
    by = {c.name: c for c in cases}
    assert A.reference(by["path_one_run_70000"])[1].tolist() == [(70000 << 2) | U.OP_EQ]
    runs = A.reference(by["path_256_singles_then_5000"])[1]
    assert ((runs[:256] >> 2) == 1).all() and runs[256] == (5000 << 2) | U.OP_EQ
    assert A.reference(by["path_empty_query"])[1].tolist() == [(40 << 2) | U.OP_D]
    assert A.reference(by["path_empty_target"])[1].tolist() == [(70 << 2) | U.OP_I]


def test_small_pairs_of_the_repeat_and_walk_cases():
    rep = A.small_distinct(64, 40, 41, 20, seed=4200)
    assert len({(c.q.tobytes(), c.t.tobytes()) for c in rep}) == 64
    assert all(A.reference(c)[0] == 20 and c.n == c.m == 40 for c in rep)
    walk = A.small_distinct(64, 24, 41, None, seed=6464)
    assert all(24 <= c.n <= 40 and 24 <= c.m <= 40 for c in walk)
    assert all(A.reference(c)[0] <= A.threshold(1.0, c.n, c.m) for c in walk)  # one pass


# ---- the prediction against nwplan.h ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("align_cases")
    exe = str(d / "nw_plan_host")
    subprocess.check_call(P.BUILD + ["-O2", "-pthread", "-o", exe, P.SOURCE])
    return exe, d


def test_predicted_attempts_are_the_plans_of_nwplan_h(program):
    exe, d = program
    full, ordinary = A.slot_cases()
    queries = []  # (n, m, distance, rate, stripe lanes)
    for c in list(A.threshold_cases()) + list(full.values()) + ordinary + [c for c in A.path_kernel_cases() if 0 < c.cells <= 10 ** 6]:
        for sl in (64, 4, 1):
            queries.append((c.n, c.m, A.reference(c)[0], 0.0, sl))
    for c in A.ring_edge_cases():
        queries.append((c.n, c.m, 0, A.RATE_LARGE, 64))  # (k = n + m holds any distance)
    for c in A.ring_below_cases():
        queries.append((c.n, c.m, 0, c.meta["rate"], 64))
    for G in (4, 8, 16, 32):
        for c in A.bundle_pool(G):
            queries += [(c.n, c.m, 0, A.RATE_LARGE, 64), (c.n, c.m, 0, A.RATE_LARGE, 4)]
    text, lines = "", []
    for n, m, dist, rate, sl in queries:
        # the first term of the threshold by the model without a fit, then every attempt's plan
        text += "fit 0 %r 1\n%d\n" % (rate, max(n, m))
        lines += ["model -1 0 0", "thresholds %d" % (int(rate * max(n, m)) + 16)]
        att = A.attempts(n, m, dist, rate, stripe_lanes=sl, budget=1 << 40)
        assert att[0] is not None and att[0][3] == A.threshold(rate, n, m)
        k = int(rate * max(n, m)) + 16
        for a in att:
            text += "plan %d %d %d %d %d\n" % (n, m, k, sl, 1 << 40)
            lines.append("plan 0" if a is None else "plan 1 %d %d %d %d %d" % a)
            k = 2 * a[3] if a is not None else 0
    P._same(P._run(exe, text, str(d / "attempts.txt")), lines)


# ---- the comparison helper -------------------------------------------------------------------------------------------------
def _expected_batch():
    full, ordinary = A.slot_cases()
    items = [ordinary[0], full["id16"], A.threshold_cases()[7], ordinary[1]]
    return items, A.expected(items)


def _rejects(got, want):
    with pytest.raises(AssertionError):
        A.compare(got, want)


def test_compare_accepts_the_reference_and_notices_defects():
    items, (dist, off, runs, op_off, ops) = _expected_batch()
    A.compare((dist.copy(), off.copy(), runs.copy()), (dist, off, runs))
    A.compare((dist.copy(), op_off.copy(), ops.copy()), (dist, op_off, ops))
    # a distance off by one
    bad = dist.copy()
    bad[2] += 1
    _rejects((bad, off, runs), (dist, off, runs))
    # two neighbouring runs merged (their counts added)
    at = int(off[1]) + 3
    merged = np.concatenate((runs[:at], [((runs[at] >> 2) + (runs[at + 1] >> 2)) << 2 | (runs[at] & 3)], runs[at + 2:])).astype(np.uint32)
    off2 = off.copy()
    off2[2:] -= 1
    _rejects((dist, off2, merged), (dist, off, runs))
    # an 'I' and a 'D' swapped: same cost, same spans, another path
    at = int(off[1])
    assert (runs[at + 1], runs[at + 3]) == ((1 << 2) | U.OP_I, (1 << 2) | U.OP_D)
    swapped = runs.copy()
    swapped[at + 1], swapped[at + 3] = runs[at + 3], runs[at + 1]
    U.check_runs(swapped[at:int(off[2])], items[1].q, items[1].t, int(dist[1]))  # (the invariants alone accept it)
    _rejects((dist, off, swapped), (dist, off, runs))
    # one pair's runs shifted into its neighbour's range
    off3 = off.copy()
    off3[2] += 1
    _rejects((dist, off3, runs), (dist, off, runs))
    # a count one too large
    fat = runs.copy()
    fat[int(off[1]) + 2] += 4
    _rejects((dist, off, fat), (dist, off, runs))
    # one byte of the ops form changed
    ops2 = ops.copy()
    ops2[int(op_off[3]) - 1] ^= 1
    _rejects((dist, op_off, ops2), (dist, op_off, ops))


def test_counter_comparison_notices_a_missing_attempt():
    cases = A.threshold_cases()
    jobs = [(c.n, c.m, A.reference(c)[0]) for c in cases]
    plans, st, la = A.predict(jobs, 0.0)
    A.compare_counters(dict(st), dict(la), st, la)
    far = cases[-1]
    lo, hi = P.band(far.n, far.m, 128)
    short = dict(st, band_cells=st["band_cells"] - far.m * (lo + hi + 1))  # the attempt at k = 128 left out
    with pytest.raises(AssertionError):
        A.compare_counters(short, dict(la), st, la)
    with pytest.raises(AssertionError):
        A.compare_counters(dict(st), dict(la, nw_forward=la["nw_forward"] - 1), st, la)
    with pytest.raises(AssertionError):
        A.compare_plans([(p[0] + 1,) + p[1:] for p in plans], plans)
    # the prediction itself, on the distance-200 pair alone: 16 -> 256, four repeats, five passes, the variants (1, 4) .. (1, 8)
    plans, st, la = A.predict([(200, 200, 200)], 0.0, ops=True)
    assert plans == [(256, 400, 1, 8, 0)]  # (kcap: 457, clipped to n + m)
    assert (st["n_retries"], st["n_batches"], st["n_aligned"], st["n_unaligned"]) == (4, 5, 1, 0)
    assert st["band_cells"] == sum(200 * (2 * (k // 2) + 1) for k in (16, 32, 64, 128, 256))
    assert la == dict(nw_forward=5, nw_traceback=5 + 3)
    # 4 200 jobs beyond their first threshold: 4 096 in the early retry, the others in the pass behind it
    plans, st, la = A.predict([(40, 40, 20)] * 4200, 0.0)
    assert (st["n_retries"], st["n_batches"], st["n_aligned"]) == (4200, 3, 4200) and la == dict(nw_forward=3, nw_traceback=5)
    # under a budget of 64 MB the early retry's one chunk (a twelfth) does not hold the 60 doubled bands of 6 000 columns:
    # the others are doubled once more by the pass behind it; every job still repeats once
    plans, st, la = A.predict([(6000, 6000, 1400)] * 60, 0.164, budget=64 << 20)
    k0 = A.threshold(0.164, 6000, 6000)
    hs, ck = P.store(6000, 6000, 2 * k0, *P.plan(6000, 6000, 2 * k0, 64, 1 << 40)[:3:2])
    fit = ((64 << 20) // 12) // (hs * 4 + ck * 16)
    assert 0 < fit < 60 and sorted(p[0] for p in plans) == [2 * k0] * fit + [4 * k0] * (60 - fit)
    assert (st["n_retries"], st["n_aligned"]) == (60, 60) and st["n_batches"] >= 3
    assert st["band_cells"] == 6000 * (60 * (2 * (k0 // 2) + 1) + fit * (2 * k0 + 1) + (60 - fit) * (4 * k0 + 1))


# ---- the CPU stepper -------------------------------------------------------------------------------------------------------
def _pack(codes):
    rs = seqio.pack_reads([np.asarray(codes, dtype=np.uint8)])
    return np.concatenate([rs.packed, np.zeros(2, np.uint64)])


def _stepper_cases():
    full, ordinary = A.slot_cases()
    return [c for c in list(A.threshold_cases()) + list(full.values()) + ordinary if c.cells <= 10 ** 6]


@pytest.mark.parametrize("walk", (0, 1, 16), ids=["lane", "lane16", "group16"])
def test_small_cases_through_the_cpu_stepper(walk):
    """the lane code of the sweep and of the walk at the predicted first threshold: the distance and racon's breakpoints of
    the reference runs (windows of 50)"""
    w = 50
    for c in _stepper_cases():
        d, runs = A.reference(c)
        for rc in (0, 1):
            read = A.revcomp(c.q) if rc else c.q
            recs, dist, band, status = hip.test_nw_breakpoints(_pack(c.t), c.n, _pack(read), c.m, 0, c.n, 0, c.m, rc, w,
                                                               k=A.threshold(0.0, c.n, c.m), group_lanes=walk)
            assert status == 0 and dist == d, (c, rc)
            assert band[0] >= d
            got = []
            for r in recs:
                if r["first_t"] != 0xFFFFFFFF:
                    got += [(int(r["first_t"]), int(r["first_q"])), (int(r["last_t"]), int(r["last_q"]))]
            want = U.breakpoints_from_runs(runs, 0, 0, c.n, w)
            assert got == [tuple(int(v) for v in p) for p in want], (c, rc)
