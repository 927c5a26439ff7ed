"""tests/ed_ring_cases.py against the oracle's DP and against itself, without a GPU: every planted distance is the one the
DP finds, every case falls into the branch of the model its class names (decided by the wave ring at sweep i, left to the
full sweep, above by threshold, ...), every class has the members it promises on both strands, the model's statements
agree with each other.  Nothing is skipped or filtered: a case that is not what it claims fails here, before the device
is asked (tests/test_gpu_ed_ring_cases.py)."""
from collections import Counter

import pytest

from tests import ed_ring_cases as ec

CAP = ec.CAP


@pytest.fixture(scope="module")
def D():
    return ec.distances()


def _tr(c, D):
    n, m, d, km = ec.shape(c, D[c["seq"]])
    return ec.trace(n, m, d, km, c["route"], c["L"])


def _sel(tag, **want):
    out = [c for c in ec.by_tag(tag) if all(c[k] == v for k, v in want.items())]
    assert out, (tag, want)
    return out


def test_every_planted_distance_is_the_dps(D):
    assert set(D) == set(ec.SEQS) and len(D) >= 90
    wrong = [(k, ec.SEQS[k][2], D[k]) for k in D if ec.SEQS[k][2] != D[k]]
    assert not wrong, wrong
    # the DP is quadratic: what the file costs (every sequence pair once, whatever the number of its placements)
    assert ec.dp_cells() <= 8_000_000_000, ec.dp_cells()
    assert len(ec.cases()) <= ec.SAMPLE  # one call holds them all without leaving "the sample" of the lane stage
    assert [c["name"] for c in ec.cases()] == [c["name"] for c in ec.cases.__wrapped__()]  # deterministic


def test_the_models_statements_agree(D):
    """expected (the value, from the distance), trace (the way through the stages) and the leaves_* statements the launch
    counts come from are three restatements: they meet on every case, on every route."""
    for c in ec.cases():
        n, m, d, km = ec.shape(c, D[c["seq"]])
        for route, L in ((0, 0), (0, 64), (1, 1), (1, 64), (1, 128), (1, 512), (1, 0)):
            t = ec.trace(n, m, d, km, route, L)
            assert t.value == ec.expected(n, m, d, km, route, L), (c["name"], route, L, t)
            assert t.value in (d, ec.ABOVE) or (min(n, m) == 0 and t.value == n + m)
            L = ec.ring_lanes(route, L)
            if L:
                assert (t.decided == "full") == ec.leaves_wide(n, m, d, km, L) and t.lane is None
                assert all(abs(n - m) <= k <= ec.cap_wide(L) for k in t.ks) and len(t.ks) <= 1
            else:
                assert (t.decided != "lane") == ec.leaves_lane(n, m, d, km), (c["name"], t)
                if t.decided != "lane":
                    assert (t.decided == "full") == ec.leaves_wave(n, m, d, km), (c["name"], t)
                assert all(max(64, abs(n - m)) <= k <= CAP for k in t.ks)
                assert all(b == min(2 * a, CAP) for a, b in zip(t.ks, t.ks[1:]))
            if km < ec.UNBOUNDED and d > km and t.decided != "full":
                assert t.value == ec.ABOVE


def test_every_class_has_both_strands_and_its_members():
    count = Counter(c["tag"] for c in ec.cases())
    assert set(count) == set(ec.TAGS)
    for tag in ec.TAGS:
        assert {c["strand"] for c in ec.by_tag(tag)} == {0, 1}, tag
    for L in (64, 128, 512, 1):
        assert {c["strand"] for c in _sel("wide", L=L)} == {0, 1}, L
    assert all(c["L"] == c["route"] == 0 for c in ec.cases() if c["tag"] != "wide") and all(c["route"] == 1 for c in ec.by_tag("wide"))
    assert [ec.ring_lanes(*x) for x in ((0, 0), (0, 128), (1, 1), (1, 0), (1, -1), (1, 64), (1, 448))] == [0, 0, 0, 512, 512, 64, 448]
    assert all(c["km"] is None for c in ec.cases() if c["tag"] not in ("bounded", "wide"))
    names = [(c["tag"], c["name"], c["L"]) for c in ec.cases()]
    assert len(set(names)) == len(names)


def test_thr_edge(D):
    ks = {c["seq"]: _tr(c, D) for c in ec.by_tag("thr_edge")}
    want = {"thr400+0": (400, (400,)), "thr400+1": (401, (400, 800)), "thr400+400": (800, (400, 800)),
            "thr400+401": (801, (400, 800, 1600)), "thr400+1200": (1600, (400, 800, 1600)),
            "thr400+1201": (1601, (400, 800, 1600, 3200)), "thr_eq512": (512, (64, 128, 256, 512)),
            "thr_eq513": (513, (64, 128, 256, 512, 1024)), "thr4100+0": (4100, (4100,)), "thr4100+1": (4101, (4100, CAP)),
            "thr4100+400": (4500, (4100, CAP))}
    assert set(ks) == set(want)
    for key, (d, seq) in want.items():
        assert D[key] == d and ks[key] == ec.Trace("wave", seq, d, ks[key].lane), (key, ks[key])
        a, b, _ = ec.SEQS[key]
        assert (a.shape[0] == b.shape[0] == 1500) if key.startswith("thr_eq") else abs(a.shape[0] - b.shape[0]) == seq[0]
        assert ks[key].lane == ("overflow" if key.startswith("thr_eq") else "no_fit")
    assert {ec.SEQS[k][0].shape[0] > ec.SEQS[k][1].shape[0] for k in want if k.startswith("thr400")} == {True, False}


def test_cap_edge(D):
    seen = set()
    for c in ec.by_tag("cap_edge"):
        a, b, _ = ec.SEQS[c["seq"]]
        n, m, d = a.shape[0], b.shape[0], D[c["seq"]]
        t = _tr(c, D)
        seen.add((abs(n - m), d, n > m))
        assert min(n, m) == 236
        if abs(n - m) == CAP + 1:
            assert t == ec.Trace("full", (), CAP + 1, "no_fit")        # no threshold holds |n - m|: straight to the full sweep
        elif d == CAP + 1:
            assert t == ec.Trace("full", (CAP - 1, CAP), CAP + 1, "no_fit")
        elif abs(n - m) == CAP:
            assert t == ec.Trace("wave", (CAP,), CAP, "no_fit")
        else:
            assert t == ec.Trace("wave", (CAP - 1, CAP), CAP, "no_fit")   # the last step min(2 k, cap), D on the capacity
    assert seen == {(dl, d, r) for dl, d in ((8064, 8064), (8063, 8064), (8063, 8065), (8065, 8065)) for r in (True, False)}


def test_geometry(D):
    rows = Counter()
    for c in ec.by_tag("geometry"):
        a, b, _ = ec.SEQS[c["seq"]]
        assert D[c["seq"]] == 400 == abs(a.shape[0] - b.shape[0]) and _tr(c, D) == ec.Trace("wave", (400,), 400, "no_fit")
        rows[min(a.shape[0], b.shape[0]), a.shape[0] < b.shape[0]] += 1
    assert rows == Counter({(n, r): 1 for n in (1, 63, 64, 65, 255, 256, 257, 511, 512, 513) for r in (True, False)})
    last = ec.by_tag("geometry")[-1]
    assert last["a_last"] and last["at"] == 0 and not any(c["a_last"] for c in ec.cases() if c is not last)


def _super_blocks(n):
    return -(-(-(-n // 64)) // 4)


def test_ring_reuse(D):
    ns = []
    for c in ec.by_tag("ring_reuse"):
        a, b, _ = ec.SEQS[c["seq"]]
        n, m, d = a.shape[0], b.shape[0], D[c["seq"]]
        t = _tr(c, D)
        ns.append(n)
        assert t.decided == "wave" and t.value == d <= CAP and t.lane == "no_fit", (c["name"], t)  # a wrap WITH a result
        if n < 32769:
            assert 385 <= abs(n - m) <= 3000 and 30 <= d - abs(n - m) <= 700
    assert sorted(set(ns)) == [16384, 16385, 16448, 16640, 16641, 32769]
    assert [_super_blocks(n) for n in sorted(set(ns))] == [64, 65, 65, 65, 66, 129]  # 64: the ring is just full; 129: a second wrap
    assert {c["strand"] for c in ec.by_tag("ring_reuse") if c["seq"] == "rr16385"} == {0, 1}
    assert {ec.SEQS[c["seq"]][0].shape[0] > ec.SEQS[c["seq"]][1].shape[0] for c in ec.by_tag("ring_reuse")} == {True, False}


def test_retire(D):
    got = {}
    for c in ec.by_tag("retire"):
        a, b, _ = ec.SEQS[c["seq"]]
        got[a.shape[0], b.shape[0]] = _tr(c, D)
    assert got == {(17000, 9000): ec.Trace("wave", (8000, CAP), 8010, "no_fit"), (9000, 17000): ec.Trace("wave", (8000, CAP), 8010, "no_fit"),
                   (237, 8300): ec.Trace("wave", (8063,), 8063, "no_fit"), (8300, 237): ec.Trace("wave", (8063,), 8063, "no_fit"),
                   (236, 8300): ec.Trace("wave", (CAP,), CAP, "no_fit"), (8300, 236): ec.Trace("wave", (CAP,), CAP, "no_fit")}
    # nobody in the class needs the full sweep: its launch count is the wave ring's alone
    assert ec.launches([ec.shape(c) for c in ec.by_tag("retire")]) == dict(edit_lane=1, edit_banded=1, edit_wide=0, edit_full=0)


def test_text_side(D):
    cs = ec.by_tag("text_side")
    for c in cs:
        assert _tr(c, D).decided == "wave" and _tr(c, D).value == D[c["seq"]]
    small = [c for c in cs if c["seq"].startswith("text")]
    res = lambda c: (c["strand"], c["bb"] % 32, (c["bb"] + ec.SEQS[c["seq"]][1].shape[0]) % 32)
    assert {(s, b0, e) for s in (0, 1) for b0 in (0, 31) for e in (0, 1)} | {(0, 1, 31), (1, 1, 31)} <= {res(c) for c in small}
    for c in small:
        a, b, _ = ec.SEQS[c["seq"]]
        assert 880 <= a.shape[0] <= 940 and 480 <= b.shape[0] <= 540
    assert {c["ab"] % 32 for c in small} >= {0, 1, 31}
    assert {c["bb"] for c in small if c["strand"] == 0} >= {0, 1, 31}          # the reverse strand, begin inside the first word
    big = [c for c in cs if c["seq"] == "rr16385"]
    assert {(c["strand"], c["bb"] % 32) for c in big} >= {(s, b0) for s in (0, 1) for b0 in (0, 31)}
    assert {c["ab"] % 32 for c in big} >= {0, 1, 31} and any(c["strand"] == 0 and c["bb"] < 32 for c in big)
    assert cs[-1]["bt"] == 0 and not cs[-1]["a_last"] and cs[-1]["strand"] == 0   # ends on the last base of the set's last read
    rs, pairs, kmax = ec.place(cs)
    assert kmax is None and int(pairs[-1][3]) == rs.n - 1 and int(pairs[-1][4] + pairs[-1][5]) == int(rs.lengths[-1])
    assert int(rs.word_offsets[-1]) + 1 == rs.packed.shape[0]                  # one pad word behind it


def test_bounded(D):
    cs = ec.by_tag("bounded")
    got = {(c["seq"], c["km"]): _tr(c, D) for c in cs}
    A = ec.ABOVE
    for key, d, delta in (("thr400+400", 800, 400), ("rr16385", 3200, 3000)):
        assert D[key] == d
        assert got[key, d - 1] == ec.Trace("wave", (d - 1,), A, "no_fit")         # one sweep at the threshold, just below D
        assert got[key, d] == ec.Trace("wave", (d,), d, "no_fit")
        assert got[key, d + 1] == ec.Trace("wave", (d + 1,), d, "no_fit")
        assert got[key, delta] == ec.Trace("wave", (delta,), A, "no_fit")          # km = |n - m|: k >= km after the first sweep
        assert got[key, delta - 1] == ec.Trace("lane", (), A, "d_above")           # |n - m| > km: nobody sweeps
        assert got[key, CAP] == ec.Trace("wave", (CAP,), d, "no_fit")
    assert [got["eq40", km].value for km in (10, 39, 40, 63)] == [A, A, 40, 40]
    assert [got["eq100", km].value for km in (10, 63)] == [A, A]
    assert all(got[k, km].decided == "lane" for k, km in got if k.startswith("eq"))  # (equal lengths: the lane window holds every km < 64)
    for s, d in ((1, 8064), (2, 8065), (3, 8066)):
        key = "cap8063+%db" % s
        assert D[key] == d
        t = {km: got[key, km] for km in (CAP, CAP + 1, 20000)}
        assert t[CAP] == ec.Trace("wave", (CAP,), d if d <= CAP else A, "no_fit")
        for km in (CAP + 1, 20000):  # thresholds beyond the capacity: the doubling sequence, then the full sweep, exact even above km
            assert t[km] == (ec.Trace("wave", (CAP - 1, CAP), d, "no_fit") if d <= CAP else ec.Trace("full", (CAP - 1, CAP), d, "no_fit"))
    assert got["cap8063+3b", CAP + 1].value == 8066 > CAP + 1
    for n in (65, 257, 513):  # the path on the band's edge, with a block boundary behind the cut: one sweep at km = D = |n - m|
        for sfx in "cr":
            a, b, _ = ec.SEQS["edge%d%s" % (n, sfx)]
            assert (a.shape[0] if sfx == "c" else b.shape[0]) == n and abs(a.shape[0] - b.shape[0]) == 400
            assert got["edge%d%s" % (n, sfx), 400] == ec.Trace("wave", (400,), 400, "no_fit")
            assert got["edge%d%s" % (n, sfx), 401] == ec.Trace("wave", (401,), 400, "no_fit")


def test_wide(D):
    A = ec.ABOVE
    got = {(c["L"], c["name"].split(" ", 1)[1]): _tr(c, D) for c in ec.by_tag("wide")}
    T = ec.Trace
    # L = 64: the capacity edge 8 064 / 8 065, by D and by |n - m|; km on both sides of D and of the capacity
    for sfx in "rc":
        assert got[64, "cap8064+0" + sfx] == T("wide", (CAP,), CAP, None) and got[64, "cap8065+0" + sfx] == T("full", (), CAP + 1, None)
    assert got[64, "cap8063+2c"] == T("full", (CAP,), CAP + 1, None) and got[64, "cap8063+1r"] == T("wide", (CAP,), CAP, None)
    assert got[64, "cap8063+1c km 8063"] == T("wide", (CAP - 1,), A, None) and got[64, "cap8063+1c km 8064"] == T("wide", (CAP,), CAP, None)
    assert got[64, "cap8063+2r km 8064"] == T("wide", (CAP,), A, None)
    assert got[64, "cap8063+2r km 8065"] == got[64, "cap8063+2r km 8066"] == T("full", (CAP,), CAP + 1, None)
    assert got[64, "cap8063+3b km 8065"] == T("full", (CAP,), CAP + 2, None)       # exact above km
    # L = 128: 16 256 / 16 257
    c128 = ec.cap_wide(128)
    assert c128 == 16256 and ec.cap_wide(64) == CAP and ec.cap_wide(512) == 65408
    for sfx in "rc":
        a, b, _ = ec.SEQS["w16256" + sfx]
        assert min(a.shape[0], b.shape[0]) == 244
        assert got[128, "w16256" + sfx] == T("wide", (c128,), c128, None) and got[128, "w16257" + sfx] == T("full", (), c128 + 1, None)
        assert got[128, "w16255+1" + sfx] == T("wide", (c128,), c128, None) and got[128, "w16255+2" + sfx] == T("full", (c128,), c128 + 1, None)
    assert got[128, "w16255+1r km 16255"] == T("wide", (c128 - 1,), A, None) and got[128, "w16255+1r km 16256"] == T("wide", (c128,), c128, None)
    assert got[128, "w16255+1c km 16257"] == T("wide", (c128,), c128, None) and got[128, "w16255+2r km 16256"] == T("wide", (c128,), A, None)
    assert got[128, "w16255+2c km 16257"] == got[128, "w16255+2r km 16258"] == T("full", (c128,), c128 + 1, None)
    for sfx in "rc":  # the path on the band's edge in the workgroup ring
        assert got[128, "w16256%s km 16256" % sfx] == T("wide", (c128,), c128, None) and got[64, "edge257%s km 400" % sfx] == T("wide", (400,), 400, None)
    assert got[128, "w16255+3r km 16257"] == got[128, "w16255+3c km 16257"] == T("full", (c128,), c128 + 2, None)
    # ring re-use (n > 256 L) and work in a second wave (L = 128, super-blocks 64 and up)
    for L, keys in ((64, ("rr16385", "rr16641")), (128, ("rr32769",))):
        for key in keys:
            cs = [c for c in _sel("wide", L=L) if c["seq"] == key and c["km"] is None]
            assert _super_blocks(ec.SEQS[key][0].shape[0]) > L and all(_tr(c, D).decided == "wide" and _tr(c, D).value == D[key] for c in cs)
    second_wave = [c for c in _sel("wide", L=128) if c["seq"] in ("rr16385", "rr16641")]
    assert all(64 < _super_blocks(ec.SEQS[c["seq"]][0].shape[0]) <= 128 and 16385 <= ec.SEQS[c["seq"]][0].shape[0] <= 16700 for c in second_wave)
    assert {(c["seq"], c["strand"]) for c in second_wave} >= {(k, s) for k in ("rr16385", "rr16641") for s in (0, 1)}
    for L in (64, 128, 512):
        cs = _sel("wide", L=L)
        assert got[L, "rr16385 km 3199"] == T("wide", (3199,), A, None) and got[L, "rr16385 km 3200"] == T("wide", (3200,), 3200, None)
        text = [c for c in cs if c["seq"].startswith("text")]
        assert {c["strand"] for c in text} == {0, 1} and {c["bb"] % 32 for c in text} & {1, 31}
        whole = [c for c in cs if c["ratio"] is not None]
        assert whole and all(c["strand"] == 1 and c["ab"] == c["bb"] == c["at"] == c["bt"] == 0 and c["km"] > CAP for c in whole)
        for c in whole:  # the length rule of the similarity test lets them through
            n, m, _, km = ec.shape(c)
            assert not (min(n, m) < max(n, m) * c["ratio"]) and km == ec.kmax_rule(max(n, m), c["ratio"])
    # L = 1: the ring switched off; the members of L = 64 again, and the usual route leaves the same values (equal capacities)
    one, ring = _sel("wide", L=1), [c for c in _sel("wide", L=64) if c["ratio"] is None]
    assert [(c["seq"], c["km"], c["name"].split(" ", 1)[1]) for c in one] == [(c["seq"], c["km"], c["name"].split(" ", 1)[1]) for c in ring]
    assert [_tr(c, D).value for c in one] == [_tr(c, D).value for c in ring]
    assert {_tr(c, D).decided for c in one} == {"wave", "full"}


def test_full(D):
    cs = ec.by_tag("full")
    stripes = Counter()
    for c in cs:
        a, b, _ = ec.SEQS[c["seq"]]
        n, m = a.shape[0], b.shape[0]
        t = _tr(c, D)
        assert t.decided == "full" and t.value == D[c["seq"]] > CAP and c["km"] is None
        stripes[-(-(-(-n // 64)) // 64)] += 1
        if c["seq"] == "full8200":
            assert n == m == 8200 and t.ks == (64, 128, 256, 512, 1024, 2048, 4096, CAP) and t.lane == "overflow"
        else:
            assert t.ks == () and abs(n - m) > CAP
    shapes = {ec.SEQS[c["seq"]][0].shape[0]: ec.SEQS[c["seq"]][1].shape[0] for c in cs}
    assert all(n + 8065 <= shapes[n] <= n + 8100 for n in (1, 10, 64, 4096)) and {4097, 8192} <= set(shapes)
    assert {(n, m) for n in (8193, 8300) for m in (1, 2, 33, 100)} <= {(ec.SEQS[c["seq"]][0].shape[0], ec.SEQS[c["seq"]][1].shape[0]) for c in cs}
    assert stripes[1] >= 4 and stripes[2] >= 2 and stripes[3] >= 8
    ms = [ec.SEQS[c["seq"]][1].shape[0] for c in cs]
    assert ms != sorted(ms) and ms != sorted(ms, reverse=True) and len(set(ms)) >= 8   # hb_off: different m, in no order


def test_batch(D):
    pool = ec.by_tag("batch")
    calls = ec.batch_calls()
    assert sorted(calls) == [1, 3, 4, 5]
    for share, idx in calls.items():
        ts = [_tr(pool[i], D) for i in idx]
        assert sum(t.decided == "wave" for t in ts) == share and all(t.decided in ("wave", "lane") for t in ts)
        assert sum(t.decided == "lane" for t in ts) >= 10 and len(set(idx)) == len(idx)
        where = [j for j, t in enumerate(ts) if t.decided == "wave"]
        assert share == 1 or where != list(range(where[0], where[0] + share))  # scattered among the others
        assert ec.launches([ec.shape(pool[i]) for i in idx]) == dict(edit_lane=1, edit_banded=1, edit_wide=0, edit_full=0)
    assert {_tr(c, D).lane for c in pool} >= {"exact", "empty", "no_fit"}
    # every case of every class in one call
    everything = ec.launches([ec.shape(c) for c in ec.cases()])
    assert everything == dict(edit_lane=1, edit_banded=1, edit_wide=0, edit_full=1)
