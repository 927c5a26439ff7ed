"""Crafted windows for window consensus (raven_amd/csrc/poa4.hip, poa2_window.h / poa2.hip, poa.hip), each placed on a
stated side of one of the kernels' hand-on limits and tagged with the outcome every kernel must report there.

cases() returns a list of dicts:
  name, family   family is one of FAMILIES
  limit, side    the limit the case addresses (a key of the table below) and where it stands: "inside", "at", "beyond"
  window         {layers, begins, ends, quals} as Engine.poa_consensus_batch / hip.poa_banded_emulate take it
  trim           the coverage trim the case is run with
  claims         what the window is BY CONSTRUCTION, as {statistic: (op, value)} over oracle.poa_window_stats (a per-layer
                 statistic is taken as its maximum over the layers, band_step_min as its minimum): tests/test_poa_cases.py
                 asserts every one of them, so a generator is held to what it is named after
  poa4           (status byte, reason) of the 32-column first attempt (the emulator, mode 9)
  final          status of the whole chain (mode 0): 1 = the oracle's consensus, 0 / 2 / 3 / 4 = the backbone
  alone          True: the case stands for a limit that depends on the batch (nmax = clamp(6 x the batch's longest
                 backbone, 512, 8192)) and is run in a batch of its own
  also           a second (limit, side) the case stands for
  walks          (in-edge, vertical) pairs: some layer's own path enters the row of the largest in-degree through that
                 in-edge, with a base (0) or without one (1) — asserted like the claims
  band           for the `band` family: (width the path is clearly outside of | 0, ...)
Sizes at a boundary are found from the oracle's statistics (a generator grows its window until the statistic is the
one wanted); nothing here runs a kernel, and nothing looks at what a kernel returns.

The limits, restated (a change of one of them in the kernels must be followed here: tests/test_poa4_limits.py
holds the poa4 ones to raven_amd/csrc/poa4_limits.h):"""
import functools
import operator

import numpy as np

from oracle import oracle

# (poa4_limits.h: struct P4; `edge`: the lambda of poa4_phase_desc_onewave, poa4_desc.h, that looks at one in-edge)
P4_RING = 22         # poa4_limits.h P4::kRing: an in-edge of at most kRing - 1 ranks (`edge`)
P4_RING_OVF = 20     # `edge`: in-edges 7..14 of a row of >= 9 (and its in-edge 7, lbk7) at most kRing - 2 ranks
P4_MAX_D = 8         # poa4_limits.h P4::kMaxD: band-start difference along an in-edge (`edge`)
P4_EDGES = 8         # poa4_limits.h P4::kEdges: in-edges in a row descriptor (the eighth is the `v7` bit)
P4_EDGES_MAX = 15    # poa4_limits.h P4::kEdgesMax: a row of 16 hands the window on with reason 3 (poa4_phase_desc_onewave)
P2_RING = 32         # poa2_window.h:14 kRing: a predecessor more than 32 computed rows back is status 7 (poa2_window.h:337)
MAX_IN = 16          # poa.h:15      kPoaMaxIn: a seventeenth in-edge is status 3
NMAX_FLOOR, NMAX_PER_BASE = 512, 6  # poa.hip:656 nmax = clamp(6 x backbone, 512, 8192): one node more is status 2
P2_MAX_SEQ = 896     # poa.h:18      kPoa2MaxSeq: a longer layer is the full-matrix kernel's
MAX_SEQ = 1024       # poa.h:16      kPoaMaxSeq: a longer layer is status 4
BANDS = (32, 64, 128, 256)  # poa4_limits.h P4::kBand, poa2.hip's 64 x NCH columns
R_EDGE, R_INDEG, R_WALK = 7, 3, 10  # reasons (status bits 24-27) of poa4.hip poa4_phase_dp and poa4_phase_tb

# Limits of the issue's table that have NO case, because another check always fires first (DESIGN.md 3.6 repeats this):
#  * `lbk > rho` (`edge`, the tail of an in-edge below the layer's rank range): an in-edge is looked at only if its
#    tail is marked (its `inside`), and r_lo is the smallest rank of a marked node (poa4_desc.h poa4_subgraph_marks), so
#    rank(tail) >= r_lo and lbk = r - rank(tail) <= r - r_lo = rho for every edge that reaches the comparison.  The
#    `below_range` family pins what CAN happen: in-edges cut by the subgraph with the tail one rank inside / below.
#  * the step budget, reason 1 (poa4.hip poa4_phase_dp): t_end = max(Srow) + 17 with Srow = rho + rho / 16 + sdiff / 2 + 1
#    (poa4_phase_desc_onewave), rho < nmax and sdiff <= lmax, so t_end + 8 <= nmax + nmax / 16 + lmax / 2 + 26 < poa4_steps().
#  * reason 9 (poa4.hip poa4_phase_dp, the last column in no end node's band): backbone node `end` is an end node of every
#    (sub)graph, its guide position is `span`, where the guide is the layer's length, and poa4_band_start clamps the band
#    to hold the last column — the straight guide rvn_poa_consensus_batch fills in cannot miss it.
#  * reason 11 (poa4.hip poa4_phase_tb, a backpointer the walk cannot follow) is a consistency check, not a limit: no
#    legal input is known to reach it.
#  * status 3 out of the first attempt itself (poa4_graph.h poa4_update_graph): the layer that would add a seventeenth
#    in-edge is aligned to a row of sixteen first, which is reason 3; the 64-column kernel reports the status 3.
#  * P4::kMaxD 8 against 9: band starts are even (poa4_band_start), so a difference is 8 or 10: `band_step` pins those.
FAMILIES = ("in_edge_ranks", "band_step", "in_degree", "below_range", "nodes", "length", "band", "ties", "groups")


def _truth(seed, n):
    return np.random.default_rng(seed).integers(0, 4, size=n, dtype=np.uint8)


def _ins(t, p, s):
    return np.concatenate([t[:p], np.asarray(s, dtype=np.uint8), t[p:]])


def _cut(t, p, d):
    """t without the d bases in front of position p."""
    return np.concatenate([t[:p - d], t[p:]])


def stats(w):
    return oracle.poa_window_stats(w["layers"], w.get("begins"), w.get("ends"), w.get("quals"))


def stat(st, key):
    v = st[key]
    if np.ndim(v) == 0:
        return int(v)
    return int(v.min() if key == "band_step_min" else v.max())


_OPS = {"==": operator.eq, "<=": operator.le, ">=": operator.ge}


def claims_hold(case, st=None):
    """The claims of a case that the oracle's statistics do NOT bear out, as (statistic, op, wanted, found); `walks` (the
    (in-edge, vertical) pairs some layer's own path must take into the row of the largest in-degree) as ("walks", ..)."""
    st = st or stats(case["window"])
    bad = [(k, op, v, stat(st, k)) for k, (op, v) in case["claims"].items() if not _OPS[op](stat(st, k), v)]
    walked = set(zip(st["walk_index"].tolist(), st["walk_vertical"].tolist()))
    missing = sorted(set(case.get("walks", ())) - walked)
    return bad + ([("walks", "has", missing, sorted(walked))] if missing else [])


def _case(name, family, limit, side, window, poa4, final, claims, trim=True, alone=False, band=None):
    claims = dict(claims)
    claims.setdefault("agree", ("==", 1))
    return dict(name=family + ":" + name, family=family, limit=limit, side=side, window=window, poa4=poa4, final=final,
                claims=claims, trim=trim, alone=alone, band=band)


def _grow(make, key, target, sizes):
    """The first size whose window has statistic `key` == target: (size, window)."""
    for s in sizes:
        w = make(s)
        if stat(stats(w), key) == target:
            return s, w
    raise AssertionError("no size in %r gives %s == %d" % (sizes, key, target))


# ---- in_edge_ranks -----------------------------------------------------------------------------------------------------
def _twin(truth, near):
    """The first position >= near whose base equals the one in front of it: a run of any OTHER letter in front of it can be
    placed in one way only (a run of a neighbour's letter could equally stand on the neighbour's other side)."""
    return next(i for i in range(near, len(truth)) if truth[i] == truth[i - 1])


def _runs_of(truth, p, total):
    """Run lengths that add up to `total` and differ by at most one, for the letters that are neither position p's nor
    position p - 1's."""
    letters = [c for c in range(4) if c not in (truth[p - 1], truth[p])]
    k = len(letters)
    return [(c, total // k + (1 if i < total % k else 0)) for i, c in enumerate(letters)]


def _fan_in_truth(seed, n, p):
    """Random bases, but position p's letter (T) and position p - 1's (G) occur nowhere in the nine bases before them (A, C): a
    deletion of 1..8 bases in front of p, a run of A or C in front of p and a replaced base among them can each be aligned
    in one way only (inside random bases a deletion moves by a base, or splits, and enters another row)."""
    truth = _truth(seed, n)
    truth[p - 10:p - 1] &= 1
    truth[p - 1], truth[p] = 2, 3
    return truth


def _skip_edge_window(truth, p, total, tail_layers=3):
    """Three layers, each with a private run of its own letter in front of backbone position p: runs of different letters do
    not merge (a mismatch costs more than a gap), so the edge p - 1 -> p spans all of them while no layer drifts by more than
    its own run."""
    layers = [truth.copy()]
    for c, j in _runs_of(truth, p, total):
        if j:
            layers.append(_ins(truth, p, [c] * j))
    layers += [truth.copy() for _ in range(tail_layers)]
    return dict(layers=layers)


def _in_edge_cases():
    out = []
    truth = _truth(101, 200)
    p = _twin(truth, 100)
    for target in (P4_RING - 2, P4_RING - 1, P4_RING, P2_RING - 1, P2_RING, P2_RING + 1):
        total, w = _grow(lambda s: _skip_edge_window(truth, p, s), "in_edge_ranks", target, range(8, 40))
        p4 = target <= P4_RING - 1
        side = "beyond" if target in (P4_RING, P2_RING + 1) else ("at" if target in (P4_RING - 1, P2_RING) else "inside")
        out.append(_case("plain_%d" % target, "in_edge_ranks", "P4::kRing" if target <= P4_RING else "poa2 kRing", side, w,
                         (1, 0) if p4 else (8, R_EDGE), 1,
                         {"in_edge_ranks": ("==", target), "final_nodes": ("==", 200 + total), "in_degree": ("<=", 4),
                          "off_centre": ("<=", 5 if p4 else 8), "band_step": ("<=", 2)}))
        out[-1]["found"] = "runs of %s in front of position %d" % ([j for _, j in _runs_of(truth, p, total)], p)
    return out + _fan_in_cases()


FAN_IN_SEED = 312  # found once by trying 303, 304, ..: the first whose ten windows are what they are named after


def _fan_in_cases(p=100):
    """A row of ten in-edges (p - 1, two runs, deletions, replaced bases in front of a deletion); the longest in-edge is the
    deletion of seven bases (tail p - 8): 8 + the runs' nodes in ranks, and it is the in-edge its layer's place in the window
    makes it.  Which bases stand in front of p decides whether every deletion enters row p (see _fan_in_truth), so the seed
    is a recorded one; tests/test_poa_cases.py asserts every claim (the in-degree, the long edge's place) from the oracle."""
    truth = _fan_in_truth(FAN_IN_SEED, 200, p)
    out = []
    for where, idx in (("low", 3), ("seventh", 7), ("overflow", 9)):
        for target in ((19, 20, 21, 22) if where == "low" else (19, 20, 21)):
            def make(s, idx=idx):
                others = [_ins(truth, p, [c] * j) for c, j in _runs_of(truth, p, s)]
                others += [_cut(truth, p, d) for d in range(1, 7)]
                others += [np.concatenate([truth[:p - 1 - d], [c], truth[p:]]).astype(np.uint8) for d in range(0, 6)
                           for c in range(4) if c != truth[p - 1 - d]]
                layers, deg = [truth.copy()], 1
                for cand in others:  # (a variant is kept if it gives the row one more in-edge: the oracle's count)
                    if deg == idx:
                        layers.append(_cut(truth, p, 7))
                        deg += 1
                    if deg == 10:
                        break
                    if oracle.poa_window_stats(layers + [cand])["final_in_degree"] == deg + 1:
                        layers.append(cand)
                        deg += 1
                return dict(layers=layers + [truth.copy(), _cut(truth, p, 7), truth.copy()])
            total, w = _grow(make, "in_edge_ranks", target, range(6, 24))
            limit = P4_RING - 1 if where == "low" else P4_RING_OVF
            ok = target <= limit
            out.append(_case("fan_in_%s_%d" % (where, target), "in_edge_ranks",
                             "P4::kRing" if where == "low" else ("lbk7" if where == "seventh" else "kRing - 2"),
                             "beyond" if not ok else ("at" if target == limit else "inside"), w,
                             (1, 0) if ok else (8, R_EDGE), 1,
                             {"in_edge_ranks": ("==", target), "long_index": ("==", idx), "long_degree": ("==", 10),
                              "in_degree": ("==", 10), "band_step": ("<=", P4_MAX_D), "off_centre": ("<=", 8)}))
            out[-1]["walks"] = [(idx, 0)]  # (the layer with the long deletion once more: its path takes that in-edge)
            out[-1]["found"] = "runs of %s in front of position %d" % ([j for _, j in _runs_of(truth, p, total)], p)
    return out


# ---- band_step ---------------------------------------------------------------------------------------------------------
def _clean_deletion(seed, n, p, d):
    """(truth, truth without the d bases in front of p) such that the deletion can be aligned in one way only: the d bases
    are G / T, the four bases on either side of them A and C — nothing of the shorter layer matches inside the gap, so the
    alignment cannot split it or move it (a deletion inside random bases does both, and its band step with it)."""
    truth = _truth(seed, n)
    truth[p - d - 4:p - d] = 0
    truth[p - d:p] = 2 + (truth[p - d:p] & 1)
    truth[p:p + 4] = 1
    return truth, _cut(truth, p, d)


def _band_step_cases():
    out = []
    for parity, p in (("even", 100), ("odd", 101)):
        def make(d, p=p):
            truth, cut = _clean_deletion(202, 200, p, d)
            return dict(layers=[truth.copy()] + [cut.copy() if k % 2 == 0 else truth.copy() for k in range(8)])
        # the largest deletion whose band step is still kMaxD, and the smallest whose step is beyond it
        d_in = max(d for d in range(4, 16) if stat(stats(make(d)), "band_step") == P4_MAX_D)
        d_out, _ = _grow(make, "band_step", P4_MAX_D + 2, range(4, 16))
        for side, d, step in (("at", d_in, P4_MAX_D), ("beyond", d_out, P4_MAX_D + 2)):
            out.append(_case("%s_start_deletion_%s" % (parity, side), "band_step", "P4::kMaxD", side, make(d),
                             (1, 0) if side == "at" else (8, R_EDGE), 1,
                             {"band_step": ("==", step), "band_step_min": (">=", 0), "in_edge_ranks": ("==", d + 1),
                              "off_centre": ("<=", 8)}))
            out[-1]["found"] = "deletion of %d bases in front of position %d" % (d, p)
    return out


# ---- in_degree ---------------------------------------------------------------------------------------------------------
def _in_degree_window(truth, p, n):
    """One row (backbone position p) with n in-edges: variants are taken from a pool, in order, as long as each adds exactly
    one in-edge to the final graph's largest in-degree (the oracle's count); then layers that walk in-edges 0, 6, 7, 8 and 14
    of that row again, diagonally (the variant once more) and vertically (the variant without base p)."""
    pool = [_cut(truth, p, d) for d in range(1, 8)]
    pool += [_ins(truth, p, [c]) for c in (0, 1)]
    pool += [np.concatenate([truth[:p - 1 - d], [c], truth[p:]]).astype(np.uint8) for d in range(0, 7) for c in range(4)
             if c != truth[p - 1 - d]]
    pool += [_ins(truth, p, [c] * j) for j in (2, 3) for c in (0, 1)]
    pool += [_ins(truth, p, [a, b]) for a in range(4) for b in range(4) if a != b]
    layers, var = [truth.copy()], [truth]
    pending = list(pool)
    while len(var) < n:
        k = len(var)  # the place the next variant's tail takes among row p's in-edges
        for i, v in enumerate(pending):
            if oracle.poa_window_stats(layers + [v])["final_in_degree"] != k + 1:
                continue
            if k in WALKED and n <= MAX_IN:  # (a tail the walk layers can also leave row p vertically from: an inserted base
                st = oracle.poa_window_stats(layers + [v, _without_p(truth, v, p)])  # in front of p is taken for p instead)
                if (st["walk_index"][-1], st["walk_vertical"][-1]) != (k, 1):
                    continue
            layers.append(pending.pop(i))
            var.append(v)
            break
        else:
            raise ValueError("the pool gives row %d no in-edge %d" % (p, k))
    if n <= MAX_IN:
        for k in WALKED:
            if k < n:
                layers.append(var[k].copy())
                # the same tail, base p left out: the walk leaves row p vertically through in-edge k
                layers.append(_without_p(truth, var[k], p))
    layers.append(truth.copy())
    return dict(layers=layers)


WALKED = (0, 6, 7, 8, 14)  # in-edges of the row that later layers walk again


def _without_p(truth, variant, p):
    """`variant` (truth changed in front of position p only) without the base of position p."""
    tail = len(truth) - p  # bases from p on are the variant's last `tail` bases
    return np.concatenate([variant[:len(variant) - tail], variant[len(variant) - tail + 1:]])


def _in_degree_cases():
    out = []
    truth, p = _fan_in_truth(303, 200, 100), 100
    for n in (4, 5, P4_EDGES, P4_EDGES + 1, P4_EDGES_MAX, MAX_IN, MAX_IN + 1):
        w = _in_degree_window(truth, p, n)
        if n <= P4_EDGES_MAX:
            poa4, final = (1, 0), 1
            limit, side = ("P4::kEdges", "inside" if n < P4_EDGES else ("at" if n == P4_EDGES else "beyond")) if n <= P4_EDGES + 1 \
                else ("P4::kEdgesMax", "at")
        elif n == MAX_IN:
            poa4, final, limit, side = (8, R_INDEG), 1, "P4::kEdgesMax", "beyond"
        else:
            poa4, final, limit, side = (8, R_INDEG), 3, "kPoaMaxIn", "beyond"
        claims = {"band_step": ("<=", P4_MAX_D), "in_edge_ranks": ("<=", P4_RING_OVF), "off_centre": ("<=", 8)}
        if n <= MAX_IN:
            claims["in_degree"] = ("==", n)
            claims["final_in_degree"] = ("==", n)
        else:
            claims["final_in_degree"] = ("==", n)
        out.append(_case("row_of_%d" % n, "in_degree", limit, side, w, poa4, final, claims))
        if n <= MAX_IN:
            out[-1]["walks"] = [(k, v) for k in WALKED if k < n for v in (0, 1)]
        if n == MAX_IN:
            out[-1]["also"] = ("kPoaMaxIn", "at")
    return out


# ---- below_range -------------------------------------------------------------------------------------------------------
def _below_range_cases():
    out = []
    p, d = 100, 5
    truth, skip = _clean_deletion(404, 200, p, d)  # edge p - d - 1 -> p

    def win(begin, end, piece):
        return dict(layers=[truth.copy(), skip.copy(), skip.copy(), truth.copy(), piece, piece.copy()],
                    begins=[0, 0, 0, 0, begin, begin], ends=[199, 199, 199, 199, end, end])
    # every partial layer cuts the backbone edge begin - 1 -> begin; with begin = p - d the skip edge's tail p - d - 1 is
    # the rank just below the range (two cut tails), with begin = p - d - 1 it is the range's first rank (one)
    for name, side, begin, below in (("tail_inside", "inside", p - d - 1, 1), ("tail_below", "beyond", p - d, 2)):
        out.append(_case(name, "below_range", "lbk > rho", side, win(begin, 160, truth[begin:161].copy()), (1, 0), 1,
                         {"tails_below": ("==", below), "in_edge_ranks": ("==", d + 1)}))
    full = win(0, 199, truth.copy())
    out.append(_case("begin_0_end_last", "below_range", "lbk > rho", "inside", full, (1, 0), 1, {"tails_below": ("==", 0)}))
    out.append(_case("end_minus_begin_1", "below_range", "lbk > rho", "inside", win(p - 1, p, truth[p - 1:p + 1].copy()), (1, 0), 1,
                     {"tails_below": ("==", 2), "rows": ("<=", 200)}))
    out.append(_case("two_bases_over_the_skip", "below_range", "lbk > rho", "inside",
                     win(p - d - 1, p, truth[[p - d - 1, p]].copy()), (1, 0), 1, {"tails_below": ("==", 1)}))
    return out


# ---- nodes -------------------------------------------------------------------------------------------------------------
def _nodes_window(truth, target, run=11):
    """A graph of exactly `target` nodes without any drift: after two whole layers, partial layers that each span two
    backbone positions (begin = i, end = i + 1, every second i: spoa's Subgraph keeps every ancestor of `end` with an id >=
    begin, the run behind position i - 1 included, and a layer would merge into it) and carry `run` private bases between them.  Such a layer is shorter than
    the narrowest band, so every row holds all of it; each adds its run's nodes (the last one as many as are still missing:
    the oracle's node count is followed layer by layer), and its in-edge i -> i + 1 spans run + 1 ranks.  (Layers of
    unrelated bases would reach the count as well, but they leave every band first: the 32-column kernel would hand the
    window on long before its own node check is asked.)"""
    n = len(truth)
    rng = np.random.default_rng(n)
    layers, begins, ends = [truth.copy(), truth.copy(), truth.copy()], [0, 0, 0], [n - 1] * 3
    nodes = n
    for i in range(1, n - 2, 2):
        if nodes == target:
            break
        free = [x for x in range(4) if x != truth[i] and x != truth[i + 1]]
        piece = rng.choice(free, size=min(run, target - nodes))
        layers.append(np.concatenate([[truth[i]], piece, [truth[i + 1]]]).astype(np.uint8))
        begins.append(i)
        ends.append(i + 1)
        nodes = oracle.poa_window_stats(layers, begins, ends)["final_nodes"]
    assert nodes == target, (nodes, target)
    return dict(layers=layers, begins=begins, ends=ends)


def _nodes_cases():
    out = []
    for blen in (85, 100):
        nmax = max(NMAX_FLOOR, NMAX_PER_BASE * blen)
        truth = _truth(505 + blen, blen)
        for side, target in (("inside", nmax - 1), ("at", nmax), ("beyond", nmax + 1)):
            w = _nodes_window(truth, target)
            ok = target <= nmax
            out.append(_case("backbone_%d_nodes_%d" % (blen, target), "nodes", "nmax", side, w, (1, 0) if ok else (2, 0),
                             1 if ok else 2, {"final_nodes": ("==", target), "off_centre": ("<=", 12), "in_degree": ("<=", 2),
                                              "in_edge_ranks": ("<=", 12), "band_step": ("<=", P4_MAX_D)}, alone=True))
    return out


# ---- length ------------------------------------------------------------------------------------------------------------
def _length_cases():
    out = []
    for n in (P2_MAX_SEQ - 1, P2_MAX_SEQ, P2_MAX_SEQ + 1, MAX_SEQ - 1, MAX_SEQ, MAX_SEQ + 1):
        truth = _truth(606 + n, n)
        other = truth.copy()
        other[n // 2] = (other[n // 2] + 1) & 3
        w = dict(layers=[other, truth.copy(), truth.copy()])
        poa4 = (1, 0) if n <= P2_MAX_SEQ else (4, 0)
        final = 1 if n <= MAX_SEQ else 4
        side = "beyond" if n in (P2_MAX_SEQ + 1, MAX_SEQ + 1) else ("at" if n in (P2_MAX_SEQ, MAX_SEQ) else "inside")
        out.append(_case("three_layers_of_%d" % n, "length", "kPoa2MaxSeq" if n <= P2_MAX_SEQ + 1 else "kPoaMaxSeq", side, w,
                         poa4, final, {"final_nodes": ("==", n + 1)}, alone=True))
    one = _truth(607, 1)
    out.append(_case("backbone_of_1", "length", "kPoaMaxSeq", "inside", dict(layers=[one]), (0, 0), 0, {"final_nodes": ("==", 1)}))
    t = _truth(608, 150)
    out.append(_case("two_layers", "length", "kPoaMaxSeq", "inside", dict(layers=[t, t.copy()]), (0, 0), 0,
                     {"final_nodes": ("==", 150)}))
    return out


# ---- band --------------------------------------------------------------------------------------------------------------
def _band_cases():
    out = []
    truth, p = _truth(707, 200), 100
    w = dict(layers=[truth.copy()] + [_cut(truth, 100, 6) if k % 2 == 0 else truth.copy() for k in range(6)])
    out.append(_case("inside_every_width", "band", "band", "inside", w, (1, 0), 1,
                     {"off_centre": ("<=", 4), "band_step": ("<=", P4_MAX_D)}, band=0))
    for width in BANDS:
        # a layer with `size` unrelated bases in front of the middle backbone position lags the straight guide by about half
        # of them before the insertion and leads it by as much behind it; the first such layer is the first one aligned, so
        # nothing shadows the band.  In the middle, because a band is clamped to the layer's ends: near an end it reaches
        # further to one side than half its width, and a path far from the guide is still inside it.
        want = width // 2 + 8

        def make(size, width=width):
            grown = _ins(truth, p, _truth(708 + width, size))
            return dict(layers=[truth.copy(), grown, grown.copy(), grown.copy(), truth.copy(), truth.copy()])
        size = next(s for s in range(want, 4 * want) if stat(stats(make(s)), "off_centre") >= want)
        centre = p * (len(truth) + size) // len(truth)  # the guide at the insertion: its band is not clamped there
        assert centre - width // 2 >= 16 and centre + width // 2 + 16 <= len(truth) + size, (width, size)
        out.append(_case("outside_%d" % width, "band", "band", "beyond", make(size), (8, R_WALK), 1,
                         {"off_centre": (">=", want)}, band=width))
        out[-1]["found"] = "%d bases in front of position %d" % (size, p)
    return out


# ---- ties --------------------------------------------------------------------------------------------------------------
def _ties_cases():
    out = []
    truth = _truth(808, 160)
    for name, pos in (("first", 0), ("middle", 80), ("last", 159)):
        other = truth.copy()
        other[pos] = (other[pos] + 1) & 3
        w = dict(layers=[truth.copy(), other, truth.copy(), other.copy()])
        out.append(_case("equal_branches_%s" % name, "ties", "consensus", "at", w, (1, 0), 1, {"final_nodes": ("==", 161)}))
    # the shape of window 7327: a node with two in-edges of equal weight, the later one from the tail with the higher score
    grown = _ins(truth, 80, [(truth[80] + 1) & 3])
    w = dict(layers=[truth.copy(), truth.copy(), truth.copy(), grown, grown.copy(), grown.copy()])
    out.append(_case("equal_in_edges_later_tail_scores_higher", "ties", "consensus", "at", w, (1, 0), 1,
                     {"final_nodes": ("==", 161)}))
    # the end node of an alignment among equal scores: two layers end in another letter, one lacks the last base, one has a base
    # more in front of the last four — the last layer's best score stands in two end nodes of different columns, and the
    # consensus depends on which one is taken (smallest node id: spoa's bytes; largest: another last base)
    t2 = truth.copy()
    t2[-6:] = [0, 2, 3, 2, 2, 0]
    lays = [t2.copy()] + [np.concatenate([t2[:-4], np.asarray(x, np.uint8)]) for x in
                          ([0, 3, 2, 2, 0], [3, 2, 2, 2], [3, 2, 2, 2], [3, 2, 2])]
    out.append(_case("end_node_among_equal_scores", "ties", "end rule", "at", dict(layers=lays), (1, 0), 1, {}))
    out[-1]["end_rule"] = True
    # weights: a backbone of weight 0, layers of weight 0 ('!') that disagree with layers of weight 60
    other = truth.copy()
    other[[40, 41, 120]] = (other[[40, 41, 120]] + 2) & 3
    lays = [other.copy(), other.copy(), other.copy(), other.copy(), truth.copy(), truth.copy()]
    quals = [np.full(len(x), 33 + (60 if i >= 4 else 0), np.uint8) for i, x in enumerate(lays)]
    out.append(_case("weights_0_and_60", "ties", "consensus", "inside", dict(layers=lays, quals=quals), (1, 0), 1,
                     {"final_nodes": ("==", 163)}))
    # coverage trim: eight layers, average coverage (9 - 1) / 2 = 4; the ends are covered by the backbone and k whole layers
    for k, side in ((3, "at"), (2, "beyond")):
        lays = [truth.copy()] + [truth.copy() for _ in range(k)] + [truth[30:120].copy() for _ in range(8 - k)]
        b = [0] * (k + 1) + [30] * (8 - k)
        e = [159] * (k + 1) + [119] * (8 - k)
        for trim in (True, False):
            out.append(_case("ends_covered_by_%d_trim_%s" % (k + 1, "on" if trim else "off"), "ties", "trim", side,
                             dict(layers=lays, begins=b, ends=e), (1, 0), 1, {"final_nodes": ("==", 160)}, trim=trim))
            out[-1]["length"] = 160 if (k == 3 or not trim) else 90
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for f in (_in_edge_cases, _band_step_cases, _in_degree_cases, _below_range_cases, _nodes_cases, _length_cases,
              _band_cases, _ties_cases):
        out += f()
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def expected(case):
    """The bytes a kernel chain must return for the case (mode 0): the oracle's consensus, or the backbone."""
    w = case["window"]
    if case["final"] == 1:
        return oracle.poa_window(w["layers"], begins=w.get("begins"), ends=w.get("ends"), quals=w.get("quals"),
                                 trim=case["trim"])[0]
    return np.asarray(w["layers"][0], dtype=np.uint8)


# ---- groups ------------------------------------------------------------------------------------------------------------
ORDINARY = ("in_edge_ranks:plain_20", "band_step:even_start_deletion_at", "in_degree:row_of_9", "ties:equal_branches_middle",
            "below_range:tail_below", "in_degree:row_of_5", "band:inside_every_width", "in_edge_ranks:fan_in_overflow_20")


def groups():
    """The `groups` family: (name, [case names]) batches of 1, 3, 4, 5 and 9 windows of the cases above — a wave of the
    rows-on-lanes kernel carries four windows — with a `beyond` case at each of the four places of a group next to
    ordinary windows, and an unpolishable window (status 2 / 3 / 4) next to polishable ones.  All trim-on cases; the node
    limit depends on the batch's longest backbone, so its group is of one backbone length."""
    out = [("batch_of_%d" % n, list(ORDINARY[:n]) if n <= 8 else list(ORDINARY) + [ORDINARY[0]]) for n in (1, 3, 4, 5, 9)]
    for place in range(4):
        g = list(ORDINARY[:3])
        g.insert(place, "in_edge_ranks:plain_22")
        out.append(("beyond_at_place_%d" % place, g + [ORDINARY[3]]))
    out.append(("status_2_among_polishable", ["nodes:backbone_85_nodes_511", "nodes:backbone_85_nodes_513",
                                              "nodes:backbone_85_nodes_512"]))  # (all of one backbone length: one nmax)
    out.append(("status_4_among_polishable", ["ties:equal_branches_first", "length:three_layers_of_1025", "in_degree:row_of_8",
                                              "in_edge_ranks:plain_21", "band_step:odd_start_deletion_at"]))
    out.append(("status_3_among_polishable", ["in_degree:row_of_5", "in_degree:row_of_17", "ties:equal_branches_middle",
                                              "in_degree:row_of_16", "in_edge_ranks:plain_21"]))
    return out
