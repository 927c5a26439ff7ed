"""Reference of the alignment-path tests: the global alignment of two code arrays by a plain numpy DP with a traceback
under the tie rule the device walk states (nwpath.h) — from the end: the diagonal where it is optimal (always at equal
bases), then a query base only ('I'), then a target base only ('D') —, as runs `count << 2 | op` in alignment order
(op = EDLIB_EDOP_*: 0 '=', 1 'I', 2 'D', 3 'X'), and racon's window breakpoints derived from runs."""
import numpy as np

OP_EQ, OP_I, OP_D, OP_X = 0, 1, 2, 3


def encode_runs(ops):
    """one op per alignment column -> uint32 runs"""
    ops = np.asarray(ops, dtype=np.uint32)
    if ops.size == 0:
        return np.zeros(0, dtype=np.uint32)
    starts = np.concatenate(([0], np.flatnonzero(ops[1:] != ops[:-1]) + 1))
    counts = np.diff(np.concatenate((starts, [ops.size]))).astype(np.uint32)
    return (counts << np.uint32(2)) | ops[starts]


def expand_runs(runs):
    runs = np.asarray(runs, dtype=np.uint32)
    return np.repeat((runs & 3).astype(np.uint8), (runs >> 2).astype(np.int64))


def dp_runs(query, target):
    """(edit distance, runs) of the global alignment of `query` (columns) against `target` (rows)."""
    q = np.asarray(query, dtype=np.uint8)
    t = np.asarray(target, dtype=np.uint8)
    n, m = len(t), len(q)
    if n == 0 or m == 0:
        return n + m, encode_runs([OP_I] * m + [OP_D] * n)
    ar = np.arange(m + 1, dtype=np.int64)
    prev = ar.copy()
    dirs = np.zeros((n + 1, m + 1), dtype=np.uint8)
    for i in range(1, n + 1):
        neq = q != t[i - 1]
        diag = prev[:-1] + neq
        cand = np.minimum(diag, prev[1:] + 1)
        cur = np.minimum.accumulate(np.concatenate(([i], cand)) - ar) + ar  # the left dependency
        c = cur[1:]
        dirs[i, 1:] = np.where(diag == c, np.where(neq, OP_X, OP_EQ), np.where(cur[:-1] + 1 == c, OP_I, OP_D))
        prev = cur
    ops = []
    i, j = n, m
    while i > 0 and j > 0:
        o = int(dirs[i, j])
        ops.append(o)
        if o != OP_D:
            j -= 1
        if o != OP_I:
            i -= 1
    ops.extend([OP_I] * j)
    ops.extend([OP_D] * i)
    return int(prev[m]), encode_runs(ops[::-1])


def check_runs(runs, query, target, distance):
    """the invariants rvn_align_path_batch states for one pair"""
    runs = np.asarray(runs, dtype=np.uint32)
    op, cnt = runs & 3, (runs >> 2).astype(np.int64)
    assert (cnt > 0).all()
    assert (op[1:] != op[:-1]).all(), "adjacent runs of one op"
    assert cnt[(op == OP_EQ) | (op == OP_X) | (op == OP_I)].sum() == len(query)
    assert cnt[(op == OP_EQ) | (op == OP_X) | (op == OP_D)].sum() == len(target)
    assert cnt[op != OP_EQ].sum() == distance
    assert len(runs) <= 2 * distance + 1


def breakpoints_from_runs(runs, q_begin, t_begin, t_end, w):
    """racon Overlap::find_breaking_points_from_cigar over the runs ('=' and 'X' are its 'M'): per window of w target
    bases that has an aligned pair, the first pair (t, q) and one past the last — rows as oracle.nw_breakpoints' """
    first, last = {}, {}
    tp, qp = t_begin, q_begin  # next target / query base
    for r in np.asarray(runs, dtype=np.uint32):
        op, c = int(r & 3), int(r >> 2)
        if op == OP_I:
            qp += c
        elif op == OP_D:
            tp += c
        else:
            while c > 0:  # an 'M' run, window by window
                wi = tp // w
                take = min(c, (wi + 1) * w - tp)
                first.setdefault(wi, (tp, qp))
                last[wi] = (tp + take, qp + take)
                tp += take
                qp += take
                c -= take
    assert tp == t_end
    out = []
    for wi in sorted(first):
        out.extend([first[wi], last[wi]])
    return np.array(out, dtype=np.uint32).reshape(-1, 2)
