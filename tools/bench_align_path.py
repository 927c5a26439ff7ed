"""Numbers of DESIGN §3.5c: rvn_align_path_batch against rvn_edit_distance_batch (the distance-only floor) on the same
pairs, the bytes of runs against the bytes of ops, and the expansion kernel alone.  One call each after a warm-up.
    python tools/bench_align_path.py [--pairs 20000]   ->  one JSON line per workload"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raven_amd import hip  # noqa: E402


def make_pairs(rng, n_pairs, length, sub, ins, dele):
    """n_pairs targets of `length` random bases, the queries = the targets with iid errors (one vectorised pass)"""
    t = rng.integers(0, 4, size=n_pairs * length, dtype=np.uint8)
    r = rng.random(t.size, dtype=np.float32)
    q = t.copy()
    is_sub = r < sub
    q[is_sub] = (q[is_sub] + rng.integers(1, 4, size=int(is_sub.sum()), dtype=np.uint8)) % 4
    cnt = np.ones(t.size, dtype=np.int8)
    is_ins = (r >= sub) & (r < sub + ins)
    cnt[is_ins] = 2
    cnt[(r >= sub + ins) & (r < sub + ins + dele)] = 0
    ends = np.cumsum(cnt, dtype=np.int64)
    q = np.repeat(q, cnt)
    pos = ends[is_ins] - 1
    q[pos] = rng.integers(0, 4, size=pos.size, dtype=np.uint8)
    cut = np.concatenate(([0], ends[length - 1::length]))
    reads, pairs = [], []
    for p in range(n_pairs):
        qq = q[cut[p]:cut[p + 1]]
        strand = p & 1
        reads.append(qq if strand else (3 - qq[::-1]).astype(np.uint8))
        reads.append(t[p * length:(p + 1) * length])
        pairs.append((2 * p, 0, len(qq), 2 * p + 1, 0, length, strand, 0))
    return reads, np.array(pairs, dtype=hip.ALIGN_PAIR_DTYPE)


def run(eng, name, reads, pairs):
    L = hip.lib()
    both = eng.upload_codes(reads)
    eng.set_kernel_timing(True)

    def paths():
        h = C.c_void_p()
        t0 = time.perf_counter()
        hip._check(L.rvn_align_path_batch(eng._h, both._h, both._h, hip._p(pairs), pairs.shape[0], C.byref(h)))
        return h, (time.perf_counter() - t0) * 1e3

    h, _ = paths()  # warm-up: buffers, streams, the rate estimate
    L.rvn_paths_destroy(h)
    eng.edit_distance_batch(both, pairs.view(hip.ED_PAIR_DTYPE))
    eng.reset_stats()
    h, wall = paths()
    k = eng.kernel_ms()
    n, n_runs, n_ops, n_bad = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    hip._check(L.rvn_paths_info(h, C.byref(n), C.byref(n_runs), C.byref(n_ops), C.byref(n_bad)))
    off = np.zeros(n.value + 1, dtype=np.uint64)
    ops = np.zeros(n_ops.value, dtype=np.uint8)
    dist = np.zeros(n.value, dtype=np.uint32)
    hip._check(L.rvn_paths_fetch(h, hip._p(dist), None, None))
    eng.reset_stats()
    t0 = time.perf_counter()
    hip._check(L.rvn_paths_fetch_ops(h, hip._p(off), hip._p(ops)))
    fetch_ops_wall = (time.perf_counter() - t0) * 1e3
    eng.reset_stats()  # (folds the fetch's event pairs in)
    k2 = eng.kernel_ms()
    L.rvn_paths_destroy(h)
    t0 = time.perf_counter()
    d2, ed_ms, _ = eng.edit_distance_batch(both, pairs.view(hip.ED_PAIR_DTYPE))
    ed_wall = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(dist, d2)
    print(json.dumps({
        "workload": name, "pairs": int(n.value), "not_aligned": int(n_bad.value), "mean_distance": float(dist.mean()),
        "align_path_wall_ms": round(wall, 1), "kernel_ms_of_the_call": {s: round(v[0], 2) for s, v in k.items() if v[1]},
        "edit_distance_wall_ms": round(ed_wall, 1), "edit_distance_device_ms": round(ed_ms, 1),
        "runs_bytes": int(n_runs.value) * 4, "ops_bytes": int(n_ops.value),
        "fetch_ops_wall_ms": round(fetch_ops_wall, 1), "kernel_ms_of_fetch_ops": {s: round(v[0], 2) for s, v in k2.items() if v[1]}}),
        flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20000)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    eng = hip.Engine(15, 5)
    run(eng, "ont_10kb", *make_pairs(rng, a.pairs, 10_000, 0.04, 0.03, 0.03))
    run(eng, "hifi_15kb", *make_pairs(rng, a.pairs, 15_000, 0.002, 0.0015, 0.0015))


if __name__ == "__main__":
    main()
