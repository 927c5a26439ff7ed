#!/usr/bin/env python3
"""Times ConstructAssemblyGraph + the marking of RemoveTransitiveEdges on the device against their single-threaded
restatement (tests/host/graph_reference.cpp), on the overlaps the device chain leaves behind
rvn_resolve_repeat_induced_overlaps (first pass -> valid regions -> second pass -> repeats), for two workloads:

  c2     30x of 10 kb reads with ONT-like errors (bench.py's c2 read model)
  hifi   40x of 15 kb reads with 0.5 % errors, second pass with identity 0.95

Per workload it reports
  device_ms        rvn_construct_assembly_graph + rvn_graph_mark_transitive + rvn_graph_fetch_transitive: one warm-up,
                   then --repeats runs, HIP events on the null stream around the entry points (they return with their
                   stream idle, so the event interval is the call) and the wall clock beside them; median and spread
  restatement_s    the same two steps on one host thread (the program's own clocks, without its file I/O)
  overlap_fetch_ms the device-to-host copy of the surviving overlaps (32 bytes each) that a host graph needs first
  out_degree       the distribution the cost of the transitive step depends on (sum over nodes of the out-degrees of
                   their heads)
and writes profiles/graph_timing_<workload>.json.  No ratio is asserted: the numbers are what DESIGN.md 3.12 quotes.

    python tools/time_graph.py --workload c2 --bases 5000000
"""
import argparse
import json
import os
import pathlib
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raven_amd import hip, synth  # noqa: E402
from tests import graph_util as gu  # noqa: E402
from tests import repeats_util as ru  # noqa: E402


def make_reads(workload, bases, seed=0x5EED0031):
    import torch
    g = synth.make_genome_torch(bases, seed=seed, device=torch.device("cuda", 0))
    if workload == "hifi":
        rs, _ = synth.make_reads_torch(g, 40, 15000, length_model="normal", sub=0.001, ins=0.002, dele=0.002, seed=seed + 1)
    else:
        rs, _ = synth.make_reads_torch(g, 30, 10000, length_model="fixed", sub=0.04, ins=0.03, dele=0.03, seed=seed + 1)
    return rs


def chain(eng, rs, identity):
    """the arguments of rvn_construct_assembly_graph from the device stages in front of it"""
    rd = eng.upload(rs)
    p = eng.find_overlaps_and_create_piles(rd)
    b, e, median, invalid = p.trim_and_annotate(4)
    data, off = p.piles()
    p.close()
    begin, end = b.astype(np.uint32) << 4, e.astype(np.uint32) << 4
    # (the second pass maps nothing when every pile is valid: some are made invalid as ResolveContainedReads would)
    invalid = (invalid | (np.random.default_rng(7).random(rs.n) < 0.15)).astype(np.uint8)
    res = eng.find_overlaps_and_repetitive_regions(rd, begin, end, invalid, freq=0.001, kmer_len=15, identity=identity)
    invalid = (invalid | res["contained"]).astype(np.uint8)
    cov = [data[int(off[i]):int(off[i + 1])] for i in range(rs.n)]
    rd.close()
    rep = ru.StageInput(res["overlaps"], cov, res["kmers"], begin, end, median, invalid).device(eng)
    return gu.ConstructInput(rep["overlaps"], begin, end, median, invalid)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c2", "hifi"], default="c2")
    ap.add_argument("--bases", type=int, default=5_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available() or hip.device_count() < 1:
        raise SystemExit("time_graph.py needs a GPU: there is nothing to time without one")
    torch.cuda.init()
    rs = make_reads(args.workload, args.bases)
    eng = hip.Engine(15, 5)
    t0 = time.perf_counter()
    inp = chain(eng, rs, 0.95 if args.workload == "hifi" else 0.0)
    chain_s = time.perf_counter() - t0

    ev_ms, wall_ms, marked, graph = [], [], 0, None
    for i in range(args.repeats + 1):  # sample 0 is the warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        a.record()
        g = inp.device(eng)
        order, pairs = g.mark_transitive()
        b.record()
        torch.cuda.synchronize()
        if i:
            wall_ms.append((time.perf_counter() - t) * 1e3)
            ev_ms.append(a.elapsed_time(b))
        marked = int(order.shape[0])
        if i == args.repeats:
            graph = g.fetch()
        g.close()

    # the copy a host graph needs first: the surviving overlaps, device to (pageable) host
    m = inp.overlaps.shape[0]
    d = torch.zeros(max(1, m) * 32, dtype=torch.uint8, device="cuda")
    fetch_ms = []
    for i in range(args.repeats + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        d.cpu()
        if i:
            fetch_ms.append((time.perf_counter() - t) * 1e3)

    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        ref = gu.build_reference(tmp)
        ref_c, ref_t, want = [], [], None
        for i in range(3):
            want, err = gu.run_construct(ref, inp, tmp, "timing")
            mt = re.search(r"construct ([0-9.e+-]+) s, transitive ([0-9.e+-]+) s", err)
            ref_c.append(float(mt.group(1)))
            ref_t.append(float(mt.group(2)))
    same = all(np.array_equal(graph[k], want[k]) for k in gu.CONSTRUCT_KEYS) and np.array_equal(order, want["order"]) and \
        np.array_equal(pairs, want["pairs"])

    deg = np.bincount(graph["tail"], minlength=int(want["n_nodes"])) if graph["tail"].shape[0] else np.zeros(1, np.int64)
    walk_pairs = int(deg[graph["head"]].sum()) if graph["tail"].shape[0] else 0
    q = [int(x) for x in np.percentile(deg, [50, 90, 99, 100])]
    out = {
        "tool": "time_graph", "device": torch.cuda.get_device_name(0), "workload": args.workload, "bases": args.bases,
        "reads": int(rs.n), "chain_s": round(chain_s, 3), "overlaps": int(m), "nodes": int(want["n_nodes"]),
        "edges": int(want["n_edges"]), "marked": marked, "same_as_restatement": bool(same),
        "device_ms": {"median_events": round(statistics.median(ev_ms), 3), "median_wall": round(statistics.median(wall_ms), 3),
                      "spread_wall": round(max(wall_ms) - min(wall_ms), 3), "runs_wall": [round(x, 3) for x in wall_ms]},
        "restatement_s": {"construct": round(statistics.median(ref_c), 4), "transitive": round(statistics.median(ref_t), 4)},
        "overlap_fetch_ms": {"median": round(statistics.median(fetch_ms), 3), "bytes": int(m) * 32},
        "out_degree": {"median": q[0], "p90": q[1], "p99": q[2], "max": q[3], "two_step_walks": walk_pairs},
    }
    print(json.dumps(out))
    path = args.out or os.path.join(ROOT, "profiles", "graph_timing_%s.json" % args.workload)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
