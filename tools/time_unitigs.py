#!/usr/bin/env python3
"""Times CreateUnitigs on the device against its single-threaded restatement (tests/host/unitig_reference.cpp), on the graph
the device chain leaves behind the transitive removal (first pass -> valid regions -> second pass -> repeats ->
rvn_construct_assembly_graph -> rvn_graph_mark_transitive, the marked edges taken out of the host's table), with
epsilon = 42 as in front of the layout, for bench.py's c2 read model (30x of 10 kb reads with ONT-like errors).

It reports
  device_ms      rvn_graph_from_edges is NOT in it (the graph handle exists when the call is made); rvn_tiling_from_piles
                 + rvn_graph_create_unitigs + rvn_unitigs_as_reads (every new node): one warm-up, then --repeats runs, HIP
                 events on the null stream around the entry points and the wall clock beside them; median and spread
  host_s         the restatement's loop on one host thread (the program's own clock, without its file I/O), and
                 rvn_reads_upload_codes of the strings it made: the way the first targets take today.  The host side is
                 the RESTATEMENT, not Raven's build.
Every run is first compared for equality (tables and packed words).  Writes profiles/unitig_timing_<tag>.json; no ratio is
asserted: the numbers are what DESIGN.md 3.13 quotes.

    python tools/time_unitigs.py --bases 5000000
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

from raven_amd import hip  # noqa: E402
from tests import graph_util as gu  # noqa: E402
from tests import repeats_util as ru  # noqa: E402
from tests import unitig_util as uu  # noqa: E402
from tools.time_graph import make_reads  # noqa: E402


def graph_after_transitive(eng, rs, rd):
    """(edge table, node_pile, node_coverage, pile begin / end in bases) behind the transitive removal"""
    p = eng.find_overlaps_and_create_piles(rd)
    b, e, median, invalid = p.trim_and_annotate(4)
    data, off = p.piles()
    p.close()
    begin, end = b.astype(np.uint32) << 4, e.astype(np.uint32) << 4
    end = np.minimum(end, rs.lengths.astype(np.uint32))
    invalid = (invalid | (np.random.default_rng(7).random(rs.n) < 0.15)).astype(np.uint8)
    res = eng.find_overlaps_and_repetitive_regions(rd, begin, end, invalid, freq=0.001, kmer_len=15, identity=0.0)
    invalid = (invalid | res["contained"]).astype(np.uint8)
    cov = [data[int(off[i]):int(off[i + 1])] for i in range(rs.n)]
    rep = ru.StageInput(res["overlaps"], cov, res["kmers"], begin, end, median, invalid).device(eng)
    g = gu.ConstructInput(rep["overlaps"], begin, end, median, invalid).device(eng)
    order, _ = g.mark_transitive()
    f = g.fetch()
    g.close()
    table = gu.EdgeTable(int(f["node_pile"].shape[0]))
    tail = f["tail"].copy()
    tail[order] = gu.EMPTY
    table.tail, table.head, table.length = tail.tolist(), f["head"].tolist(), f["length"].tolist()
    return table, f["node_pile"], f["node_coverage"], begin, end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=5_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--epsilon", type=int, default=42)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available() or hip.device_count() < 1:
        raise SystemExit("time_unitigs.py needs a GPU: there is nothing to time without one")
    torch.cuda.init()
    rs = make_reads("c2", args.bases)
    eng = hip.Engine(15, 5)
    rd = eng.upload(rs)
    table, node_pile, node_cov, begin, end = graph_after_transitive(eng, rs, rd)
    n = table.n_nodes
    count = np.ones(n, np.uint32)
    t, h, ln = table.arrays()
    graph = eng.graph_from_edges(n, t, h, ln)

    ev_ms, wall_ms, got, words = [], [], None, None
    for i in range(args.repeats + 1):  # sample 0 is the warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        tl = eng.tiling_from_piles(rd, node_pile, begin, end)
        u = graph.create_unitigs(tl, count, node_cov, args.epsilon)
        targets = u.as_reads(hip.UNITIGS_ALL)
        b.record()
        torch.cuda.synchronize()
        if i:
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            ev_ms.append(a.elapsed_time(b))
        if i == args.repeats:
            got, words = u.fetch(), targets.fetch()[:3]
        for x in (targets, u, tl):
            x.close()

    # the restatement on the same graph: nodes as the valid regions of their reads, as strings
    case = uu.Case([rs.codes(i) for i in range(rs.n)])
    for k in range(0, n, 2):
        pile = int(node_pile[k])
        case.node([(pile, int(begin[pile]), int(end[pile] - begin[pile]), 0)], coverage=int(node_cov[k]))
    case.table = table
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        ref = uu.build_reference(tmp)
        blob = case.reference_blob(args.epsilon, 9999)
        loop_s, want = [], None
        for i in range(3):
            b_, p = gu._run(ref, "unitigs", blob, tmp, "timing")
            loop_s.append(float(re.search(r"unitigs ([0-9.e+-]+) s", p.stderr).group(1)))
        want = uu.reference(ref, case, args.epsilon, tmp, "timing")
    up_ms = []
    for i in range(args.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = eng.upload_codes(want["sequences"])
        torch.cuda.synchronize()
        if i:
            up_ms.append((time.perf_counter() - t0) * 1e3)
        host_words = x.fetch()[:3]
        x.close()
    same = all(np.array_equal(got[k], want[k]) for k in uu.TABLE_KEYS) and all(np.array_equal(a_, b_) for a_, b_ in zip(words, host_words))

    out = {
        "tool": "time_unitigs", "device": torch.cuda.get_device_name(0), "bases": args.bases, "reads": int(rs.n), "epsilon": args.epsilon,
        "nodes": int(n), "edge_slots": int(t.shape[0]), "live_edges": int((t != gu.EMPTY).sum()),
        "unitigs": int(want["begin"].shape[0] // 2), "members": int(want["members"].shape[0]),
        "unitig_bases": int(want["length"].astype(np.int64).sum()), "same_as_restatement": bool(same),
        "device_ms": {"median_events": round(statistics.median(ev_ms), 3), "median_wall": round(statistics.median(wall_ms), 3),
                      "spread_wall": round(max(wall_ms) - min(wall_ms), 3), "runs_wall": [round(x, 3) for x in wall_ms]},
        "host_s": {"restatement_loop": round(statistics.median(loop_s), 5),
                   "upload_codes_ms": round(statistics.median(up_ms), 3)},
        "note": "the host side is the restatement (tests/host/unitig_reference.cpp), not Raven's build",
    }
    print(json.dumps(out))
    tag = "c2" if args.bases == 5_000_000 else "c2_%dmb" % (args.bases // 1_000_000)
    path = args.out or os.path.join(ROOT, "profiles", "unitig_timing_%s.json" % tag)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
