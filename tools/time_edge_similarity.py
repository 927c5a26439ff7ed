#!/usr/bin/env python3
"""Times rvn_graph_edge_similarity against its single-threaded restatement (tests/host/edge_similarity_reference.cpp, its
strings and its plain Myers distance: the RESTATEMENT, not Raven's build).

Graphs (--parts), each written to profiles/edge_similarity_timing_<tag>.json; no figure is fixed in advance, the numbers are
what DESIGN.md 3.15 quotes, the places where the device loses included.

  c2          the graph the device chain leaves behind rvn_resolve_repeat_induced_overlaps for 30x of 10 kb ONT-like reads
              (tools/time_graph.py: chain), once with every edge of ConstructAssemblyGraph (before the transitive removal) and
              once with the marked edges' slots emptied (behind it).  Every node is one segment: the direct route.
  generated   --edges overlaps of about --overlap bases at --rate divergence between nodes that are tilings of three segments
              of either strand each (tests/edge_sim_util.py: overlap_case): the packed route.
  long        two overlaps of --long bases at --rate: distances beyond the wave ring.  The pair's time with the workgroup
              ring (the default) and without it (engine option ed_wide_lanes = 1: the full sweep, one wave).

Per graph: the device call (one warm-up, then --repeats runs; HIP events on the null stream around the entry point, which
returns with its stream idle, and the wall clock beside them), the restatement's loop on one thread of the same box (its
own clock, without file I/O), the share of edges on each route, and, from one more run with the kernel timers on, the
launches and device time per edit-distance site and of the two new sites.  Every run is first compared for equality.

    python tools/time_edge_similarity.py --bases 1000000 --edges 2000
"""
import argparse
import json
import os
import pathlib
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from raven_amd import hip  # noqa: E402
from tests import edge_sim_util as eu  # noqa: E402
from tests import graph_util as gu  # noqa: E402
from tests import unitig_util as uu  # noqa: E402

SITES = ("edge_pairs", "slice_pack", "edit_lane", "edit_banded", "edit_wide", "edit_full")


def mutate_fast(rng, seq, rate):
    """tests/edge_sim_util.py's mutate in numpy: substitutions, insertions and deletions at rate / 3 each."""
    seq = np.asarray(seq, np.uint8)
    r = rng.random(seq.shape[0])
    out = np.where((r >= 2 * rate / 3) & (r < rate), (seq + rng.integers(1, 4, size=seq.shape[0]).astype(np.uint8)) & 3, seq)
    ins = np.flatnonzero((r >= rate / 3) & (r < 2 * rate / 3))
    out = np.insert(out, ins, rng.integers(0, 4, size=ins.shape[0]).astype(np.uint8))
    keep = np.ones(out.shape[0], bool)
    keep[np.flatnonzero(r < rate / 3) + np.searchsorted(ins, np.flatnonzero(r < rate / 3))] = False
    return out[keep].astype(np.uint8)


def routes(case, want):
    """Share of edge slots per route, from the tiling's segment counts and the restatement's lengths."""
    segs = np.array([len(t) for t in case.tiling])
    t, h, _ = case.table.arrays()
    live = t != gu.EMPTY
    single = np.zeros(t.shape[0], bool)
    single[live] = (segs[t[live]] == 1) & (segs[h[live]] == 1)
    swept = live & (want["lhs_length"] > 0)
    return dict(slots=int(t.shape[0]), empty=int((~live).sum()), no_sweep=int((live & ~swept).sum()), direct=int((swept & single).sum()),
                packed=int((swept & ~single).sum()))


def measure(eng, case, tmp, tag, repeats, device=None):
    """One graph: the restatement, the device call compared with it, the timings."""
    import torch
    ref = eu.build_reference(tmp)
    want = eu.reference(ref, case, tmp, tag)
    rd, tl, g = device if device is not None else eu.device(eng, case)
    ev_ms, wall_ms, got = [], [], None
    for i in range(repeats + 1):  # sample 0 is the warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        got = g.edge_similarity(tl)
        b.record()
        torch.cuda.synchronize()
        if i:
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            ev_ms.append(a.elapsed_time(b))
    same = all(np.array_equal(got[k], want[k]) for k in ("lhs_length", "rhs_length", "distance")) and \
        np.array_equal(eu.bits(got["score"]), eu.bits(want["score"]))
    eng.set_kernel_timing(True)
    eng.reset_stats()
    g.edge_similarity(tl)
    sites = {k: dict(launches=int(v[1]), ms=round(float(v[0]), 3)) for k, v in eng.kernel_ms().items() if k in SITES}
    eng.set_kernel_timing(False)
    swept = want["lhs_length"] > 0
    d, l = want["distance"][swept].astype(np.float64), want["lhs_length"][swept].astype(np.float64)
    out = dict(graph=tag, nodes=case.n_nodes, routes=routes(case, want), same_as_restatement=bool(same),
               device_ms=dict(median_events=round(statistics.median(ev_ms), 3), median_wall=round(statistics.median(wall_ms), 3),
                              spread_wall=round(max(wall_ms) - min(wall_ms), 3), runs_wall=[round(x, 3) for x in wall_ms]),
               restatement_loop_s=round(want["seconds"], 4), sites=sites,
               overlaps=dict(bases_lhs=int(l.sum()), median_lhs=int(np.median(l)) if l.size else 0, max_lhs=int(l.max()) if l.size else 0,
                             median_divergence=round(float(np.median(d / l)), 4) if l.size else 0.0,
                             max_distance=int(d.max()) if d.size else 0))
    return out, (rd, tl, g)


def c2_graphs(eng, bases):
    """(case before the transitive removal, case behind it, device reads, pile begin / end) of the c2 chain"""
    import time_graph
    rs = time_graph.make_reads("c2", bases)
    inp = time_graph.chain(eng, rs, 0.0)
    g = inp.device(eng)
    order, _ = g.mark_transitive()
    f = g.fetch()
    g.close()
    begin, end = inp.begin.astype(np.uint32), np.minimum(inp.end.astype(np.uint32), rs.lengths.astype(np.uint32))
    cases = []
    for behind in (False, True):
        case = uu.Case([rs.codes(i) for i in range(rs.n)])
        for k in range(0, int(f["node_pile"].shape[0]), 2):
            pile = int(f["node_pile"][k])
            case.node([(pile, int(begin[pile]), int(end[pile] - begin[pile]), 0)])
        tail = f["tail"].copy()
        if behind:
            tail[order] = gu.EMPTY
        case.table.tail, case.table.head, case.table.length = tail.tolist(), f["head"].tolist(), f["length"].tolist()
        cases.append(case)
    return cases, rs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="c2,generated,long")
    ap.add_argument("--bases", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=2000)
    ap.add_argument("--overlap", type=int, default=5000)
    ap.add_argument("--rate", type=float, default=0.19)
    ap.add_argument("--long", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available() or hip.device_count() < 1:
        raise SystemExit("time_edge_similarity.py needs a GPU: there is nothing to time without one")
    torch.cuda.init()
    eng = hip.Engine(15, 5)
    parts = args.parts.split(",")
    ok = True
    note = "the host side is the restatement (tests/host/edge_similarity_reference.cpp) on one thread, not Raven's build"

    def write(tag, body):
        body = dict(tool="time_edge_similarity", device=torch.cuda.get_device_name(0), note=note, **body)
        print(json.dumps(body))
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, "edge_similarity_timing_%s.json" % tag), "w") as f:
            f.write(json.dumps(body, indent=1) + "\n")

    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        if "c2" in parts:
            cases, rs = c2_graphs(eng, args.bases)
            runs = []
            for case, tag in zip(cases, ("before_transitive", "behind_transitive")):
                r, dev = measure(eng, case, tmp, tag, args.repeats)
                for x in dev[::-1]:
                    x.close()
                runs.append(r)
                ok = ok and r["same_as_restatement"]
            write("c2", dict(bases=args.bases, reads=int(rs.n), graphs=runs))
        if "generated" in parts:
            rng = np.random.default_rng(0x5EED0315)
            lengths = np.maximum(64, rng.normal(args.overlap, args.overlap / 4, size=args.edges)).astype(np.int64)
            case = eu.overlap_case(rng, [int(x) for x in lengths], args.rate, multi=True, flip=True, mutator=mutate_fast)
            r, dev = measure(eng, case, tmp, "generated_unitigs", args.repeats)
            for x in dev[::-1]:
                x.close()
            ok = ok and r["same_as_restatement"]
            write("generated", dict(edges=args.edges, overlap=args.overlap, rate=args.rate, graphs=[r]))
        if "long" in parts:
            rng = np.random.default_rng(0x5EED0316)
            case = eu.overlap_case(rng, [args.long], args.rate, mutator=mutate_fast)
            runs = []
            dev = None
            for lanes, tag in ((-1, "workgroup_ring"), (1, "without_workgroup_ring")):
                eng.set_option("ed_wide_lanes", lanes)
                r, dev = measure(eng, case, tmp, tag, 1, device=dev)
                runs.append(r)
                ok = ok and r["same_as_restatement"]
            eng.set_option("ed_wide_lanes", -1)
            write("long", dict(overlap=args.long, rate=args.rate, graphs=runs))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
