#!/usr/bin/env python3
"""Times RemoveBubbles' device side against its single-threaded restatement (tests/host/bubble_reference.cpp, its strings
and its plain Myers distance: the RESTATEMENT, not Raven's build).

Three parts (--parts), written to profiles/bubble_timing_<tag>.json; no ratio is asserted, the numbers are what DESIGN.md 3.14
quotes, the places where the device loses included.

  facade      raven::RemoveBubbles of include/raven_hip/bubbles.hpp (tests/cpp/bubble_facade_test.cpp) on a generated
              chain with planted bubbles (tests/bubble_util.py: chain_with_bubbles; --bubbles of them, arms of --arm
              bases): its prediction batch, its loop and its misses, beside the restatement's loop on one thread.  The two
              are first compared for equality (return value, surviving nodes and edges, number of tests).  The junctions,
              tests and misses, the lengths and distances of the tested pairs and the launches per edit-distance kernel
              site (which stage the pairs took) are recorded.
  diploid     the same comparison and the same records on the graph the device chain leaves behind the transitive removal
              (tools/time_unitigs.py: graph_after_transitive) for reads of TWO haplotypes: a random genome of --diploid
              bases and a copy with a substitution every ~1 000 bases and a short deletion every ~20 000 (raven_amd/synth.py
              makes genome and reads), 15x of 10 kb ONT-like reads of each.  What it is for: how many junctions, how many
              complex bubbles, how long their paths, the prediction's hit rate.  (At these settings the graph comes out as a
              chain without a junction: DESIGN.md 3.14.)
  long sweep  three pairs (100 kb, 250 kb and 500 kb at 5 % substitutions) through rvn_path_similarity_batch by the
              workgroup ring (the default) and by the usual route (engine option ed_wide_lanes = 1: lane window, wave ring,
              full sweep), each once after a warm-up on a small pair, with the edit-distance kernel sites' launch counts.

    python tools/time_bubbles.py --bubbles 400 --arm 5000
"""
import argparse
import json
import os
import pathlib
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raven_amd import hip, seqio, synth  # noqa: E402
from tests import bubble_util as bu  # noqa: E402
from tests import unitig_util as uu  # noqa: E402


def build_facade(d):
    exe = str(d / "bubble_facade_test")
    lib = os.path.join(ROOT, "raven_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "bubble_facade_test.cpp"), "-L", lib, "-lraven_hip",
                           "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run_both(case, d, extra):
    """The restatement and the facade program on one graph: compared, then what both counted and what the facade timed."""
    ref = bu.build_reference(d)
    want = bu.reference(ref, case, d, "t")
    src, dst = str(d / "f.in"), str(d / "f.out")
    with open(src, "wb") as f:
        f.write(bu.reference_blob(case))
    exe = build_facade(d)
    runs = []
    for i in range(3):  # the first run carries the process's first touch of the device; the second is quoted; the third
        # counts the launches per edit-distance kernel site (its event pairs are kept out of the quoted times)
        r = subprocess.run([exe, src, dst] + (["sites"] if i == 2 else []), capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("facade run failed: " + r.stdout + r.stderr)
        words = " ".join(x for x in r.stdout.splitlines() if not x.startswith("sites")).split()
        runs.append(dict(popped=int(words[1]), junctions=int(words[3]), checked=int(words[5]), predicted=int(words[7]),
                         misses=int(words[9]), predict_s=float(words[words.index("predict") + 1]),
                         loop_s=float(words[words.index("loop") + 1]), miss_s=float(words[words.index("misses", 10) + 1])))
    site_words = r.stdout.splitlines()[0].split()[1:]
    sites = {site_words[i]: dict(launches=int(site_words[i + 1]), ms=float(site_words[i + 2])) for i in range(0, len(site_words), 3)}
    rd = bu.Reader(open(dst, "rb").read())
    popped = int(rd.one(np.uint32))
    rd.take(np.uint64, 4)
    same = (popped == want["popped"] and np.array_equal(rd.take(np.uint8, case.n_nodes), want["node_alive"]) and
            np.array_equal(rd.take(np.uint8, len(case.table.tail)), want["edge_alive"]) and runs[-1]["checked"] == len(want["tests"]) and
            runs[-1]["junctions"] == want["n_junctions"])
    if not same:
        raise SystemExit("the facade and the restatement differ")
    tests = want["tests"]
    live = int((np.asarray(case.table.tail, np.uint32) != 0xFFFFFFFF).sum())
    out = dict(nodes=case.n_nodes, edge_slots=len(case.table.tail), live_edges=live, popped=popped, restatement_loop_s=want["seconds"],
               restatement_tests=len(tests), facade_first_run=runs[0], facade=runs[1], edit_distance_sites=sites,
               pair_lengths=[[t["l"], t["r"]] for t in tests][:64],
               pair_distances=[None if t["distance"] == bu.BY_LENGTH else t["distance"] for t in tests][:64],
               verdicts=dict(similar=sum(t["similar"] for t in tests), by_length=sum(t["distance"] == bu.BY_LENGTH for t in tests),
                             by_score=sum((not t["similar"]) and t["distance"] != bu.BY_LENGTH for t in tests)))
    out.update(extra)
    return out


def time_facade(args, d):
    g = bu.chain_with_bubbles(np.random.default_rng(args.seed), n_bubbles=args.bubbles, arm=args.arm, node_len=args.arm // 2,
                              step=args.arm // 6)
    return run_both(g.case, d, dict(bubbles=args.bubbles, arm=args.arm))


def time_diploid(args, d):
    from tools.time_unitigs import graph_after_transitive
    rng = np.random.default_rng(args.seed)
    h1 = synth.make_genome(args.diploid, seed=0x5EED0041)
    h2 = h1.copy()
    snp = rng.choice(args.diploid, size=args.diploid // 1000, replace=False)
    h2[snp] = (h2[snp] + rng.integers(1, 4, size=snp.shape[0]).astype(np.uint8)) & 3
    cut = np.concatenate([np.arange(p, p + int(rng.integers(1, 30))) for p in rng.choice(args.diploid - 30, size=max(1, args.diploid // 20000), replace=False)])
    h2 = np.delete(h2, cut)
    sets = [synth.make_reads(h, 15, 10000, seed=0x5EED0042 + i)[0] for i, h in enumerate((h1, h2))]
    codes = [rs.codes(i) for rs in sets for i in range(rs.n)]
    rs = seqio.pack_reads(codes)
    eng = hip.Engine(15, 5)
    rd = eng.upload(rs)
    table, node_pile, node_cov, begin, end = graph_after_transitive(eng, rs, rd)
    case = uu.Case(codes)
    for k in range(0, table.n_nodes, 2):
        pile = int(node_pile[k])
        case.node([(pile, int(begin[pile]), int(end[pile] - begin[pile]), 0)])
    case.table = table
    return run_both(case, d, dict(haplotype_bases=args.diploid, variants=dict(substitutions=int(snp.shape[0]), deleted_bases=int(cut.shape[0])),
                                  reads=int(rs.n)))


def time_long_sweep(args, d):
    eng = hip.Engine(15, 5)
    eng.set_kernel_timing(True)
    rng = np.random.default_rng(args.seed)
    warm = rng.integers(0, 4, size=2000).astype(np.uint8)
    eng.path_similarity(eng.upload_codes([warm, bu.plant(rng, warm, 50)]), [(0, 1)])
    ref = bu.build_reference(d)
    rows = []
    for n in args.long:
        a = rng.integers(0, 4, size=n).astype(np.uint8)
        b = bu.plant(rng, a, n // 20)
        t0 = time.perf_counter()
        want = int(bu.distances(ref, [(a, b)], d, "l%d" % n)[0])
        cpu_s = time.perf_counter() - t0
        rd = eng.upload_codes([a, b])
        row = dict(bases=n, distance=want, restatement_s=cpu_s)
        for name, lanes in (("workgroup_ring", -1), ("full_sweep", 1)):
            eng.set_option("ed_wide_lanes", lanes)
            eng.reset_stats()
            t0 = time.perf_counter()
            similar, dist = eng.path_similarity(rd, [(0, 1)])
            wall = time.perf_counter() - t0
            la = {k: (round(v[0], 3), v[1]) for k, v in eng.kernel_ms().items() if k.startswith("edit_") and v[1]}
            if int(dist[0]) != want or int(similar[0]) != 1:
                raise SystemExit("%s at %d bases: distance %d, the restatement's %d" % (name, n, int(dist[0]), want))
            row[name] = dict(wall_s=wall, kernels_ms_launches=la)
            print(json.dumps(row), flush=True)
        eng.set_option("ed_wide_lanes", -1)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bubbles", type=int, default=400)
    ap.add_argument("--arm", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--long", type=int, nargs="*", default=[100_000, 250_000, 500_000])
    ap.add_argument("--diploid", type=int, default=1_000_000, help="bases of one haplotype")
    ap.add_argument("--parts", nargs="*", default=["facade", "long", "diploid"], choices=["facade", "long", "diploid"])
    ap.add_argument("--tag", default="generated")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        d = pathlib.Path(tmp)
        out = {}
        if "facade" in args.parts:
            out["facade"] = time_facade(args, d)
            print(json.dumps(out["facade"]), flush=True)
        if "long" in args.parts:
            out["long_sweep"] = time_long_sweep(args, d)
        if "diploid" in args.parts:
            out["diploid"] = time_diploid(args, d)
            print(json.dumps(out["diploid"]), flush=True)
    path = args.out or os.path.join(ROOT, "profiles", "bubble_timing_%s.json" % args.tag)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
