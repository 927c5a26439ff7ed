#!/usr/bin/env python3
"""Times the tail of stage -5 of ConstructGraph (ResolveContainedReads + ResolveChimericSequences) on a HiFi-like read
set: the path a caller has without Pass1.resolve against Pass1.resolve, on the same box in the same process.

  before   trim_and_annotate -> find_chimeric_regions -> fetch of the lists -> filter_overlaps_by_identity ->
           hip.overlap_update_and_type with the numpy containment marking.  This path has no ResolveChimericSequences
           and no is_maybe_chimeric() exception, so it does LESS work than `after`.
  after    Pass1.resolve(reads, identity, phases=3).

The read set is what tests/test_gpu_fullsize.py generates for the HiFi workload (40x of 15 kb reads, 0.5 % errors), at
--bases (default 20 Mb; 100 Mb when the box's time allows).  A pass takes each phase once, so every `after` sample
runs on a first pass of its own, made outside the timed window; the `before` path leaves the pass as it was (the trim
is idempotent) and reuses one.  Samples alternate.  One warm-up each, then --repeats timed runs (default 5): median,
spread (largest minus smallest), and the share of the edit-distance kernels (common to both paths) from the engine's
per-site kernel timers, which are collected in a second, untimed run of each path.

The requirement it prints a verdict on: the median of `after` does not exceed the median of `before` by more than the
larger of the two spreads.

    python tools/time_resolve.py --bases 20000000 --out profiles/resolve_timing_20mb.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from raven_amd import hip, synth  # noqa: E402

ED_SITES = ("edit_banded", "edit_full", "edit_lane")


def make_reads(bases, seed=0x5EED0021):
    import torch
    dev = torch.device("cuda", 0)
    g = synth.make_genome_torch(bases, seed=seed, device=dev)
    rs, _ = synth.make_reads_torch(g, 40, 15000, length_model="normal", sub=0.001, ins=0.002, dele=0.002, seed=seed + 1)
    return rs


def before(eng, reads, p, identity):
    begin, end, median, invalid = p.trim_and_annotate(4)
    regions = p.find_chimeric_regions(invalid)
    ovl, off = p.overlaps()
    b, e = begin.astype(np.uint32) << 4, end.astype(np.uint32) << 4
    kept, koff = eng.filter_overlaps_by_identity(reads, ovl, off, b, e, invalid, identity)
    upd, ok, ty = hip.overlap_update_and_type(kept, b, e, invalid.astype(np.uint8))
    contained = np.zeros(p.n, bool)
    contained[upd["lhs_id"][(ok == 1) & (ty == 1)]] = True
    contained[upd["rhs_id"][(ok == 1) & (ty == 2)]] = True
    return dict(overlaps=int(ovl.shape[0]), kept=int(kept.shape[0]), contained=int(contained.sum()),
                invalid=int((invalid.astype(bool) | contained).sum()), regions=int(sum(len(r) for r in regions)))


def after(eng, reads, p, identity):
    r = p.resolve(reads, identity=identity, phases=3)
    return dict(contained=int(r["contained"].sum()), invalid=int(r["invalid"].sum()), chimeric=int(r["chimeric"].sum()),
                regions=int(r["regions"].shape[0]), median=r["median"], stats=r["stats"])


def timed(fn, *a):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn(*a)
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def ed_share(eng, fn, *a):
    """Device ms of the edit-distance kernel sites and of all timed sites in one run of `fn`."""
    eng.set_kernel_timing(True)
    eng.reset_stats()
    fn(*a)
    k = eng.kernel_ms()
    eng.set_kernel_timing(False)
    return sum(k[s][0] for s in ED_SITES if s in k), sum(v[0] for v in k.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=20_000_000)
    ap.add_argument("--identity", type=float, default=0.95)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    # torch's HIP runtime first, the library's second: that order works in one process
    if not torch.cuda.is_available() or hip.device_count() < 1:
        raise SystemExit("time_resolve.py needs a GPU: there is nothing to time without one")
    torch.cuda.init()
    rs = make_reads(args.bases)
    eng = hip.Engine(15, 5)
    eng.set_kernel_timing(False)
    reads = eng.upload(rs)

    def first_pass():
        return eng.find_overlaps_and_create_piles(reads)

    t_pass, p_before = timed(first_pass)
    tb, ta, info_b, info_a = [], [], None, None
    for i in range(args.repeats + 1):  # sample 0 is the warm-up of either path
        t, info_b = timed(before, eng, reads, p_before, args.identity)
        if i:
            tb.append(t)
        p = first_pass()
        t, info_a = timed(after, eng, reads, p, args.identity)
        p.close()
        if i:
            ta.append(t)
    ed_b, all_b = ed_share(eng, before, eng, reads, p_before, args.identity)
    p = first_pass()
    ed_a, all_a = ed_share(eng, after, eng, reads, p, args.identity)
    p.close()
    p_before.close()
    med_b, med_a = statistics.median(tb), statistics.median(ta)
    spread_b, spread_a = max(tb) - min(tb), max(ta) - min(ta)
    margin = max(spread_b, spread_a)
    out = {
        "tool": "time_resolve", "device": torch.cuda.get_device_name(0), "bases": args.bases, "reads": int(rs.n),
        "identity": args.identity, "repeats": args.repeats, "first_pass_s": round(t_pass, 4),
        "before": {"median_s": round(med_b, 4), "spread_s": round(spread_b, 4), "runs_s": [round(x, 4) for x in tb],
                   "edit_distance_kernel_ms": round(ed_b, 2), "timed_kernel_ms": round(all_b, 2), "result": info_b},
        "after": {"median_s": round(med_a, 4), "spread_s": round(spread_a, 4), "runs_s": [round(x, 4) for x in ta],
                  "edit_distance_kernel_ms": round(ed_a, 2), "timed_kernel_ms": round(all_a, 2), "result": info_a},
        "margin_s": round(margin, 4),
        "after_not_slower": bool(med_a <= med_b + margin),
        "within_spread": bool(abs(med_a - med_b) <= margin),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0 if out["after_not_slower"] else 1


if __name__ == "__main__":
    sys.exit(main())
