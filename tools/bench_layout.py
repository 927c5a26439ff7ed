#!/usr/bin/env python
"""Times rvn_layout_force_directed (100 iterations) beside the one-thread host yardstick of the tests
(tests/host/layout_reference.cpp, g++ -O2 -ffp-contract=off: a restatement of the reference's loop, NOT Raven's threaded
build) on the chain-plus-chords graphs of the tests: one component of 5 000, 50 000 and 200 000 points, and 1 000
components of 50 points.  The point counts are illustrations: nobody has measured how many nodes a real assembly graph
has at this stage.  One JSON line per workload; --out appends them to a file.

Device timing: one warm-up call (allocations, code load), then --repeats calls timed wall-clock around the blocking C
call (uploads, the per-iteration flag read-back and the result's download included); the median is reported, all
samples kept.  Per-kernel-site device times come from a further call with the engine's kernel timing on.  The result of
every workload is compared with the yardstick (==) before any time is reported."""
import argparse
import json
import os
import pathlib
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raven_amd import hip  # noqa: E402
from tests import layout_util as lu  # noqa: E402

WORKLOADS = [("1x5000", [5000]), ("1x50000", [50000]), ("1x200000", [200000]), ("1000x50", [50] * 1000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--only", default="", help="comma-separated workload names")
    ap.add_argument("--no-host", action="store_true", help="skip the host column (and the comparison)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    eng = hip.Engine(15, 5)
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="bench_layout"))
    ref_exe = None if a.no_host else lu.build_reference(tmp)
    only = [s for s in a.only.split(",") if s]
    for name, sizes in WORKLOADS:
        if only and name not in only:
            continue
        case = lu.random_case(np.random.default_rng(len(sizes) * 1000003 + sizes[0]), sizes, a.iterations)
        got, st = case.device(eng)  # warm-up
        samples = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            got, st = case.device(eng)
            samples.append(time.perf_counter() - t0)
        eng.set_kernel_timing(True)
        eng.reset_stats()
        case.device(eng)
        sites = {k: {"ms": round(v[0], 3), "launches": v[1]} for k, v in eng.kernel_ms().items() if v[1]}
        eng.set_kernel_timing(False)
        rec = {"workload": name, "points": case.n, "components": len(sizes), "iterations": a.iterations,
               "device_s": float(np.median(samples)), "device_samples_s": samples, "stats": st, "kernel_sites": sites}
        if ref_exe:
            t0 = time.perf_counter()
            want = lu.run_program(ref_exe, case, tmp, None, name)[0]
            rec["host_one_thread_s"] = time.perf_counter() - t0
            rec["host_is"] = "tests/host/layout_reference.cpp (restatement, one thread), not Raven's threaded build"
            rec["equal_to_host"] = lu.same_doubles(got, want)
            rec["host_over_device"] = rec["host_one_thread_s"] / rec["device_s"]
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
