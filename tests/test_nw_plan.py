"""The plan of the alignment-path stage on the CPU: raven_amd/csrc/nwplan.h compiled for the host
(tests/host/nw_plan_host.cpp) against a restatement, written here, of the rules as DESIGN.md 3.5b and the comments of
nwpath.h / nwplan.h state them — the variant a job gets, the order of a pass, its chunks and buffer sets, the layout of the
device arrays, the threshold model, the pilot sample and the head.  The restatement never asks the library: the variant
is chosen by the band's ring lanes (not by a closed form of the largest threshold), the order is a stable sort, the fit
is numpy's.  The same program built with -fsanitize=address,undefined runs the same cases once more."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = ["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "raven_amd", "csrc")]
SOURCE = os.path.join(ROOT, "tests", "host", "nw_plan_host.cpp")

VARIANTS = [(1, 4), (1, 8), (1, 16), (1, 32), (1, 64), (2, 64), (4, 64), (8, 64)]  # (R, G), by the band they hold
STRIPED, CLASSES, MAX_STRIPES, HEAD_MAX = 8, 9, 8, 4096
OWN_FIRST, HEAD_ONLY, ROTATING = 0, 1, 2


# ---- the restatement -----------------------------------------------------------------------------------------------------
def band(n, m, k):
    """offsets row - column in [-lo, hi] of the band that holds every alignment of cost <= k"""
    d = abs(n - m)
    return (k - d) // 2 + (d if m > n else 0), (k - d) // 2 + (d if n > m else 0)


def ring_lanes(lo, hi, R):
    return max(1, -(-(64 * R + lo + hi) // (64 * R + 1)))


def fits(n, m, k, R, G):
    return ring_lanes(*band(n, m, k), R) <= G


def largest_threshold(n, m, R, G):
    """largest k (at most n + m) whose band fits a ring of G lanes: by bisection on the ring's lanes, which grow with k"""
    d = abs(n - m)
    if not fits(n, m, d, R, G):
        return 0
    lo, hi = d, 1 << 40  # fits(lo), not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(n, m, mid, R, G) else (lo, mid)
    return min(lo, n + m)


def store(n, m, k, R, S):
    """(hs words, ck entries) a sweep leaves: one word per lane and block every 16 steps, (Pv, Mv) every 32"""
    lo, hi = band(n, m, k)
    n_super = -(-((n + 63) // 64) // R)
    if S == 0:
        L, n_steps = ring_lanes(lo, hi, R), m + n_super
        return -(-n_steps // 16) * L * R, (n_steps // 32) * L * R
    n_stripes = -(-n_super // S)
    gps = (64 * R * S + lo + hi + S + 46) // 16 + 2
    qps = gps // 2 + 1
    return n_stripes * (gps * S * R + 1), n_stripes * qps * S * R


def n_stripes_of(n, R, S):
    return -(-(-(-((n + 63) // 64) // R)) // S)


def plan(n, m, k, stripe_lanes, budget):
    """(R, G, S, k, kcap) or None"""
    k = min(max(k, abs(n - m), 16), n + m)
    for R, G in VARIANTS:
        if G <= stripe_lanes and fits(n, m, k, R, G):
            return R, G, 0, k, largest_threshold(n, m, R, G)
    R, G = VARIANTS[-1]
    if not fits(n, m, k, R, MAX_STRIPES * stripe_lanes):
        return None
    hs, ck = store(n, m, k, R, stripe_lanes)
    if hs * 4 + ck * 16 > budget:
        return None
    return R, G, stripe_lanes, k, largest_threshold(n, m, R, MAX_STRIPES * stripe_lanes)


def level(job):
    n, m, k, R, G, S = job
    return STRIPED if S else VARIANTS.index((R, G))


def order_key(job):
    n, m, k, R, G, S = job
    return level(job), min(n_stripes_of(n, R, S) if S else m >> 3, (1 << 20) - 1)


def set_of(ci, layout):
    return ci % 3 if layout == ROTATING else (3 if ci == 0 else (ci - 1) % 3)


def chunks(jobs, budget, layout, slots):
    """the output lines of a "chunks" case for jobs in pass order"""
    need = [store(n, m, k, R, S) for n, m, k, R, G, S in jobs]
    lines, cut, c0, slot_w, cells = [], [], 0, 0, 0
    while c0 < len(jobs):
        share = budget // 12 if not cut and layout != ROTATING else budget // 3
        c1, hs_w, ck_e, rows = c0, 0, 0, []
        while c1 < len(jobs):
            hw, ce = need[c1]
            if c1 > c0 and (hs_w + hw) * 4 + (ck_e + ce) * 16 > share:
                break
            rows.append("job %d %d %d %d" % (c1, hs_w, ck_e, slot_w if slots else -1))
            slot_w += 2 * jobs[c1][2] + 2 if slots else 0
            lo, hi = band(*jobs[c1][:3])
            cells += jobs[c1][1] * (lo + hi + 1)
            hs_w, ck_e, c1 = hs_w + hw, ck_e + ce, c1 + 1
        counts = [sum(level(j) == x for j in jobs[c0:c1]) for x in range(CLASSES)]
        coff = [sum(counts[x + 1:]) for x in range(CLASSES)] + [c1 - c0]  # widest class first
        cut.append((hs_w, ck_e))
        lines.append("chunk %d %d %d %d %d " % (c0, c1, hs_w, ck_e, set_of(len(cut) - 1, layout)) + " ".join(map(str, coff + counts)))
        lines += rows
        c0 = c1
        if layout == HEAD_ONLY:
            break
    lines.append(" ".join(["left"] + [str(x) for x in range(c0, len(jobs))]))
    lines.append("totals %d %d %d" % (slot_w, cells, max(h * 4 + c * 16 for h, c in cut)))
    for b in range(4):
        mine = [cut[ci] for ci in range(len(cut)) if set_of(ci, layout) == b]
        lines.append("set %d %d %d %d" % (b, bool(mine), max([h for h, _ in mine] + [0]), max([c for _, c in mine] + [0])))
    return lines, cut


def fit(lens, d):
    """(mu, va, vb) or None: mean rate, then least squares of the squared residuals on (len, len^2) without the 2 % largest
    standardised residuals; a fit outside the model puts all spread on the linear term"""
    if len(lens) < 256:
        return None
    mu = d.sum() / lens.sum()
    z = np.abs(d - mu * lens) / np.sqrt(lens)
    keep = z <= np.sort(z)[int(len(z) * 0.98)]
    L, r2 = lens[keep] * 1e-3, ((d - mu * lens) ** 2)[keep]
    s11, s12, s22, t1, t2 = (L ** 2).sum(), (L ** 3).sum(), (L ** 4).sum(), (r2 * L).sum(), (r2 * L * L).sum()
    det = s11 * s22 - s12 * s12
    a = b = -1.0
    if det > 1e-9 * s11 * s22:
        a, b = (t1 * s22 - t2 * s12) / det, (t2 * s11 - t1 * s12) / det
    if not a >= 0 or not b >= 0:
        a, b = (r2 / L).sum() / len(L), 0.0
    return mu, max(a * 1e-3, 0.25 * mu), b * 1e-6


def threshold(model, length, rate):
    if model is None:
        return int(rate * length) + 16
    mu, va, vb = model
    return int(mu * length + 4.5 * np.sqrt(va * length + vb * length * length)) + 6


# ---- the cases: (input text, check of the output lines) ------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 200, 3000, 20000, 300000)


def job_text(j):
    return " ".join(map(str, j))


def plan_cases():
    cases = []
    for budget in (64 << 20, 1 << 30):
        for sl in (1, 2, 4, 64):
            for n in SIZES:
                for m in SIZES:
                    cases.append((n, m, int(0.15 * max(n, m)) + 16, sl, budget))
            # every level at its largest threshold and one beyond: the next variant with G <= stripe_lanes, or stripes
            for lvl, (R, G) in enumerate(VARIANTS):
                n, m = (300000, 299990) if lvl % 2 else (299950, 300000)
                cap = largest_threshold(n, m, R, G)
                assert abs(n - m) < cap < n + m
                cases += [(n, m, cap, sl, budget), (n, m, cap + 1, sl, budget)]
            cases += [(300000, 300000, 40000, sl, budget),  # beyond the widest ring: stripes (sl = 64; refused below)
                      (300000, 300000, 3500 * sl, sl, budget), (300000, 300000, 4200 * sl, sl, budget),  # eight stripes: just in, out
                      (300000, 300000, 300000, sl, budget),   # beyond eight stripes of any size
                      (200, 200, 1000, sl, budget), (63, 1, 1 << 40, sl, budget),  # k > n + m: clamped
                      (3000, 200, 5, sl, budget), (200, 205, 0, sl, budget), (20000, 20000, 3, sl, budget)]  # k < max(|n - m|, 16)
    want = [plan(*c) for c in cases]
    # the cases meet what they are there for
    by = dict(zip(cases, want))
    for budget in (64 << 20, 1 << 30):
        for lvl, (R, G) in enumerate(VARIANTS):
            n, m = (300000, 299990) if lvl % 2 else (299950, 300000)
            cap = largest_threshold(n, m, R, G)
            assert by[(n, m, cap, 64, budget)][:3] == (R, G, 0) and by[(n, m, cap, 64, budget)][4] == cap
            nxt = by[(n, m, cap + 1, 64, budget)]
            if lvl + 1 < len(VARIANTS):
                assert nxt[:3] == VARIANTS[lvl + 1] + (0,)
            else:  # beyond the widest ring: stripes, whose store (~250 MB) the small budget does not hold
                assert nxt is None if budget == 64 << 20 else nxt[:3] == (8, 64, 64)
        assert by[(300000, 300000, 300000, 64, budget)] is None
        assert by[(200, 200, 1000, 64, budget)][3] == 400 and by[(3000, 200, 5, 64, budget)][3] == 2800
        assert by[(200, 205, 0, 64, budget)][3] == 16
    assert by[(300000, 300000, 40000, 64, 1 << 30)][:3] == (8, 64, 64)  # striped; its store (~280 MB) beyond 64 MB: refused
    assert by[(300000, 300000, 40000, 64, 64 << 20)] is None
    assert by[(300000, 300000, 14000, 4, 1 << 30)][:3] == (8, 64, 4) and by[(300000, 300000, 16800, 4, 1 << 30)] is None
    text = "".join("plan %d %d %d %d %d\n" % c for c in cases)
    lines = ["plan 0" if p is None else "plan 1 %d %d %d %d %d" % p for p in want]
    return text, lambda out: _same(out, lines)


def planned(n, m, k, sl=64):
    R, G, S, k, _ = plan(n, m, k, sl, 1 << 40)
    return n, m, k, R, G, S


def order_cases():
    rng = np.random.default_rng(5)
    lens = [300, 2400, 5600, 12000, 24000, 48000, 100000, 200000]  # one per variant at 12.5 % distance
    jobs = []
    for x in range(56):
        n = lens[x % 8] + (0 if x % 3 else int(rng.integers(0, 64)))  # equal keys among them: ties keep todo order
        jobs.append(planned(n, n - n // 50, n // 8))
    for n in (9000, 9000, 30000, 16000, 9000, 70000, 70000, 3000):  # striped (stripes of four lanes), by number of stripes
        jobs.append(planned(n, n, n // 8, sl=4))
    assert sorted({level(j) for j in jobs}) == list(range(CLASSES))
    assert len({order_key(j) for j in jobs}) < len(jobs) - 10
    todo = [int(x) for x in rng.permutation(len(jobs))]
    # the 20-bit length field saturates: 2^24 and 2^23 columns tie, 2^23 - 16 do not
    big = [(1 << 24, 1 << 24, 16, 8, 64, 0), (1 << 23, 1 << 23, 16, 8, 64, 0), (1 << 23, (1 << 23) - 16, 16, 8, 64, 0),
           (1 << 23, 1 << 24, 16, 8, 64, 0)]
    cases = [(jobs, todo), (jobs, todo[:20]), (jobs[:1], [0]), (big, [2, 1, 0, 3]), (big, [3, 2, 0, 1])]
    text, lines = "", []
    for js, td in cases:
        text += "order %d %d\n" % (len(js), len(td)) + "".join(job_text(j) + "\n" for j in js) + " ".join(map(str, td)) + "\n"
        want = sorted(td, key=lambda i: tuple(-v for v in order_key(js[i])))  # stable, descending
        lines.append(" ".join(["order"] + [str(i) for i in want]))
    assert lines[3] == "order 1 0 3 2" and lines[4] == "order 3 0 1 2"
    return text, lambda out: _same(out, lines)


def chunk_jobs():
    rng = np.random.default_rng(9)
    jobs = [planned(100000, 99000, 12000)]  # its store is beyond every share of the budget below: alone in its chunk
    for length in (300, 900, 2400, 5600, 12000, 24000, 48000):
        for _ in range(5):
            n = length + int(rng.integers(0, length // 4))
            jobs.append(planned(n, n - int(rng.integers(0, n // 40 + 1)), n // 8))
    jobs += [planned(n, n, n // 8, sl=4) for n in (20000, 15000, 9000, 9000)]
    assert len(jobs) == 40
    return sorted(jobs, key=lambda j: tuple(-v for v in order_key(j)))  # a pass is cut in its order


def chunk_cases():
    jobs = chunk_jobs()
    total = sum(h * 4 + c * 16 for h, c in (store(n, m, k, R, S) for n, m, k, R, G, S in jobs))
    budget = 3 * total // 5
    text, lines = "", []
    for layout in (OWN_FIRST, HEAD_ONLY, ROTATING):
        for slots in (0, 1):
            text += "chunks %d %d %d %d\n" % (len(jobs), layout, slots, budget) + "".join(job_text(j) + "\n" for j in jobs)
            got, cut = chunks(jobs, budget, layout, slots)
            lines += got
            # what the case is there for: several chunks, a lone job beyond the share, every set in use
            if layout == HEAD_ONLY:
                assert len(cut) == 1 and len(got[-6].split()) > 10
            else:
                assert len(cut) >= 5 and max(h * 4 + c * 16 for h, c in cut) > budget // 3
                assert [set_of(ci, layout) for ci in range(5)] == ([3, 0, 1, 2, 0] if layout == OWN_FIRST else [0, 1, 2, 0, 1])
    return text, lambda out: _same(out, lines)


def layout_cases():
    sizes = (1, 4095, 4096, 300000)

    def check(out):
        assert len(out) == 16 * len(sizes)
        for x, nj in enumerate(sizes):
            rows = [ln.split() for ln in out[16 * x:16 * x + 16]]
            arrays = {r[2]: (r[1], int(r[3]), int(r[4])) for r in rows[:14]}
            assert len(arrays) == 14 and rows[14][0] == "sizes" and rows[15] == ["pointers", "1"]
            size = {"words": int(rows[14][1]), "jobs": int(rows[14][2])}
            for block in ("words", "jobs"):
                spans = sorted((off, off + n) for b, off, n in arrays.values() if b == block)
                assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans  # no two overlap
                assert spans[-1][1] <= size[block]  # the last one ends inside the block
            for p in ("head", "retry"):
                assert all(arrays["%s.%s" % (p, a)][2] == HEAD_MAX for a in ("jobs", "res", "status", "idx"))
            assert all(arrays["all.%s" % a][2] >= nj for a in ("jobs", "res", "status", "idx"))
            assert arrays["side_next"][2] == len(VARIANTS) and arrays["next"][2] >= 1

    return "".join("layout %d\n" % nj for nj in sizes), check


def fit_cases():
    rng = np.random.default_rng(2024)
    asked = np.array([500, 1000, 2000, 4000, 8000, 12000, 20000, 30000, 40000, 50000], np.float64)

    def sample(count, lens=None, noise=1.0):
        lens = rng.integers(500, 50001, count).astype(np.float64) if lens is None else np.full(count, lens, np.float64)
        d = 0.1 * lens + noise * rng.standard_normal(count) * np.sqrt(0.1 * lens + 1e-4 * lens * lens)
        return lens, np.maximum(np.rint(d), 0.0)

    # the model's own shape; one length only (no second regressor: all spread on the linear term), the same with next to no
    # noise (the floor of a quarter of mu); too few observations (no model: the rate rule)
    samples = [sample(1024), sample(1024, lens=8000), sample(1024, lens=8000, noise=0.01), sample(255)]
    rate = 0.13
    text = ""
    for lens, d in samples:
        text += "fit %d %r %d\n" % (len(lens), rate, len(asked)) + "".join("%d %d\n" % (a, b) for a, b in zip(lens, d))
        text += " ".join("%d" % a for a in asked) + "\n"

    def check(out):
        assert len(out) == 2 * len(samples)
        for x, (lens, d) in enumerate(samples):
            model = fit(lens, d)
            got_model = [float(v) for v in out[2 * x].split()[1:]]
            got = [int(v) for v in out[2 * x + 1].split()[1:]]
            want = [threshold(model, a, rate) for a in asked]
            assert len(got) == len(want) and all(abs(g - w) <= 1 for g, w in zip(got, want)), (x, got, want)
            if model is None:
                assert got_model[0] < 0 and got == [int(rate * a) + 16 for a in asked]
            else:
                assert np.allclose(got_model, model, rtol=1e-9, atol=0)
        assert 0.09 < float(out[0].split()[1]) < 0.11 and float(out[0].split()[3]) > 0  # both terms fitted
        assert float(out[2].split()[3]) == 0 and float(out[2].split()[2]) > 0.25 * float(out[2].split()[1])
        assert float(out[4].split()[3]) == 0 and float(out[4].split()[2]) == 0.25 * float(out[4].split()[1])

    return text, check


def pilot_cases():
    rng = np.random.default_rng(31)
    lens = rng.integers(1000, 1500, 6000)  # many equal lengths: the head's cut falls among ties
    stride = len(lens) // 1400
    cap = np.sort(lens)[len(lens) * 3 // 4]
    pilot = [x for x in range(len(lens)) if x % stride == stride // 2 and lens[x] <= cap]
    assert stride == 4 and len(pilot) > 1024  # the cap of 1 024 cuts
    n_head = min(HEAD_MAX, len(lens) // 8)
    head = sorted(sorted(range(len(lens)), key=lambda i: (-lens[i], i))[:n_head])
    assert lens[head].min() == np.sort(lens)[-n_head] == np.sort(lens)[-n_head - 1]
    lines = [" ".join(["pilot"] + [str(i) for i in pilot[:1024]]), " ".join(["head"] + [str(i) for i in head]),
             "rest %d" % (len(lens) - n_head)]
    return "pilot %d\n" % len(lens) + " ".join(map(str, lens)) + "\n", lambda out: _same(out, lines)


def rate_cases():
    rng = np.random.default_rng(77)
    text, lines = "", []
    for count in (31, 32, 1000):
        r = rng.uniform(0.01, 0.2, count)
        text += "rate %d 0.125\n" % count + " ".join(repr(float(v)) for v in r) + "\n"
        want = 0.125 if count < 32 else float(np.sort(r)[min(count - 1, int(count * 0.9))]) * 1.05 + 0.002
        lines.append("rate %.17g" % want)
    return text, lambda out: _same(out, lines)


CASES = (plan_cases, order_cases, chunk_cases, layout_cases, fit_cases, pilot_cases, rate_cases)


def _same(out, lines):
    assert len(out) == len(lines), (len(out), len(lines))
    for x, (a, b) in enumerate(zip(out, lines)):
        assert a == b, "line %d: program %r, restatement %r" % (x, a, b)


def _run(exe, text, path):
    with open(path, "w") as f:
        f.write(text)
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-3000:])
    return run.stdout.splitlines()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("nw_plan")
    exe = str(d / "nw_plan_host")
    subprocess.check_call(BUILD + ["-O2", "-pthread", "-o", exe, SOURCE])
    return exe, d


@pytest.mark.parametrize("cases", CASES, ids=lambda c: c.__name__)
def test_plan_matches_the_restatement(program, cases):
    exe, d = program
    text, check = cases()
    check(_run(exe, text, str(d / (cases.__name__ + ".txt"))))


def test_same_cases_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone host program: nothing sanitized is loaded into Python."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "nw_plan_host_san")
    build = subprocess.run(BUILD + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-o", exe,
                                    SOURCE], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtimes")
    assert build.returncode == 0, build.stderr
    for cases in CASES:
        text, check = cases()
        check(_run(exe, text, str(tmp_path / (cases.__name__ + ".txt"))))
