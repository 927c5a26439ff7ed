"""The size-class tables of Map's chain stage on the CPU: raven_amd/csrc/sizeclass.h compiled for the host
(tests/host/size_class_host.cpp) against their restatement in tests/chain_util.py (SEG_CLASS_CAPS, CHAIN_SMALL_CAP,
CHAIN_CLASS_CAPS), which the crafted GPU suites build their inputs and their expected launch counts from.  The header is
the one statement the device's class-list kernel and the host's launch ladders go by (segsort.h, chain.hip), so this ties
the Python restatement to them.  Values of n: 0 and 1, the lower bound and one below it, every cap with its two
neighbours, and one value beyond the last cap — the chain tables at chain = 1, 4, 33 and 40 (below, at and beyond the
one-lane kernel's cap)."""
import bisect
import os
import subprocess

from tests import chain_util as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = ["g++", "-std=c++17", "-I", os.path.join(ROOT, "raven_amd", "csrc")]
SOURCE = os.path.join(ROOT, "tests", "host", "size_class_host.cpp")
SEG_MIN = 2  # a read with fewer matches has nothing to sort
CHAINS = (1, 4, 33, 40)


def expected_class(n, caps, min_n):
    """-1: no class (nothing is launched for it); len(caps): beyond the table"""
    return -1 if n < min_n else bisect.bisect_left(caps, n)


def values(caps, min_n):
    v = {0, 1, min_n, min_n - 1, caps[-1] + 1000}
    for cap in caps:
        v.update((cap - 1, cap, cap + 1))
    return sorted(x for x in v if x >= 0)


def cases():
    lines, want = ["tables"], []
    for n in values(cu.SEG_CLASS_CAPS, SEG_MIN):
        lines.append("seg %d" % n)
        want.append(("seg", n, expected_class(n, cu.SEG_CLASS_CAPS, SEG_MIN)))
    for chain in CHAINS:
        min_n = max(cu.CHAIN_SMALL_CAP + 1, chain)
        for n in values(cu.CHAIN_CLASS_CAPS, min_n):
            lines.append("chain %d %d" % (chain, n))
            want.append(("chain %d" % chain, n, expected_class(n, cu.CHAIN_CLASS_CAPS, min_n)))
    return "\n".join(lines) + "\n", want


def check(exe, d):
    text, want = cases()
    path = os.path.join(str(d), "cases.txt")
    with open(path, "w") as f:
        f.write(text)
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-3000:])
    out = run.stdout.splitlines()
    assert out[0].split() == ["seg", str(SEG_MIN)] + [str(c) for c in cu.SEG_CLASS_CAPS]
    assert out[1].split() == ["chain", str(cu.CHAIN_SMALL_CAP)] + [str(c) for c in cu.CHAIN_CLASS_CAPS]
    got = [int(line.split()[1]) for line in out[2:]]
    assert len(got) == len(want)
    wrong = [(w, g) for w, g in zip(want, got) if w[2] != g]
    assert not wrong, wrong[:10]


def test_size_class_matches_the_restatement(tmp_path):
    exe = str(tmp_path / "size_class_host")
    subprocess.check_call(BUILD + ["-O2", "-o", exe, SOURCE])
    check(exe, tmp_path)

