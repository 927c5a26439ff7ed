"""rvn_layout_force_directed (raven_amd/csrc/layout.hip) against the yardstick (tests/host/layout_reference.cpp: the
reference's insertion-built recursive quadtree and loop restated, g++ without contraction): every position compared with
== on the doubles, no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

from raven_amd import hip
from tests import layout_util as lu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def engine():
    return hip.Engine(15, 5)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("layout_gpu")


@pytest.fixture(scope="module")
def ref_exe(work):
    return lu.build_reference(work)


def yardstick(ref_exe, work, case, tag):
    return lu.run_program(ref_exe, case, work, None, tag)[0]


def test_device_sqrt_and_divide_are_correctly_rounded(work):
    """The premise everything else rests on: sqrt(x*x + y*y), a / b and m * (k*k) / (d*d) computed by a kernel built as
    the library's kernels are (layout.h, contraction off) equal the host's IEEE results bit for bit on 2^20 operands of
    the layout's ranges — coordinate differences in [-2, 2] and down to 1e-15 (squared norms down to 1e-30), k between
    1e-3 and 0.5."""
    exe = str(work / "layout_arith")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "raven_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "layout_arith.hip")])
    n = 1 << 20
    rng = np.random.default_rng(99)

    def differences():
        wide = rng.uniform(-2.0, 2.0, n)
        tiny = 10.0 ** rng.uniform(-15.0, 0.3, n) * rng.choice([-1.0, 1.0], n)
        return np.where(rng.random(n) < 0.5, wide, tiny)

    x, y, a = differences(), differences(), differences()
    b = np.where(rng.random(n) < 0.5, 10.0 ** rng.uniform(-15.0, 0.5, n), rng.uniform(1e-3, 0.5, n))
    m = rng.integers(1, 200_000, n).astype(np.uint32)
    k = np.where(rng.random(n) < 0.5, 1.0 / np.sqrt(rng.integers(4, 1_000_000, n)), rng.uniform(1e-3, 0.5, n))
    d = np.abs(differences()) + 1e-15
    src, dst = str(work / "arith.in"), str(work / "arith.out")
    with open(src, "wb") as f:
        f.write(np.uint32(n).tobytes())
        for v in (x, y, a, b, m, k, d):
            f.write(np.ascontiguousarray(v).tobytes())
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    got = np.fromfile(dst, np.float64).reshape(3, n)
    want = [np.sqrt(x * x + y * y), a / b, m.astype(np.float64) * (k * k) / (d * d)]
    for name, g, w in zip(("sqrt(x*x + y*y)", "a / b", "m * (k*k) / (d*d)"), got, want):
        differ = np.flatnonzero(g.view(np.uint64) != w.view(np.uint64))
        print("%s: %d of %d results differ from the host's" % (name, differ.shape[0], n))
        assert differ.shape[0] == 0, (name, differ[:5], g[differ[:5]], w[differ[:5]])


SIZES = [6, 7, 63, 64, 65, 1000]


@pytest.fixture(scope="module")
def one_iteration(ref_exe, work):
    rng = np.random.default_rng(1)
    cases = {m: lu.random_case(rng, [m], 1) for m in SIZES}
    return {m: (c, yardstick(ref_exe, work, c, "one%d" % m)) for m, c in cases.items()}


@pytest.mark.parametrize("m", SIZES)
def test_one_iteration_equals_the_yardstick(engine, one_iteration, m):
    case, want = one_iteration[m]
    got, st = case.device(engine)
    assert lu.same_doubles(got, want) and not np.array_equal(got, case.xy)
    assert st["host_tree_iterations"] == 0 and 1 <= st["max_depth"] <= 32


@pytest.fixture(scope="module")
def several(ref_exe, work):
    rng = np.random.default_rng(2)
    a = lu.random_case(rng, [6, 100, 1000, 4097], 100)          # 5 203 points
    b = lu.random_case(rng, [6, 100, 1000, 4097, 14797], 3)     # 20 000 points
    return {"100_iterations": (a, yardstick(ref_exe, work, a, "several_a")), "3_iterations": (b, yardstick(ref_exe, work, b, "several_b"))}


@pytest.mark.parametrize("name", ["100_iterations", "3_iterations"])
def test_components_of_one_call_are_independent_and_exact(engine, several, name):
    case, want = several[name]
    got, st = case.device(engine)
    assert st["host_tree_iterations"] == 0
    assert lu.same_doubles(got, want)
    for c in range(case.off.shape[0] - 1):
        alone, st1 = case.component(c).device(engine)
        assert st1["host_tree_iterations"] == 0
        assert lu.same_doubles(alone, got[int(case.off[c]):int(case.off[c + 1])])


def test_permuting_the_points_permutes_the_result(engine):
    rng = np.random.default_rng(3)
    case = lu.random_case(rng, [1000], 5)
    perm = rng.permutation(case.n)
    got, _ = case.device(engine)
    moved, _ = case.permuted(perm).device(engine)
    assert lu.same_doubles(moved[perm], got)


@pytest.mark.parametrize("name", sorted(lu.crafted_cases()))
def test_crafted_geometry(engine, ref_exe, work, name):
    """Points on cell boundaries and on a nucleus, on one line, neighbours closer than 0.01; 0, 1 and 3 iterations."""
    for it in (0, 1, 3):
        case = lu.crafted_cases(it)[name]
        got, st = case.device(engine)
        if it == 0:
            assert got.tobytes() == case.xy.tobytes()
            continue
        assert lu.same_doubles(got, yardstick(ref_exe, work, case, "crafted%d" % it)), (name, it)
        assert st["host_tree_iterations"] == 0


@pytest.mark.parametrize("name", sorted(lu.exceptional_cases()))
def test_exceptional_geometry_takes_the_host_tree(engine, ref_exe, work, name):
    """Duplicates in both insertion orders, two points 1e-13 apart, a point no child accepts: equal to the yardstick, with
    iterations counted; a regular component in the same call is not affected and reports none when it runs alone."""
    case = lu.exceptional_cases()[name]
    got, st = case.device(engine)
    assert lu.same_doubles(got, yardstick(ref_exe, work, case, "exc"))
    assert st["host_tree_iterations"] > 0
    regular = lu.random_case(np.random.default_rng(4), [40], case.n_iterations)
    both, st2 = lu.join([regular, case, regular]).device(engine)
    assert st2["host_tree_iterations"] == st["host_tree_iterations"]
    alone, st3 = regular.device(engine)
    assert st3["host_tree_iterations"] == 0
    assert lu.same_doubles(both[:40], alone) and lu.same_doubles(both[40:40 + case.n], got) and lu.same_doubles(both[40 + case.n:], alone)
    assert lu.same_doubles(alone, yardstick(ref_exe, work, regular, "reg"))


def test_argument_errors(engine):
    """RVN_EINVAL (a ValueError here) and nothing launched: the kernel sites' launch counts do not move."""
    rng = np.random.default_rng(6)
    good = lu.random_case(rng, [8, 9], 2)
    engine.set_kernel_timing(True)
    engine.reset_stats()

    def call(off=None, xy=None, adj=None, adj_off=None):
        return engine.layout_force_directed(good.off if off is None else off, good.xy if xy is None else xy,
                                            good.adj_off if adj_off is None else adj_off, good.adj if adj is None else adj, 2)

    bad_xy = [good.xy.copy(), good.xy.copy()]
    bad_xy[0][3, 1] = np.nan
    bad_xy[1][16, 0] = np.inf
    adj_far, adj_other = good.adj.copy(), good.adj.copy()
    adj_far[0] = 17           # beyond the last point
    adj_other[0] = 12         # a point of the other component
    bad_adj_off = good.adj_off.copy()
    bad_adj_off[3] = bad_adj_off[2] - 1 if bad_adj_off[2] else bad_adj_off[4] + 1
    for kw in (dict(off=[0, 9, 8, 17]), dict(off=[1, 8, 17]), dict(off=[0, 8, 8, 17]), dict(xy=bad_xy[0]), dict(xy=bad_xy[1]),
               dict(adj=adj_far), dict(adj=adj_other), dict(adj_off=bad_adj_off)):
        with pytest.raises(ValueError):
            call(**kw)
    launches = engine.kernel_ms()
    assert sum(v[1] for v in launches.values()) == 0
    out, _ = call()
    assert sum(v[1] for v in engine.kernel_ms().values()) > 0 and not np.array_equal(out, good.xy)
    engine.set_kernel_timing(False)


def test_facade_equals_the_restated_function(tmp_path):
    """tests/cpp/layout_facade_test.cpp: raven::CreateForceDirectedLayout on a graph double (junctions, small components, a
    junction-free chain, pruned transitive neighbours) == the restated host function on the same graph, every edge weight,
    two calls in a row (the seed doubles)."""
    exe = str(tmp_path / "layout_facade_test")
    lib = os.path.join(ROOT, "raven_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "tests", "cpp"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "layout_facade_test.cpp"),
                           "-L", lib, "-lraven_hip", "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 2
    for call, ln in enumerate(lines):
        f = ln.split()
        assert f[:2] == ["call", str(call)] and f[2:4] == ["components", "4"], ln
        assert int(f[7]) > 1000 and f[8:10] == ["mismatches", "0"], ln
