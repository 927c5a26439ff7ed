"""Crafted coverage piles for TrimAndAnnotatePiles on the device (raven_amd/csrc/pile.hip: pile_trim_kernel,
pile_chimeric_wave_kernel, pile_chimeric_kernel), each tagged with the class it stands for.

generate() returns (data, offsets, tags): one coverage CSR (uint16 cells, uint64 offsets) and one dict per pile:
  kind      "trim" | "median" | "chim"
  cls       the class of the list in the docstrings below, name = cls + a distinguishing suffix
  coverage  the FindValidRegion threshold the pile was built for (trim / median piles)
  trim      (begin, end, invalid) the pile has BY CONSTRUCTION at that threshold (where the construction says so)
  median    the median it has by construction (numpy's sort of the region, position size // 2)
  regions   the chimeric regions the issue states for the pile (pit piles)
tests/test_pile_cases.py checks every such claim against the oracle on the CPU; tests/test_gpu_pile_annotate.py runs
the kernels over the piles.  Nothing here looks at what the code under test returns."""
import numpy as np

MIN_CELLS = 1260 >> 4  # 78: Pile::FindValidRegion rejects a shorter region
WINDOW = 847 >> 4      # 52: the window of Pile::FindSlopes
LDS_CELLS = 4096       # pile_chimeric_wave_kernel keeps at most this many cells in LDS


def profile(rng, cells):
    """A synthetic coverage profile: plateau with pits (chimeric junctions), spikes (repeats), ramps, noise, zeroed ends."""
    base = int(rng.integers(8, 60))
    d = np.full(cells, base, dtype=np.int64)
    d += rng.integers(-2, 3, size=cells)
    for _ in range(int(rng.integers(0, 5))):  # pits: coverage drops (chimeric junctions), various widths / depths
        c, wdt = int(rng.integers(60, cells - 60)), int(rng.integers(1, 40))
        depth = rng.choice([0.05, 0.2, 0.45, 0.6])
        lo, hi = max(0, c - wdt), min(cells, c + wdt)
        d[lo:hi] = (d[lo:hi] * depth).astype(np.int64)
    for _ in range(int(rng.integers(0, 4))):  # spikes (repeats)
        c, wdt = int(rng.integers(60, cells - 60)), int(rng.integers(3, 80))
        d[max(0, c - wdt):min(cells, c + wdt)] *= int(rng.integers(2, 5))
    if rng.random() < 0.5:  # ramps at the ends, as real piles have
        r = int(rng.integers(10, 60))
        d[:r] = (d[:r] * np.linspace(0.1, 1, r)).astype(np.int64)
        d[-r:] = (d[-r:] * np.linspace(1, 0.1, r)).astype(np.int64)
    if rng.random() < 0.5:  # zeroed outside the valid region (UpdateValidRegion)
        a, b = int(rng.integers(0, 30)), int(rng.integers(0, 30))
        d[:a] = 0
        if b:
            d[-b:] = 0
    if rng.random() < 0.1:
        d[rng.integers(0, cells, size=5)] = 65535  # saturated cells: the clamp matters
    return np.clip(d, 0, 65535).astype(np.uint16)


PIT_LEN = 400
PIT_CELLS = (0, 1, 5, 51, 52, 53, 61, 62, 63, 64, 65, 127, 128, 129, PIT_LEN - 54, PIT_LEN - 53, PIT_LEN - 52, PIT_LEN - 3,
             PIT_LEN - 2)
THRESHOLDS = (1, 4, 300, 65535)
PILE_COUNTS = (1, 3, 4, 5, 257)


def _runs(*parts):
    """Concatenation of (value, count) pairs as uint16 cells."""
    return np.concatenate([np.full(c, v, dtype=np.uint16) for v, c in parts] or [np.zeros(0, np.uint16)])


def _trim_cases(rng):
    """Pile::FindValidRegion: valid region = the first longest run of cells >= coverage that a lower cell terminates."""
    out = []

    def add(cls, name, cells, coverage=4, trim=None):
        t = dict(kind="trim", cls=cls, name=cls + ":" + name, coverage=coverage)
        if trim is not None:
            t["trim"] = trim
        out.append((np.asarray(cells, dtype=np.uint16), t))

    # pile length: below, at and above the 64-cell chunk of the ballot scan, and several chunks
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 4096, 8300):
        framed = _runs((0, 1), (5, n - 2), (0, 1)) if n >= 2 else _runs((5, n))
        add("length", "framed_%d" % n, framed, trim=(1, n - 1, False) if n - 2 >= MIN_CELLS else (0, n, True))
        if n <= 129:
            add("length", "full_%d" % n, _runs((5, n)), trim=(0, n, True))  # no terminator
        if n >= 2:  # random runs of random lengths
            cells = np.zeros(n, dtype=np.uint16)
            i = 0
            while i < n:
                ln = int(rng.integers(1, 200))
                cells[i:i + ln] = int(rng.integers(4, 40)) if rng.random() < 0.7 else int(rng.integers(0, 4))
                i += ln
            add("length", "runs_%d" % n, cells)
    # run start: the first cell of the valid run on lanes 0, 1, 63 and on lanes 0, 1 of the second chunk
    for s in (0, 1, 63, 64, 65):
        add("run_start", "%d" % s, _runs((0, s), (5, 100), (0, 20)), trim=(s, s + 100, False))
    # run end: the terminating lower cell on lanes 63 / 0 / 1.  A run that ends there is followed directly by the
    # longer, valid one: a missed terminator would merge the two
    for t in (63, 64, 65, 127, 128):
        add("run_end", "then_valid_%d" % t, _runs((5, t), (0, 1), (5, t + 20), (0, 7)), trim=(t + 1, 2 * t + 21, False))
        if t >= MIN_CELLS + 1:
            add("run_end", "valid_%d" % t, _runs((0, t - 80), (5, 80), (0, 30)), trim=(t - 80, t, False))
    # a run that reaches the last cell is never recorded
    add("unterminated", "alone", _runs((0, 10), (5, 100)), trim=(0, 110, True))
    add("unterminated", "after_shorter", _runs((0, 1), (5, 80), (0, 1), (5, 200)), trim=(1, 81, False))
    add("unterminated", "from_cell_0", _runs((5, 300)), trim=(0, 300, True))
    # run length at the 78-cell minimum
    for n in (77, 78, 79):
        add("run_length", "%d" % n, _runs((0, 1), (5, n), (0, 1)), trim=(1, n + 1, False) if n >= MIN_CELLS else (0, n + 2, True))
        add("run_length", "%d_at_64" % n, _runs((0, 64), (5, n), (0, 3)),
            trim=(64, 64 + n, False) if n >= MIN_CELLS else (0, n + 67, True))
    # ties for the longest run: the first wins
    add("ties", "two", _runs((0, 3), (5, 90), (0, 1), (7, 90), (0, 2)), trim=(3, 93, False))
    add("ties", "three", _runs((0, 1), (5, 80), (0, 2), (6, 90), (0, 1), (7, 90), (0, 40), (8, 90), (0, 1)), trim=(83, 173, False))
    add("ties", "two_shorter_first", _runs((5, 89), (0, 1), (5, 90), (0, 1), (5, 90), (0, 1)), trim=(90, 180, False))
    # many short runs: both branches of the ballot loop alternate within every chunk
    cells = []
    for _ in range(300):
        cells += [5] * int(rng.integers(1, 4)) + [0] * int(rng.integers(1, 4))
    add("short_runs", "alone", cells, trim=(0, len(cells), True))
    add("short_runs", "then_valid", cells + [5] * 100 + [0], trim=(len(cells), len(cells) + 100, False))
    add("short_runs", "valid_first", [0] + [5] * 100 + [0] + cells, trim=(1, 101, False))
    # thresholds: cells at the threshold form the run, cells one below terminate it
    for cov in THRESHOLDS:
        add("threshold", "at_%d" % cov, _runs((cov - 1, 2), (cov, 100), (cov - 1, 2)), coverage=cov, trim=(2, 102, False))
        add("threshold", "below_%d" % cov, _runs((cov - 1, 120)), coverage=cov, trim=(0, 120, True))
    add("threshold", "all_65535_terminated", _runs((65535, 150), (65534, 1)), coverage=65535, trim=(0, 150, False))
    add("threshold", "all_65535", _runs((65535, 150)), coverage=65535, trim=(0, 150, True))
    # all or nothing
    add("all_or_nothing", "below", _runs((3, 200)), trim=(0, 200, True))
    add("all_or_nothing", "above", _runs((4, 200)), trim=(0, 200, True))
    return out


def _median_cases(rng):
    """Pile::FindMedian: the element at sorted position size // 2 of the valid region; all piles here are valid at
    coverage 4: [0] + region + [0]."""
    out = []

    def add(name, region):
        region = np.asarray(region, dtype=np.uint16)
        assert region.shape[0] >= MIN_CELLS and int(region.min()) >= 4
        region = region[rng.permutation(region.shape[0])]
        n = region.shape[0]
        t = dict(kind="median", cls="median", name="median:" + name, coverage=4, trim=(1, n + 1, False),
                 median=int(np.sort(region)[n // 2]))
        out.append((np.concatenate([[0], region, [0]]).astype(np.uint16), t))
        return t

    def around(v, size=100):
        """size cells with exactly size // 2 below v, v once, the rest above: v is the median.  The neighbours v - 1
        and v + 1 are frequent, so the neighbouring bins of the radix select are not empty."""
        below = size // 2
        lo = np.concatenate([np.full(min(20, below), v - 1), rng.integers(4, v, size=below - min(20, below))])
        n_hi = size - below - 1
        hi = rng.integers(v + 1, 65536, size=n_hi) if v < 65535 else np.full(n_hi, v)  # (65535: nothing lies above)
        hi[:min(20, n_hi)] = min(v + 1, 65535)
        return np.concatenate([lo, [v], hi])

    for v in (5, 255, 256, 257, 65535):
        assert add("all_%d" % v, np.full(100, v))["median"] == v
    assert add("255_256_even", [255] * 50 + [256] * 50)["median"] == 256
    assert add("255_256_odd_low", [255] * 51 + [256] * 50)["median"] == 255
    assert add("255_256_odd_high", [255] * 50 + [256] * 51)["median"] == 256
    assert add("255_256_even_low", [255] * 51 + [256] * 49)["median"] == 255
    t = add("three_high_bytes", np.concatenate([rng.integers(0x100, 0x200, 30), rng.integers(0x200, 0x300, 40),
                                                rng.integers(0x300, 0x400, 30)]))
    assert t["median"] >> 8 == 2
    t = add("minority_high_byte", np.concatenate([rng.integers(0x100, 0x200, 45), rng.integers(0x200, 0x300, 10),
                                                  rng.integers(0x300, 0x400, 45)]))
    assert t["median"] >> 8 == 2
    for b in (0, 1, 2, 3, 252, 253, 254, 255):  # all four sub-bins of lanes 0 and 63, in the second pass ...
        assert add("low_byte_%d" % b, around(0x300 + b))["median"] == 0x300 + b
        assert add("low_byte_%d_top" % b, around(65280 + b))["median"] == 65280 + b
    for b in (0, 1, 2, 3, 252, 253, 254, 255):  # ... and in the first
        assert add("high_byte_%d" % b, around(b * 256 + 128))["median"] == b * 256 + 128
    for n in (78, 79, 128, 4095):
        add("random_%d" % n, rng.integers(4, 65536, size=n))
    return out


def _chimeric_cases(rng):
    """Pile::FindChimericRegions: FindSlopes(1.82) over 52-cell windows, pit pairing, MergeRegions."""
    out = []

    def add(cls, name, cells, **extra):
        out.append((np.asarray(cells, dtype=np.uint16), dict(kind="chim", cls=cls, name=cls + ":" + name, **extra)))

    for i in range(400):
        add("profile", "%d" % i, profile(rng, int(rng.integers(130, 1500))))
    for n in (4032, 4095, 4096, 4097, 4160, 6000):  # around the LDS limit of the wave kernel
        d = profile(rng, n)
        d[n - 104:n - 98] //= 10  # one pit for certain, near the end (behind cell 3990: close to the limit)
        add("profile_long", "%d" % n, d)
    for n in range(1, 131):
        add("random", "%d" % n, rng.integers(0, 60, size=n))
    for c in PIT_CELLS:  # a 2-cell pit at the pile's ends, at the window's width from them and at the chunk boundaries
        d = np.full(PIT_LEN, 40, dtype=np.uint16)
        d[c:c + 2] = 3
        add("pit", "%d" % c, d, regions=[] if c in (0, PIT_LEN - 2) else [[c, c + 1]])
    for w in range(1, 81):  # pits whose first cell is on lane 0 (left wall on lane 63) / whose last cell is on lane 63
        d = np.full(448, 40, dtype=np.uint16)
        d[128:128 + w] = 3
        d[384 - w:384] = 5
        add("wall", "%d" % w, d)
    for n in (64, 128, 4096):  # every second cell is a one-cell run of both kinds
        d = np.full(n, 40, dtype=np.uint16)
        d[1::2] = 3
        add("staircase", "%d" % n, d)
        d = np.full(n, 40, dtype=np.uint16)
        d[0::2] = 3
        add("staircase", "%d_from_0" % n, d)
    d = np.zeros(400, dtype=np.uint16)  # a plateau of 300: the median's high byte is 1; a pit down to 100
    d[20:380] = 300
    d[200:204] = 100
    add("plateau", "300", d)
    for lo in (36008, 36009):  # u16(36009 * 1.82) saturates to 65535, u16(36008 * 1.82) = 65534 does not
        d = np.full(300, 65535, dtype=np.uint16)
        d[100:102] = lo
        d[190:193] = lo
        add("saturated", "pits_%d" % lo, d)
    for i in range(4):
        add("saturated", "mix_%d" % i, rng.choice([65535, 36008, 36009, 20000], size=300, p=[0.55, 0.2, 0.2, 0.05]))
    d = np.full(300, 36009, dtype=np.uint16)
    d[150] = 65535
    add("saturated", "spike", d)
    for v in (50, 100, 150, 250, 1000, 5000, 35000):  # v * 1.82 is an integer in exact arithmetic, not in double
        n = v * 91 // 50
        add("near_integer", "%d" % v, rng.choice([v, n - 1, n, n + 1], size=200, p=[0.4, 0.2, 0.2, 0.2]))
        d = np.full(200, v, dtype=np.uint16)
        d[40], d[100], d[160] = n - 1, n, n + 1
        add("near_integer", "%d_spikes" % v, d)
    return out


def generate(seed=20261018):
    rng = np.random.default_rng(seed)
    piles = _trim_cases(rng) + _median_cases(rng) + _chimeric_cases(rng)
    offsets = np.zeros(len(piles) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([p.shape[0] for p, _ in piles])
    data = np.concatenate([p for p, _ in piles]).astype(np.uint16)
    return data, offsets, [t for _, t in piles]


def pick(data, offsets, idx):
    """The CSR of the piles idx (in that order)."""
    parts = [data[int(offsets[i]):int(offsets[i + 1])] for i in idx]
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([p.shape[0] for p in parts])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint16)).astype(np.uint16), off


def pile(data, offsets, i):
    return data[int(offsets[i]):int(offsets[i + 1])]


def first_sweep_runs(cells):
    """(down runs, up runs) of the first sweep of Pile::FindSlopes(1.82), restated cell by cell: a cell is flagged down
    (up) when the highest cell within 52 on its left (right) is above uint16(min(cell * 1.82, 65535))."""
    d = np.asarray(cells, dtype=np.int64)
    n = d.shape[0]
    lim = np.minimum(d.astype(np.float64) * 1.82, 65535.0).astype(np.int64)
    down = np.array([i > 0 and d[max(0, i - WINDOW):i].max() > lim[i] for i in range(n)], dtype=bool)
    up = np.array([i < n - 1 and d[i + 1:i + 1 + WINDOW].max() > lim[i] for i in range(n)], dtype=bool)

    def starts(f):
        return int(np.count_nonzero(f & ~np.concatenate([[False], f[:-1]])))
    return starts(down), starts(up)


def layers_of(cells):
    """Cell intervals [x, y) whose coverage sum is the profile (first and last cell must be 0): what Pile::AddLayers has
    to be given to build it."""
    d = np.asarray(cells, dtype=np.int64)
    assert d[0] == 0 and d[-1] == 0
    open_at, out = [], []
    for i in range(1, d.shape[0]):
        step = int(d[i] - d[i - 1])
        if step > 0:
            open_at += [i] * step
        for _ in range(-step):
            out.append((open_at.pop(), i))
    assert not open_at
    return out
