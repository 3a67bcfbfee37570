"""Hand-made tables for the smoothing tests (tests/test_smooth_cpu.py, tests/test_gpu_smooth.py) and their expected results, computed
once per (table, parameters) by tests/smooth_rule.py and shared."""
import random

import smooth_rule as rule

# (half_bases, min_sites): no window beyond the site; min_sites alone; half_bases alone, small and larger; BSmooth's shape at a tenth; a
# window that min_sites always decides and that is most of a contig or all of it
PARAMS = ((0, 1), (0, 3), (5, 1), (50, 7), (500, 70), (3, 200))


def table(n, S, seed):
    """(contig, start, nmeth, nunmeth): n rows strictly ascending over several contigs -- one-site contigs among them, no contig above 600
    rows, their sizes such that contigs change inside a wavefront's 64 rows and inside a tile and hardly ever at a multiple of 64 --, dense
    runs of consecutive starts, steps of up to 200 and gaps of thousands; S rows of counts with a tenth of the entries uncovered and
    the LAST sample uncovered over a stretch of 260 rows (whole windows of it have no depth)"""
    rng = random.Random(seed)
    contig, start = [], []
    c = 0
    while len(start) < n:
        size = rng.choice((1, 1, 2, 5, 37, 70, 150, 301, 600))
        x = rng.randint(0, 5000)
        dense = 0
        for _ in range(min(size, n - len(start))):
            contig.append(c); start.append(x)
            if dense:
                dense -= 1; x += 1
            elif rng.random() < 0.08:
                dense = rng.randint(3, 40); x += 1
            elif rng.random() < 0.05:
                x += rng.randint(1000, 9000)
            else:
                x += rng.randint(1, 200)
        c += rng.choice((1, 1, 3))                  # (contig indices need not be consecutive)
    m, u = [[0] * n for _ in range(S)], [[0] * n for _ in range(S)]
    hole = range(n // 3, min(n, n // 3 + 260))
    for s in range(S):
        for i in range(n):
            if rng.random() < 0.1 or (s == S - 1 and i in hole):
                continue
            depth = rng.randint(1, 30)
            m[s][i] = rng.randint(0, depth); u[s][i] = depth - m[s][i]
    return contig, start, m, u


_tables, _windows, _expected = {}, {}, {}


def shared_table(n, S, seed):
    key = (n, S, seed)
    if key not in _tables:
        _tables[key] = table(n, S, seed)
    return _tables[key]


def expected(n, S, seed, half_bases, min_sites, kernel):
    """rule.smooth of shared_table(n, S, seed), computed once; the windows once per (table, half_bases, min_sites)"""
    key = (n, S, seed, half_bases, min_sites, kernel)
    if key not in _expected:
        contig, start, m, u = shared_table(n, S, seed)
        wkey = (n, S, seed, half_bases, min_sites)
        if wkey not in _windows:
            _windows[wkey] = rule.windows(contig, start, half_bases, min_sites)
        _expected[key] = rule.smooth(contig, start, m, u, half_bases, min_sites, kernel, win=_windows[wkey])
    return _expected[key]
