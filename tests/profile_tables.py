"""The tables tests/test_profile_cpu.py and tests/test_gpu_profile.py share: seeded count matrices and group columns that mix what the
profile has to meet, the checks that they really do, and the cells at the boundaries of the level bins."""
import functools

import numpy as np

import profile_rule as rule

PLANTED_FROM = 8                                                    # tables of this many cells or more hold the planted depths
LEVEL_BINS = (1, 2, 3, 20, 255, 256)


@functools.lru_cache(maxsize=None)
def table(S, n, B, seed=1):
    """(nmeth, nunmeth): int64 arrays [S, n], read-only.  Depths as a library has them: Poisson around 10, a tenth of the cells `0 0`, a
    twentieth of the others 1 to 4 deep; levels bimodal -- four cells in ten all methylated, three in ten not at all, the rest uniform.
    From PLANTED_FROM cells on six cells, spread over the table, hold the depths 0, 3, B - 1, B, B + 1 and 2: what lies next to
    min_depth 1 and 5 and next to the overflow bin."""
    rng = np.random.default_rng(7000003 * seed + 1013 * S + 31 * n + B)
    depth = rng.poisson(10.0, (S, n)).astype(np.int64)
    depth = np.where(rng.random((S, n)) < 0.05, rng.integers(1, 5, (S, n)), depth)
    depth = np.where(rng.random((S, n)) < 0.10, 0, depth)
    if S * n >= PLANTED_FROM:
        flat = depth.reshape(-1)
        for j, d in enumerate((0, 3, B - 1, B, B + 1, 2)):
            flat[S * n * (j + 1) // 7] = d
    kind = rng.random((S, n))
    m = np.where(kind < 0.4, depth, np.where(kind < 0.7, 0, (rng.random((S, n)) * (depth + 1)).astype(np.int64)))
    m = np.minimum(m, depth)
    u = depth - m
    m.setflags(write=False), u.setflags(write=False)
    return m, u


@functools.lru_cache(maxsize=None)
def groups(n, G, seed=1):
    """a group column: n uint8 entries below G, read-only; None for G = 1, the call without a column"""
    if G == 1:
        return None
    g = np.random.default_rng(9000011 * seed + 17 * n + G).integers(0, G, n).astype(np.uint8)
    g.setflags(write=False)
    return g


def check_mix(m, u, B):
    """the table holds what it is meant to: asserted, so a change of the generator cannot quietly empty a test"""
    d = m + u
    if d.size >= PLANTED_FROM:
        assert (d == 0).any() and ((d > 0) & (d < 5)).any()         # depth 0, and depths below min_depth 5
        assert (d == B - 1).any() and (d == B).any() and (d == B + 1).any()
    if d.size >= 1000:
        assert 0.05 <= (d == 0).mean() <= 0.2 and 8 <= np.median(d[d > 4]) <= 12
        assert ((m == d) & (d > 0)).mean() > 0.3 and ((m == 0) & (d > 0)).mean() > 0.2


@functools.lru_cache(maxsize=None)
def expected(S, n, G, B, L, min_depth, seed=1):
    """the five numpy arrays of table(S, n, B, seed) grouped by groups(n, G, seed)"""
    m, u = table(S, n, B, seed)
    out = rule.profile_np(m, u, groups(n, G, seed), G, min_depth, B, L)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def boundary_cells(L):
    """(nmeth, nunmeth) cells whose level m L / d lies at or next to a bin's lower bound l / L: depths next to the powers of two up to
    2^27 - 2, the largest there is, and m the three integers around l d / L for the first, a middle and the last two l -- among them
    those with m L equal to l d - 1, l d and l d + 1 --, m = 0 and m = d, and entries of 2^26 - 1"""
    top = rule.LIMIT - 1
    depths = sorted({d for k in range(1, 27) for d in ((1 << k) - 1, 1 << k, (1 << k) + 1)} | {2 * top, 2 * top - 1, top, top + 1, 1})
    cells = [(top, top), (top, 0), (0, top), (top, 1), (1, top), (top - 1, top)]
    for d in depths:
        ms = {0, d}
        for l in sorted({1, 2, (L + 1) // 2, L - 1, L}):
            ms |= {l * d // L - 1, l * d // L, l * d // L + 1}
        cells += [(a, d - a) for a in sorted(ms) if 0 <= a <= min(d, top) and d - a <= top]
    return tuple(dict.fromkeys(cells))
