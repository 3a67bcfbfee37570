"""The tables tests/test_moments_cpu.py and tests/test_gpu_moments.py share: seeded count matrices that mix what the moments have to
meet, and the checks that they really do."""
import functools

import numpy as np

import moments_rule as rule

SPECIAL_FROM = 12                                                   # tables of this many samples or more hold the special samples


@functools.lru_cache(maxsize=None)
def table(S, n, seed=1):
    """(nmeth, nunmeth): int64 arrays [S, n], read-only.  A tenth of the cells are `0 0`, placed by a stream of the sample's own; a
    twentieth of the others have a depth of 1 to 4, the rest 5 to 40.  From SPECIAL_FROM samples on: sample 0 is covered nowhere, sample
    1 has one level everywhere (depth 8, 2 methylated: variance 0), sample 3 is sample 2 again, and samples 4 and 5 are covered on the
    even and on the odd sites alone but for site n // 2, where both are -- their one common site (given n >= 3)."""
    rng = np.random.default_rng(1000003 * seed + 1009 * S + n)
    m, u = np.zeros((S, n), dtype=np.int64), np.zeros((S, n), dtype=np.int64)
    for s in range(S):
        own = np.random.default_rng(rng.integers(1 << 62))
        depth = np.where(own.random(n) < 0.05, own.integers(1, 5, n), own.integers(5, 41, n))
        depth = np.where(own.random(n) < 0.10, 0, depth)
        m[s] = (own.random(n) * (depth + 1)).astype(np.int64)
        if s % 3 == 1:
            m[s] = np.where(own.random(n) < 0.5, depth, m[s])       # many cells all methylated: levels of 65536
        u[s] = depth - m[s]
    if S >= SPECIAL_FROM:
        m[0], u[0] = 0, 0
        m[1], u[1] = 2, 6
        m[3], u[3] = m[2], u[2]
        site = np.arange(n)
        for s, parity in ((4, 0), (5, 1)):
            off = (site % 2 != parity) & (site != n // 2)
            m[s], u[s] = np.where(off, 0, m[s] + 3), np.where(off, 0, u[s] + 2)        # (covered at either min_depth where it is on)
    m.setflags(write=False), u.setflags(write=False)
    return m, u


def check_mix(m, u, min_depth):
    """the table holds what it is meant to: asserted, so a change of the generator cannot quietly empty a test"""
    S, n = m.shape
    covered = (m + u) >= min_depth
    ordinary = [s for s in range(S) if S < SPECIAL_FROM or s not in (0, 1, 4, 5)]
    if n >= 63:
        if covered[ordinary].size >= 500:                           # (fewer cells than that say little about a tenth)
            frac = 1.0 - covered[ordinary].mean()
            assert 0.05 <= frac <= 0.20, frac
        if len(ordinary) >= 2 and S < SPECIAL_FROM:
            assert not np.array_equal(covered[ordinary[0]], covered[ordinary[1]])      # placed differently per sample
    if S >= SPECIAL_FROM and n >= 3:
        assert not covered[0].any()
        assert covered[1].all() and len({rule.level(int(a), int(b)) for a, b in zip(m[1], u[1])}) == 1
        assert np.array_equal(m[2], m[3]) and np.array_equal(u[2], u[3]) and covered[2].sum() >= 2
        assert (covered[4] & covered[5]).sum() == 1
        if n >= 63:
            assert not np.array_equal(covered[6], covered[7])                          # placed differently per sample


@functools.lru_cache(maxsize=None)
def expected(S, n, min_depth, seed=1):
    """(n, sx, sxx, sxy as lists of lists of ints, cxy and vxx as lists of lists of 64-bit patterns) of table(S, n, seed)"""
    m, u = table(S, n, seed)
    sums = [a.tolist() for a in rule.moments_np(m, u, min_depth)]
    cxy, vxx = rule.center(*sums)
    return tuple(sums) + (rule.pattern(cxy), rule.pattern(vxx))


# sums written by hand at the limits of what centring accepts: cancellation to 0 and to +-1, 2^92, products that round
LIMIT_SUMS = [
    # n, sx_ij, sx_ji, sxx_ij, sxx_ji, sxy
    (1 << 30, 1 << 46, 1 << 46, 1 << 62, 1 << 62, 1 << 62),        # everything at its bound: both cancel to 0
    (1 << 30, 1 << 46, 0, 1 << 62, 0, 0),                          # vxx_ij = 0, cxy = 0
    (1 << 30, 0, 0, 1 << 62, 1 << 62, 1 << 62),                    # 2^92, nothing subtracted
    (1 << 30, (1 << 46) - 1, (1 << 46) - 1, 1 << 62, 1 << 62, 1 << 62),       # 2^92 - (2^46 - 1)^2 = 2^47 - 1
    (3, 5, 5, 9, 9, 8),                                            # cxy = 24 - 25 = -1, vxx = 2
    (3, 5, 5, 9, 9, 9),                                            # cxy = +2
    (2, 3, 3, 5, 5, 5),                                            # cxy = vxx = +1
    (2, 3, 3, 5, 5, 4),                                            # cxy = -1
    ((1 << 30) - 1, (1 << 45) + 12345, (1 << 44) + 999, (1 << 61) + 7, (1 << 60) + 3, (1 << 60) + 11),
    ((1 << 30) - 3, 3 << 44, 1 << 20, 1 << 61, 1 << 30, (1 << 53) + 1),       # products that need rounding
    (1 << 27, (1 << 27) + 1, (1 << 27) + 3, (1 << 27) + 1, (1 << 27) + 9, 1 << 27),
    (0, 0, 0, 0, 0, 0),
]


def limit_matrices():
    """the hand-written sums as 2 x 2 matrices: cell (0, 1) and (1, 0) are the pair, the diagonals each sample's own"""
    out = []
    for n, a, b, aa, bb, ab in LIMIT_SUMS:
        out.append(([[n, n], [n, n]], [[a, a], [b, b]], [[aa, aa], [bb, bb]], [[aa, ab], [ab, bb]]))
    return out
