"""The count profile (csrc/mdk_profile_core.h) restated with Python ints: a loop over samples and sites, ``//`` for the level bin's one
division, and ``Fraction`` for the percentile.  ``profile_np`` is the same five tensors from numpy's ``bincount`` in int64 for tables
too large to loop over; tests/test_profile_cpu.py holds it to ``profile``."""
import math
from fractions import Fraction

LIMIT = 1 << 26
E_NEGATIVE, E_ENTRY, E_GROUP = 1, 2, 4
MAX_GROUPS, MAX_DEPTH_BINS, MAX_LEVEL_BINS = 4, 4096, 256


def level_bin(m, d, L):
    """the bin of a covered cell: L equal bins of the methylated fraction, a cell all methylated in the last"""
    return min(L - 1, m * L // d)


def refusal(m, u, group, G):
    """(bit, site) of the refusal that is reported -- the smallest site with one: a negative entry before one too large before a group of
    G or more -- or None"""
    n = len(m[0]) if len(m) else 0
    for k in range(n):
        col = [int(row[k]) for row in m] + [int(row[k]) for row in u]
        if any(v < 0 for v in col):
            return E_NEGATIVE, k
        if any(v >= LIMIT for v in col):
            return E_ENTRY, k
        if group is not None and int(group[k]) >= G:
            return E_GROUP, k
    return None


def profile(m, u, group, G, min_depth, B, L):
    """(depth_hist [S][G][B + 1], level_hist [S][G][L], nmeth_sum, nunmeth_sum, max_depth [S][G]) as lists of ints, of a table without
    refused cells"""
    S = len(m)
    dh = [[[0] * (B + 1) for _ in range(G)] for _ in range(S)]
    lh = [[[0] * L for _ in range(G)] for _ in range(S)]
    ms, us, mx = ([[0] * G for _ in range(S)] for _ in range(3))
    for s in range(S):
        for k, (a, b) in enumerate(zip(m[s], u[s])):
            a, b = int(a), int(b)
            g, d = 0 if group is None else int(group[k]), a + b
            dh[s][g][min(d, B)] += 1
            mx[s][g] = max(mx[s][g], d)
            if d >= min_depth:
                lh[s][g][level_bin(a, d, L)] += 1
                ms[s][g] += a
                us[s][g] += b
    return dh, lh, ms, us, mx


def profile_np(m, u, group, G, min_depth, B, L):
    """the same five as numpy int64 arrays, from int64 arrays [S, n] without refused entries: m L stays below 2^34"""
    import numpy as np
    m, u = np.asarray(m, dtype=np.int64), np.asarray(u, dtype=np.int64)
    S, n = m.shape
    g = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    d = m + u
    covered = d >= min_depth
    lb = np.minimum(L - 1, m * L // np.maximum(d, 1))
    dh, lh = np.zeros((S, G, B + 1), dtype=np.int64), np.zeros((S, G, L), dtype=np.int64)
    ms, us, mx = (np.zeros((S, G), dtype=np.int64) for _ in range(3))
    for s in range(S):
        dh[s] = np.bincount(g * (B + 1) + np.minimum(d[s], B), minlength=G * (B + 1)).reshape(G, B + 1)
        c = covered[s]
        lh[s] = np.bincount(g[c] * L + lb[s][c], minlength=G * L).reshape(G, L)
        ms[s] = np.array([m[s][c & (g == k)].sum() for k in range(G)], dtype=np.int64)
        us[s] = np.array([u[s][c & (g == k)].sum() for k in range(G)], dtype=np.int64)
        mx[s] = np.array([d[s][g == k].max(initial=0) for k in range(G)], dtype=np.int64)
    return dh, lh, ms, us, mx


def add(a, b):
    """the profile of two disjoint site sets, from numpy arrays: the counts and the sums add, max_depth is the larger"""
    import numpy as np
    return tuple(x + y for x, y in zip(a[:4], b[:4])) + (np.maximum(a[4], b[4]),)


class Overflow(Exception):
    """the percentile lies in the overflow bin"""


def depth_quantile(depths, min_depth, B, q):
    """the percentile of one (sample, group) from its cells' depths themselves, by sorting: with N the covered count and k = max(1,
    ceil(Fraction(q) N)), the k-th smallest covered depth; -1 where N is 0; Overflow where that depth is B or more"""
    covered = sorted(int(d) for d in depths if d >= min_depth)
    if not covered:
        return -1
    k = max(1, math.ceil(Fraction(q) * len(covered)))
    v = covered[k - 1]
    if v >= B:
        raise Overflow(v)
    return v
