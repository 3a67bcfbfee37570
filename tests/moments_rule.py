"""The pairwise sample moments (csrc/mdk_moments_core.h) restated with Python ints: a loop over pairs and sites, 128-bit quantities as
plain ints, and ``float(int)`` -- correctly rounded, ties to even -- for the one conversion.  ``moments_np`` is the same sums as exact int64
matrix products for tables too large to loop over; tests/test_moments_cpu.py holds it to ``moments``."""
import struct

LIMIT = 1 << 26
ONE = 65536
MAX_SITES = 1 << 30
E_NEGATIVE, E_ENTRY = 1, 2
E_SUM_NEGATIVE, E_SUM_N, E_SUM_SX, E_SUM_SQ = 1, 2, 4, 8


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def level(m, u):
    """the level of a covered cell: the methylated fraction in units of 2^-16, rounded half up"""
    d = m + u
    return (2 * m * ONE + d) // (2 * d)


def refusal(m, u):
    """(bit, site) of the refusal that is reported -- the smallest site with a refused entry, negative before too large -- or None"""
    n = len(m[0]) if m else 0
    for k in range(n):
        col = [row[k] for row in m] + [row[k] for row in u]
        if any(v < 0 for v in col):
            return E_NEGATIVE, k
        if any(v >= LIMIT for v in col):
            return E_ENTRY, k
    return None


def cells(m, u, min_depth):
    """per sample and site (covered, level): an uncovered cell has level 0"""
    out = []
    for ms, us in zip(m, u):
        out.append([(1, level(a, b)) if a + b >= min_depth else (0, 0) for a, b in zip(ms, us)])
    return out


def moments(m, u, min_depth):
    """n, sx, sxx, sxy as lists of lists of ints, over the sites where both samples are covered"""
    w = cells(m, u, min_depth)
    S = len(w)
    n, sx, sxx, sxy = ([[0] * S for _ in range(S)] for _ in range(4))
    for i in range(S):
        for j in range(S):
            for (ci, xi), (cj, xj) in zip(w[i], w[j]):
                if ci and cj:
                    n[i][j] += 1
                    sx[i][j] += xi
                    sxx[i][j] += xi * xi
                    sxy[i][j] += xi * xj
    return n, sx, sxx, sxy


def moments_np(m, u, min_depth):
    """the same four matrices as numpy int64 arrays, from int64 arrays [S, n] without refused entries: every product and sum stays below 2^63"""
    import numpy as np
    m, u = np.asarray(m, dtype=np.int64), np.asarray(u, dtype=np.int64)
    d = m + u
    c = (d >= min_depth).astype(np.int64)
    x = np.where(c == 1, (2 * m * ONE + d) // np.maximum(2 * d, 1), 0)
    return c @ c.T, x @ c.T, (x * x) @ c.T, x @ x.T


def sums_refusal(n, sx, sxx, sxy):
    """(bit, cell) of the first refused cell of the four sums, row-major, or None"""
    S = len(n)
    for i in range(S):
        for j in range(S):
            a, b, c, d = n[i][j], sx[i][j], sxx[i][j], sxy[i][j]
            if min(a, b, c, d) < 0:
                return E_SUM_NEGATIVE, i * S + j
            if a > MAX_SITES:
                return E_SUM_N, i * S + j
            if b > a * ONE:
                return E_SUM_SX, i * S + j
            if c > a << 32 or d > a << 32:
                return E_SUM_SQ, i * S + j
    return None


def center(n, sx, sxx, sxy):
    """cxy and vxx as lists of lists of floats: exact ints, rounded once"""
    S = len(n)
    cxy = [[float(int(n[i][j]) * int(sxy[i][j]) - int(sx[i][j]) * int(sx[j][i])) for j in range(S)] for i in range(S)]
    vxx = [[float(int(n[i][j]) * int(sxx[i][j]) - int(sx[i][j]) ** 2) for j in range(S)] for i in range(S)]
    return cxy, vxx


def pattern(matrix):
    """a matrix of floats as lists of 64-bit patterns"""
    return [[bits(float(v)) for v in row] for row in matrix]
