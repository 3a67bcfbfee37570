"""The rule of csrc/mdk_diff_core.h restated in Python floats -- the same IEEE operations in the same order, so the same bits --, the same
p-value in exact rational arithmetic, and the tables the tests of mdk.diff_counts share (test_diff_cpu.py, test_gpu_diff.py)."""
import random
import struct
from fractions import Fraction
from math import comb

LIMIT = 1 << 26
ONE, TINY, NEGLIGIBLE = 2.0 ** 60, 2.0 ** -900, 2.0 ** -64
BAR = 1.0 + 1e-7
E_NEGATIVE, E_ENTRY, E_MARGIN = 1, 2, 4
MESSAGES = {E_NEGATIVE: "a count is negative", E_ENTRY: "a count is 2^26 or more", E_MARGIN: "a pooled margin"}


def bits(x):
    """the 64-bit pattern of a double"""
    return struct.unpack("<q", struct.pack("<d", x))[0]


def entry_check(v):
    return E_NEGATIVE if v < 0 else E_ENTRY if v >= LIMIT else 0


def margin_check(a, b, c, d):
    return E_MARGIN if a + b >= LIMIT or c + d >= LIMIT or a + c >= LIMIT or b + d >= LIMIT else 0


def meth_diff(a, b, c, d):
    if a + b == 0 or c + d == 0:
        return 0.0
    fa = float(a) / float(a + b)
    fb = float(c) / float(c + d)
    x = fb - fa
    return 100.0 * x


def pvalue(a, b, c, d):
    """(p, steps): diff_pvalue of the header, statement by statement"""
    n, K, M = a + b, a + c, b + d
    lo, hi = max(0, n - M), min(n, K)
    if lo == hi:
        return 1.0, 0
    mode = min(max(((n + 1) * (K + 1)) // (n + c + d + 2), lo), hi)

    def up(r, k):
        t = r * float((K - k) * (n - k))
        return t / float((k + 1) * (M - n + k + 1))

    def down(r, k):
        t = r * float(k * (M - n + k))
        return t / float((K - k + 1) * (n - k + 1))

    k, r = mode, ONE
    while k != a:
        if a > k:
            r, k = up(r, k), k + 1
        else:
            r, k = down(r, k), k - 1
        if r < TINY:
            return 0.0, 0
    thr = r * BAR
    tail = total = 0.0
    steps = 0
    k, r = mode, ONE
    while True:
        total = total + r
        if r <= thr:
            tail = tail + r
        steps += 1
        if k == hi or (a <= k and r <= thr and r < NEGLIGIBLE * tail):
            break
        r, k = up(r, k), k + 1
    if mode > lo:
        k, r = mode - 1, down(ONE, mode)
        while True:
            total = total + r
            if r <= thr:
                tail = tail + r
            steps += 1
            if k == lo or (a >= k and r <= thr and r < NEGLIGIBLE * tail):
                break
            r, k = down(r, k), k - 1
    q = tail / total
    return (q if q < 1.0 else 1.0), steps


def exact(a, b, c, d):
    """(p, the observed table's weight over the mode's) as Fractions: every table of the margins weighed in integers, the tie rule the
    header's -- a table counts if its weight is at most the observed one's times the double 1.0 + 1e-7"""
    n, K, M = a + b, a + c, b + d
    lo, hi = max(0, n - M), min(n, K)
    bar = Fraction(BAR)
    w = comb(K, lo) * comb(M, n - lo)
    weights = [w]
    for k in range(lo, hi):
        w = w * ((K - k) * (n - k)) // ((k + 1) * (M - n + k + 1))
        weights.append(w)
    obs = weights[a - lo]
    tail = sum(x for x in weights if x * bar.denominator <= obs * bar.numerator)
    return Fraction(tail, sum(weights)), Fraction(obs, max(weights))


def expected(nmeth, nunmeth, ga, gb):
    """what mdk.diff_counts gives for count matrices (lists of rows) and two lists of sample indices: six lists"""
    out = [[], [], [], [], [], []]
    for i in range(len(nmeth[0])):
        a, b = sum(nmeth[s][i] for s in ga), sum(nunmeth[s][i] for s in ga)
        c, d = sum(nmeth[s][i] for s in gb), sum(nunmeth[s][i] for s in gb)
        for col, v in zip(out, (a, b, c, d, meth_diff(a, b, c, d), pvalue(a, b, c, d)[0])):
            col.append(v)
    return out


def seeded(seed=20261018):
    """tables (a, b, c, d): small, medium and deep cells, margins far apart, far tails, symmetric tables whose two tails tie"""
    rng = random.Random(seed)
    out = []
    for top, count in ((6, 300), (40, 400), (300, 300), (1500, 150)):
        out += [tuple(rng.randint(0, top) for _ in range(4)) for _ in range(count)]
    for _ in range(100):                                    # one group deep, one shallow; one margin small
        out.append((rng.randint(0, 1500), rng.randint(0, 1500), rng.randint(0, 12), rng.randint(0, 12)))
        out.append((rng.randint(0, 8), rng.randint(0, 1500), rng.randint(0, 8), rng.randint(0, 1500)))
    for _ in range(150):                                    # far tails: the groups nearly apart
        x, y = rng.randint(1, 1500), rng.randint(1, 1500)
        e, f = rng.randint(0, 3), rng.randint(0, 3)
        out.append((x, e, f, y) if rng.random() < 0.5 else (e, x, y, f))
    for _ in range(150):                                    # symmetric: (x, y, y, x) ties with (y, x, x, y)
        x, y = rng.randint(0, 700), rng.randint(0, 700)
        out.append((x, y, y, x))
    for _ in range(100):                                    # near the observed table of an exact tie
        x, y = rng.randint(0, 60), rng.randint(0, 60)
        out.append((x, y + rng.randint(0, 1), y, x + rng.randint(0, 1)))
    return out


# (name, table, p or None): p where it is known by hand
HAND = [
    ("tea tasting", (3, 1, 1, 3), 0.48571428571428577),
    ("symmetric tie", (7, 2, 2, 7), None),
    ("lo == hi: n = 0", (0, 0, 4, 9), 1.0),
    ("lo == hi: K = 0", (0, 6, 0, 9), 1.0),
    ("lo == hi: n = N", (5, 8, 0, 0), 1.0),
    ("lo == hi: K = N", (5, 0, 7, 0), 1.0),
    ("no coverage in A", (0, 0, 12, 30), 1.0),
    ("no coverage in B", (12, 30, 0, 0), 1.0),
    ("no coverage at all", (0, 0, 0, 0), 1.0),
    ("apart", (5000, 0, 0, 5000), 0.0),
    ("largest margins", (1, 5, LIMIT - 3, 1), None),
    ("equal groups", (20, 20, 20, 20), 1.0),
]

# (name, table, refusal bit): each just outside its bound, the rest of the table inside
REFUSED = [
    ("negative", (-1, 3, 2, 2), E_NEGATIVE),
    ("negative", (3, 2, 2, -1), E_NEGATIVE),
    ("entry", (LIMIT, 0, 0, 0), E_ENTRY),
    ("entry", (0, 0, 0, LIMIT), E_ENTRY),
    ("margin", (LIMIT - 1, 1, 0, 0), E_MARGIN),
    ("margin", (0, 0, 1, LIMIT - 1), E_MARGIN),
    ("margin", (LIMIT - 1, 0, 1, 0), E_MARGIN),
    ("margin", (0, LIMIT - 1, 0, 1), E_MARGIN),
    ("margin", (1, 1, LIMIT - 3, 5), E_MARGIN),             # c + d = 2^26 + 2
]
ACCEPTED = [(LIMIT - 1, 0, 0, 0), (LIMIT - 2, 1, 0, 0), (0, 1, LIMIT - 2, 0), (1, 5, LIMIT - 3, 1)]


def bh(p):
    """Benjamini-Hochberg on the host: descending, p * n / rank, running minimum, capped at 1; equal p-values get equal q-values"""
    n = len(p)
    order = sorted(range(n), key=lambda i: -p[i])
    q, low = [0.0] * n, 1.0
    for j, i in enumerate(order):
        rank = sum(1 for x in p if x <= p[i])               # the largest rank among the rows tied with row i
        low = min(low, p[i] * float(n) / float(rank))
        q[i] = low
    return q
