"""The rule of csrc/mdk_qdiff_core.h restated in Python floats -- the same IEEE operations in the same order, so the same bits (math.frexp
and math.ldexp are exact; nothing else of math is used) --, the same test in exact arithmetic, and the sites its test uses
(test_qdiff_cpu.py)."""
import random
from fractions import Fraction
from math import frexp, ldexp

from diff_rule import E_ENTRY, E_MARGIN, E_NEGATIVE, LIMIT, entry_check, margin_check, meth_diff

TINY, HUGE, NEGLIGIBLE = 2.0 ** -940, 2.0 ** 1000, 2.0 ** -64
PI = float.fromhex("0x1.921fb54442d18p+1")
SQRT_STEPS = 5
C_STEPS, C_NU, C_CONST = 4, 12, 32                            # the error bound: (C_STEPS steps + C_NU nu + C_CONST) 2^-53
NAMES = ("nmeth_a", "nunmeth_a", "nmeth_b", "nunmeth_b", "meth_diff", "pvalue", "df", "dispersion", "statistic")


def qsqrt(v):
    m, e = frexp(v)                                          # v = m 2^e, m in [0.5, 1): v = (2 m) 2^(e - 1)
    E = e - 1
    if E & 1:
        f, h = m, (E + 1) // 2
    else:
        f, h = ldexp(m, 1), E // 2
    r = 0.5 * f
    r = r + 0.5
    for _ in range(SQRT_STEPS):
        q = f / r
        r = 0.5 * (r + q)
    return ldexp(r, h)


def score(a, b, c, d):
    det = a * d - b * c
    dd = float(det) * float(det)
    num = dd * float(a + b + c + d)
    den = float((a + b) * (c + d)) * float((a + c) * (b + d))
    return num / den


def term(m, u, gm, gu):
    e = m * (gm + gu) - (m + u) * gm
    ee = float(e) * float(e)
    den = float(m + u) * float(gm * gu)
    return ee / den


def tail(F, nu):
    """(p, steps): qdiff_tail of the header, statement by statement"""
    if F < TINY:
        return 1.0, 0
    if F >= HUGE:
        return 0.0, 0
    dnu = float(nu)
    t = dnu + F
    x, y = dnu / t, F / t
    if nu & 1:
        B, j = PI, 1
    else:
        B, j = 2.0, 2
    while j < nu:
        B = B * float(j)
        B = B / float(j + 1)
        j += 2
    sx, sy = qsqrt(x), qsqrt(y)
    pw = sx if nu & 1 else 1.0
    for _ in range(nu // 2):
        pw = pw * x
        if pw < TINY:
            return 0.0, 0
    top = pw * sy
    in_tail = x * float(nu + 5) <= float(nu + 2)
    pre = top / ((dnu / 2.0) * B) if in_tail else top / (0.5 * B)
    v = x if in_tail else y
    total, u, steps = 0.0, 1.0, 0
    up, down = nu + 1, (nu + 2 if in_tail else 3)
    while True:
        total = total + u
        steps += 1
        u = u * v
        u = u * float(up)
        u = u / float(down)
        up, down = up + 2, down + 2
        if u < NEGLIGIBLE * total:
            break
    q = pre * total
    if in_tail:
        return (q if q < 1.0 else 1.0), steps
    p = 1.0 - q
    return (p if p > 0.0 else 0.0), steps


def pool(ma, ua, mb, ub):
    """a site's pooled counts, covered samples and Pearson's sum from its entries, group A's and group B's: (a, b, c, d, ka, kb, pearson)"""
    a, b, c, d = sum(ma), sum(ua), sum(mb), sum(ub)
    ka, kb = sum(1 for m, u in zip(ma, ua) if m + u > 0), sum(1 for m, u in zip(mb, ub) if m + u > 0)
    pearson = 0.0
    for ms, us, gm, gu in ((ma, ua, a, b), (mb, ub, c, d)):
        if gm > 0 and gu > 0:
            for m, u in zip(ms, us):
                if m + u > 0:
                    pearson = pearson + term(m, u, gm, gu)
    return a, b, c, d, ka, kb, pearson


def site(ma, ua, mb, ub, min_dispersion=1.0):
    """(the nine columns of a site as a tuple in NAMES' order, steps) from its entries, checked elsewhere"""
    a, b, c, d, ka, kb, pearson = pool(ma, ua, mb, ub)
    nu = ka + kb - 2
    head = (a, b, c, d, meth_diff(a, b, c, d))
    if ka == 0 or kb == 0 or nu < 1 or a + c == 0 or b + d == 0:
        return head + (1.0, max(nu, 0), 1.0, 0.0), 0
    phi = pearson / float(nu)
    if phi < min_dispersion:
        phi = min_dispersion
    F = score(a, b, c, d) / phi
    p, steps = tail(F, nu)
    return head + (p, nu, phi, F), steps


def refusal(ma, ua, mb, ub):
    """the DIFF_E_* bits of a site: its entries, then its margins"""
    err = 0
    for v in list(ma) + list(ua) + list(mb) + list(ub):
        err |= entry_check(v)
    return err or margin_check(sum(ma), sum(ua), sum(mb), sum(ub))


def exact_statistic(ma, ua, mb, ub, min_dispersion=1.0):
    """(X, phi, F, nu) of a site that is not degenerate, as Fractions"""
    a, b, c, d = sum(ma), sum(ua), sum(mb), sum(ub)
    pairs = [(ms, us, gm, gu) for ms, us, gm, gu in ((ma, ua, a, b), (mb, ub, c, d))]
    nu = sum(1 for ms, us, _, _ in pairs for m, u in zip(ms, us) if m + u > 0) - 2
    X = Fraction((a * d - b * c) ** 2 * (a + b + c + d), (a + b) * (c + d) * (a + c) * (b + d))
    pearson = Fraction(0)
    for ms, us, gm, gu in pairs:
        if gm > 0 and gu > 0:
            for m, u in zip(ms, us):
                if m + u > 0:
                    pearson += Fraction((m * (gm + gu) - (m + u) * gm) ** 2, (m + u) * gm * gu)
    phi = max(pearson / nu, Fraction(min_dispersion))
    return X, phi, X / phi, nu


def seeded(seed=20261019, per_shape=420):
    """sites (ma, ua, mb, ub): S of 3, 4, 5, 7 and 12 samples split in two groups, depths 0 to 40, a tenth of the entries uncovered,
    now and then a group all methylated or all unmethylated"""
    rng = random.Random(seed)
    out = []
    for S in (3, 4, 5, 7, 12):
        for _ in range(per_shape):
            na = rng.randint(1, S - 1)
            frac = [rng.choice((0.0, 1.0)) if rng.random() < 0.08 else rng.random() for _ in range(2)]
            m, u = [], []
            for s in range(S):
                n = 0 if rng.random() < 0.1 else rng.randint(0, 40)
                f = min(1.0, max(0.0, frac[s >= na] + rng.uniform(-0.15, 0.15))) if 0.0 < frac[s >= na] < 1.0 else frac[s >= na]
                k = sum(1 for _ in range(n) if rng.random() < f)
                m.append(k); u.append(n - k)
            out.append((m[:na], u[:na], m[na:], u[na:]))
    return out


def null_sites(count=4000, rho=0.2, depth=30, fraction=0.6, seed=20261019):
    """sites without a difference, three replicates against three: every replicate's own fraction is a beta draw of mean `fraction` and
    intra-class correlation rho, its depth uniform in depth +- 10, its methylated count binomial"""
    rng = random.Random(seed)
    al, be = fraction * (1.0 - rho) / rho, (1.0 - fraction) * (1.0 - rho) / rho
    out = []
    for _ in range(count):
        m, u = [], []
        for _ in range(6):
            n = rng.randint(depth - 10, depth + 10)
            f = rng.betavariate(al, be)
            k = sum(1 for _ in range(n) if rng.random() < f)
            m.append(k); u.append(n - k)
        out.append((m[:3], u[:3], m[3:], u[3:]))
    return out


# (name, (ma, ua, mb, ub), what is known by hand: a dict of column -> value)
HAND = [
    ("nu < 1: one sample a group", ([5], [3], [2], [7]), {"pvalue": 1.0, "df": 0, "dispersion": 1.0, "statistic": 0.0}),
    ("nu < 1: an uncovered sample leaves two", ([5, 0], [3, 0], [2], [7]), {"pvalue": 1.0, "df": 0, "dispersion": 1.0, "statistic": 0.0}),
    ("group A without coverage", ([0, 0], [0, 0], [4, 6, 5], [9, 3, 5]), {"pvalue": 1.0, "df": 1, "dispersion": 1.0, "statistic": 0.0, "meth_diff": 0.0}),
    ("group B without coverage", ([4, 6, 5], [9, 3, 5], [0], [0]), {"pvalue": 1.0, "df": 1, "dispersion": 1.0, "statistic": 0.0, "meth_diff": 0.0}),
    ("K == 0", ([0, 0], [6, 4], [0, 0], [9, 5]), {"pvalue": 1.0, "df": 2, "dispersion": 1.0, "statistic": 0.0}),
    ("M == 0", ([6, 4], [0, 0], [9, 5], [0, 0]), {"pvalue": 1.0, "df": 2, "dispersion": 1.0, "statistic": 0.0}),
    ("identical replicates", ([6, 6, 6], [4, 4, 4], [3, 3, 3], [7, 7, 7]), {"df": 4, "dispersion": 1.0}),
    ("parity: all covered, nu = 4", ([6, 5, 7], [4, 6, 4], [3, 2, 4], [7, 9, 5]), {"df": 4}),
    ("parity: one uncovered, nu = 3", ([6, 5, 0], [4, 6, 0], [3, 2, 4], [7, 9, 5]), {"df": 3}),
    # X = N = 1.2e8 and nu = 118: x is about 2^-20 and x^59 far below 2^-940
    ("huge F", ([1000000] * 60, [0] * 60, [0] * 60, [1000000] * 60), {"pvalue": 0.0, "df": 118, "dispersion": 1.0}),
    ("no difference", ([5, 5], [5, 5], [5, 5], [5, 5]), {"pvalue": 1.0, "df": 2, "statistic": 0.0, "dispersion": 1.0}),
]

# (name, site, refusal bit): each just outside its bound
REFUSED = [
    ("negative", ([3, -1], [2, 2], [2, 2], [1, 1]), E_NEGATIVE),
    ("negative", ([3, 1], [2, 2], [2, 2], [1, -1]), E_NEGATIVE),
    ("entry", ([LIMIT, 1], [0, 0], [1, 1], [1, 1]), E_ENTRY),
    ("entry", ([1, 1], [0, 0], [1, 1], [1, LIMIT]), E_ENTRY),
    ("margin", ([LIMIT // 2, LIMIT // 2], [0, 0], [1, 1], [1, 1]), E_MARGIN),
    ("margin", ([1, 1], [2, 2], [3, 3], [LIMIT // 2 - 1, LIMIT // 2]), E_MARGIN),
]
ACCEPTED = [([LIMIT // 2 - 1, LIMIT // 2 - 2], [0, 1], [1, 1], [1, 1]), ([LIMIT - 3, 0], [0, 0], [0, 1], [1, 0])]
