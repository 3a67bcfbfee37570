"""The rule of csrc/mdk_gdiff_core.h restated in Python floats -- the same IEEE operations in the same order, so the same bits; what it
shares with two groups is qdiff_rule's --, the same statistic in exact arithmetic, and the sites its tests use (test_gdiff_cpu.py,
test_gpu_gdiff.py).  A site is a list of groups in the order given, a group a pair (ms, us) of its samples' entries in visiting order."""
import random
from fractions import Fraction

from diff_rule import E_ENTRY, E_MARGIN, E_NEGATIVE, LIMIT, entry_check, meth_diff
from qdiff_rule import NEGLIGIBLE, PI, TINY, HUGE, qsqrt, score, term

C_STEPS, C_NU, C_CONST = 4, 12, 32                            # the error bound: (C_STEPS steps + C_NU (nu + q) + C_CONST) 2^-53
NAMES = ("meth_diff", "group_lo", "group_hi", "pvalue", "df", "df_groups", "dispersion", "statistic")


def tail(W, nu, q):
    """(p, steps): gdiff_tail of the header, statement by statement"""
    if W < TINY:
        return 1.0, 0
    if W >= HUGE:
        return 0.0, 0
    dnu, dq = float(nu), float(q)
    t = dnu + W
    x, y = dnu / t, W / t
    if q & 1:
        if nu & 1:
            B, j = PI, 1
        else:
            B, j = 2.0, 2
        while j < nu:
            B = B * float(j)
            B = B / float(j + 1)
            j += 2
        g = 1
    else:
        B = 2.0 / dnu
        g = 2
    in_tail = x * float(nu + q + 4) <= float(nu + 2)
    ended = 0.0 if in_tail else 1.0
    sx, sy = qsqrt(x), qsqrt(y)
    last = q - 2                                             # the factors of B(nu / 2, q / 2): (nu + g) / g for g, g + 2, ... up to q - 2
    pw = sx if nu & 1 else 1.0
    for _ in range(nu // 2):
        pw = pw * x
        while pw < 1.0 and g <= last:
            pw = pw * float(nu + g)
            pw = pw / float(g)
            g += 2
        if pw < TINY:
            return ended, 0
    top = pw * sy if q & 1 else pw
    for _ in range(q // 2):
        top = top * y
        while top < 1.0 and g <= last:
            top = top * float(nu + g)
            top = top / float(g)
            g += 2
        if top < TINY:
            return ended, 0
    while g <= last:
        top = top * float(nu + g)
        top = top / float(g)
        g += 2
    pre = top / ((dnu / 2.0) * B) if in_tail else top / ((dq / 2.0) * B)
    v = x if in_tail else y
    total, u, steps = 0.0, 1.0, 0
    up, down = nu + q, (nu + 2 if in_tail else q + 2)
    while True:
        total = total + u
        steps += 1
        u = u * v
        u = u * float(up)
        u = u / float(down)
        up, down = up + 2, down + 2
        if u < NEGLIGIBLE * total:
            break
    s = pre * total
    if in_tail:
        return (s if s < 1.0 else 1.0), steps
    p = 1.0 - s
    return (p if p > 0.0 else 0.0), steps


def covered(groups):
    """the indices of the groups with a covered sample, and the covered samples of these"""
    idx = [g for g, (ms, us) in enumerate(groups) if any(m + u > 0 for m, u in zip(ms, us))]
    return idx, sum(1 for g in idx for m, u in zip(*groups[g]) if m + u > 0)


def extremes(gm, gu, idx):
    """(group_lo, group_hi): the covered groups of the smallest and the largest fraction, compared in integers, a tie to the lower index"""
    if not idx:
        return -1, -1
    lo = hi = idx[0]
    for g in idx[1:]:
        if gm[g] * (gm[lo] + gu[lo]) < gm[lo] * (gm[g] + gu[g]):
            lo = g
        if gm[g] * (gm[hi] + gu[hi]) > gm[hi] * (gm[g] + gu[g]):
            hi = g
    return lo, hi


def site(groups, min_dispersion=1.0):
    """(the groups' pooled nmeth, their nunmeth, the eight columns of NAMES as a tuple, steps) of a site, its entries checked elsewhere"""
    gm, gu = [sum(ms) for ms, _ in groups], [sum(us) for _, us in groups]
    idx, k = covered(groups)
    q, nu = len(idx) - 1, k - max(len(idx), 2)               # (fewer than two covered groups: nothing to test, and df is diff_replicates' there)
    lo, hi = extremes(gm, gu, idx)
    diff = meth_diff(gm[lo], gu[lo], gm[hi], gu[hi]) if idx else 0.0
    K, M = sum(gm), sum(gu)
    N = K + M
    if len(idx) < 2 or nu < 1 or K == 0 or M == 0:
        return gm, gu, (diff, lo, hi, 1.0, max(nu, 0), max(q, 0), 1.0, 0.0), 0
    if len(idx) == 2:
        X = score(gm[idx[0]], gu[idx[0]], gm[idx[1]], gu[idx[1]])
    else:
        X = 0.0
        for g in idx:
            e = gm[g] * N - (gm[g] + gu[g]) * K
            ee = float(e) * float(e)
            den = float(gm[g] + gu[g]) * float(K * M)
            X = X + ee / den
    pearson = 0.0
    for g in idx:
        if gm[g] > 0 and gu[g] > 0:
            for m, u in zip(*groups[g]):
                if m + u > 0:
                    pearson = pearson + term(m, u, gm[g], gu[g])
    phi = pearson / float(nu)
    if phi < min_dispersion:
        phi = min_dispersion
    W = X / phi
    p, steps = tail(W, nu, q)
    return gm, gu, (diff, lo, hi, p, nu, q, phi, W / float(q)), steps


def refusal(groups):
    """the DIFF_E_* bits of a site: its entries, then a group's depth, the methylated or the unmethylated of all"""
    err = 0
    for ms, us in groups:
        for v in list(ms) + list(us):
            err |= entry_check(v)
    if err:
        return err
    gm, gu = [sum(ms) for ms, _ in groups], [sum(us) for _, us in groups]
    return E_MARGIN if any(m + u >= LIMIT for m, u in zip(gm, gu)) or sum(gm) >= LIMIT or sum(gu) >= LIMIT else 0


def exact_statistic(groups, min_dispersion=1.0):
    """(X, phi, W, nu, q) of a site that is not degenerate, as Fractions"""
    idx, k = covered(groups)
    q, nu = len(idx) - 1, k - len(idx)
    gm, gu = [sum(ms) for ms, _ in groups], [sum(us) for _, us in groups]
    K, M = sum(gm), sum(gu)
    N = K + M
    X = sum(Fraction((gm[g] * N - (gm[g] + gu[g]) * K) ** 2, (gm[g] + gu[g]) * K * M) for g in idx)
    pearson = Fraction(0)
    for g in idx:
        if gm[g] > 0 and gu[g] > 0:
            for m, u in zip(*groups[g]):
                if m + u > 0:
                    pearson += Fraction((m * (gm[g] + gu[g]) - (m + u) * gm[g]) ** 2, (m + u) * gm[g] * gu[g])
    phi = max(pearson / nu, Fraction(min_dispersion))
    return X, phi, X / phi, nu, q


def seeded(seed=20261020, per_shape=160):
    """sites of G = 2, 3, 4, 5, 8 and 17 groups of 1 to 6 samples each (1,024 at the most), depths 0 to 40, a tenth of the entries uncovered,
    now and then a group all methylated or all unmethylated, now and then a whole group uncovered"""
    rng = random.Random(seed)
    out = []
    for G in (2, 3, 4, 5, 8, 17):
        for _ in range(per_shape):
            groups = []
            for _ in range(G):
                size = rng.randint(1, 6)
                frac = rng.choice((0.0, 1.0)) if rng.random() < 0.08 else rng.random()
                gone = rng.random() < 0.06
                ms, us = [], []
                for _ in range(size):
                    n = 0 if gone or rng.random() < 0.1 else rng.randint(0, 40)
                    f = min(1.0, max(0.0, frac + rng.uniform(-0.15, 0.15))) if 0.0 < frac < 1.0 else frac
                    k = sum(1 for _ in range(n) if rng.random() < f)
                    ms.append(k); us.append(n - k)
                groups.append((ms, us))
            out.append(groups)
    return out


def null_sites(count=4000, groups=3, replicates=3, rho=0.2, depth=30, fraction=0.6, seed=20261020):
    """sites without a difference, `groups` groups of `replicates` replicates, made as qdiff_rule.null_sites makes its own: every
    replicate's fraction a beta draw of mean `fraction` and intra-class correlation rho, its depth uniform in depth +- 10, its
    methylated count binomial"""
    rng = random.Random(seed)
    al, be = fraction * (1.0 - rho) / rho, (1.0 - fraction) * (1.0 - rho) / rho
    out = []
    for _ in range(count):
        site_groups = []
        for _ in range(groups):
            ms, us = [], []
            for _ in range(replicates):
                n = rng.randint(depth - 10, depth + 10)
                f = rng.betavariate(al, be)
                k = sum(1 for _ in range(n) if rng.random() < f)
                ms.append(k); us.append(n - k)
            site_groups.append((ms, us))
        out.append(site_groups)
    return out


def two(s):
    """a site of qdiff_rule, (ma, ua, mb, ub), as two groups"""
    return [(list(s[0]), list(s[1])), (list(s[2]), list(s[3]))]


DEGENERATE = {"pvalue": 1.0, "dispersion": 1.0, "statistic": 0.0}
# (name, site, what is known by hand: a dict of column -> value)
HAND = [
    ("one sample a group: nu = 0", [([5], [3]), ([2], [7]), ([4], [4])], dict(DEGENERATE, df=0, df_groups=2, group_lo=1, group_hi=0)),
    ("nothing covered", [([0, 0], [0, 0]), ([0], [0]), ([0], [0])], dict(DEGENERATE, df=0, df_groups=0, group_lo=-1, group_hi=-1, meth_diff=0.0)),
    ("one group covered", [([0], [0]), ([3, 4], [5, 6]), ([0, 0], [0, 0])], dict(DEGENERATE, df=0, df_groups=0, group_lo=1, group_hi=1, meth_diff=0.0)),
    ("K == 0", [([0, 0], [6, 4]), ([0, 0], [9, 5]), ([0, 0], [2, 2])], dict(DEGENERATE, df=3, df_groups=2, group_lo=0, group_hi=0, meth_diff=0.0)),
    ("M == 0", [([6, 4], [0, 0]), ([9, 5], [0, 0]), ([2, 2], [0, 0])], dict(DEGENERATE, df=3, df_groups=2, group_lo=0, group_hi=0, meth_diff=0.0)),
    ("no difference", [([5, 5], [5, 5])] * 3, {"pvalue": 1.0, "statistic": 0.0, "dispersion": 1.0, "df": 3, "df_groups": 2, "group_lo": 0, "group_hi": 0, "meth_diff": 0.0}),
    ("identical replicates", [([6, 6], [4, 4]), ([3, 3], [7, 7]), ([5, 5], [5, 5])], {"df": 3, "df_groups": 2, "dispersion": 1.0, "group_lo": 1, "group_hi": 0, "meth_diff": 30.0}),
    ("the middle group uncovered", [([6, 5, 7], [4, 6, 4]), ([0, 0], [0, 0]), ([3, 2, 4], [7, 9, 5])], {"df": 4, "df_groups": 1, "group_lo": 2, "group_hi": 0}),
    ("ties go to the lower group", [([2, 2], [6, 6]), ([1, 1], [1, 1]), ([1, 3], [3, 9]), ([5, 1], [5, 1])], {"group_lo": 0, "group_hi": 1, "meth_diff": 25.0, "df": 4, "df_groups": 3}),
    ("parity: q = 2, nu = 3", [([6, 5], [4, 6]), ([3, 2], [7, 9]), ([4, 8], [5, 3])], {"df": 3, "df_groups": 2}),
    ("parity: q = 3, nu = 4", [([6, 5], [4, 6]), ([3, 2], [7, 9]), ([4, 8], [5, 3]), ([1, 9], [9, 2])], {"df": 4, "df_groups": 3}),
    ("parity: q = 2, nu = 4", [([6, 5, 2], [4, 6, 2]), ([3, 2], [7, 9]), ([4, 8], [5, 3])], {"df": 4, "df_groups": 2}),
    # x is about 2^-20 and x^59 far below 2^-940; 1 / B(59, 1) is 59
    ("huge W", [([1000000] * 40, [0] * 40), ([0] * 40, [1000000] * 40), ([500000] * 41, [500000] * 41)], {"pvalue": 0.0, "df": 118, "df_groups": 2, "dispersion": 1.0, "group_lo": 1, "group_hi": 0, "meth_diff": 100.0}),
]

# (name, site, refusal bit): each just outside its bound
REFUSED = [
    ("negative", [([3, -1], [2, 2]), ([2, 2], [1, 1]), ([1], [1])], E_NEGATIVE),
    ("negative", [([3, 1], [2, 2]), ([2, 2], [1, 1]), ([1], [-1])], E_NEGATIVE),
    ("entry", [([LIMIT, 1], [0, 0]), ([1, 1], [1, 1]), ([1], [1])], E_ENTRY),
    ("entry", [([1, 1], [0, 0]), ([1, 1], [1, 1]), ([1], [LIMIT])], E_ENTRY),
    ("a group's depth", [([1, 1], [1, 1]), ([LIMIT // 2, LIMIT // 4], [0, LIMIT // 4]), ([1], [1])], E_MARGIN),
    ("the methylated of all", [([LIMIT // 2, 1], [0, 0]), ([LIMIT // 4, 1], [1, 1]), ([LIMIT // 4 - 2], [1])], E_MARGIN),
    ("the unmethylated of all", [([1, 1], [2, 2]), ([3, 3], [LIMIT // 2 - 4, 0]), ([0], [LIMIT // 2])], E_MARGIN),
    ("an entry before a margin", [([LIMIT - 1, LIMIT - 1], [0, 0]), ([1, LIMIT], [1, 1]), ([1], [1])], E_ENTRY),
]
ACCEPTED = [
    [([LIMIT // 2 - 1, LIMIT // 2 - 2], [0, 1]), ([0, 0], [1, 1]), ([0], [1])],                      # a group's depth 2^26 - 2
    [([LIMIT // 2, 0], [0, 0]), ([LIMIT // 4, 1], [1, 1]), ([LIMIT // 4 - 3], [1])],               # K = 2^26 - 2
    [([1, 1], [2, 2]), ([3, 3], [LIMIT // 2 - 5, 0]), ([0], [LIMIT // 2])],                        # M = 2^26 - 1
]
