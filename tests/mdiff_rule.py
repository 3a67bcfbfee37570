"""The rule of csrc/mdk_mdiff_core.h restated in Python floats -- the same IEEE operations in the same order, so the same bits; the tail
is gdiff_rule's --, the same estimator in mpmath, and the sites its tests use (test_mdiff_cpu.py, test_gpu_mdiff.py).  A site is (ms, us,
X, q): the used samples' entries in visiting order, their design rows -- the reduced columns first, then the q tested ones --, and q."""
import random

from diff_rule import E_ENTRY, E_MARGIN, E_NEGATIVE, LIMIT, entry_check
from gdiff_rule import tail
from qdiff_rule import qsqrt

MAX_COLUMNS, MAX_PASSES = 8, 40
RANK, NUMERIC, REDUCED, FULL = 1, 2, 4, 8
C_STEPS, C_NU, C_FIT, C_CONST, C_TOL = 4, 12, 16, 32, 1
ETA_MAX, STEP_MAX, CONVERGED, RANK_PIVOT, NORMAL = 40.0, 4.0, 2.0 ** -40, 2.0 ** -26, 2.0 ** -1022
INV_LN2, LN2_HI, LN2_LO = float.fromhex("0x1.71547652b82fep+0"), float.fromhex("0x1.62e42fee00000p-1"), float.fromhex("0x1.a39ef35793c76p-33")
EXP_C = [float.fromhex(h) for h in ("0x1.0000000000000p+0", "0x1.0000000000000p+0", "0x1.0000000000000p-1", "0x1.5555555555555p-3", "0x1.5555555555555p-5",
                                    "0x1.1111111111111p-7", "0x1.6c16c16c16c17p-10", "0x1.a01a01a01a01ap-13", "0x1.a01a01a01a01ap-16", "0x1.71de3a556c734p-19",
                                    "0x1.27e4fb7789f5cp-22", "0x1.ae64567f544e4p-26", "0x1.1eed8eff8d898p-29", "0x1.6124613a86d09p-33")]
NAMES = ("pvalue", "df", "dispersion", "statistic", "flags", "iterations")


def bound(steps, nu, q, k, p):
    """the header's error bound, as a relative error"""
    return (C_STEPS * steps + (nu + q) * (C_NU + C_FIT * k * p) + C_CONST) * 2.0 ** -53 + C_TOL * (nu + q) * 2.0 ** -42


def exp(t):
    """mdiff_exp of the header, statement by statement: e^t, t in [-40, 0]"""
    z = t * INV_LN2
    kk = -int(-z + 0.5)
    dk = float(kk)
    rr = (t - dk * LN2_HI) - dk * LN2_LO
    s = EXP_C[13]
    for j in range(12, -1, -1):
        s = s * rr + EXP_C[j]
    return s * 2.0 ** kk


def a_pass(rows, beta, c):
    """(g, A as a list of rows of the lower triangle, pearson) at beta over the first c columns; rows: (m, u, x) of the covered samples"""
    g = [0.0] * c
    A = [[0.0] * (a + 1) for a in range(c)]
    pearson = 0.0
    for m, u, x in rows:
        eta = 0.0
        for a in range(c):
            eta = eta + x[a] * beta[a]
        if eta > ETA_MAX:
            eta = ETA_MAX
        if eta < -ETA_MAX:
            eta = -ETA_MAX
        e = exp(eta if eta < 0.0 else -eta)
        ope = 1.0 + e
        mu = 1.0 / ope if eta >= 0.0 else e / ope
        v = e / (ope * ope)
        dn = float(m + u)
        w = dn * v
        res = float(m) - dn * mu
        pearson = pearson + (res * res) / w
        for a in range(c):
            g[a] = g[a] + x[a] * res
            for b in range(a + 1):
                A[a][b] = A[a][b] + (x[a] * x[b]) * w
    return g, A, pearson


def cholesky(A, rel):
    """A's lower triangle made L in place; False: a pivot is not above rel times its diagonal entry, or is no normal double"""
    c = len(A)
    for j in range(c):
        diag = A[j][j]
        s = diag
        for k in range(j):
            s = s - A[j][k] * A[j][k]
        if not s > rel * diag or not s >= NORMAL:
            return False
        l = qsqrt(s)
        A[j][j] = l
        for i in range(j + 1, c):
            v = A[i][j]
            for k in range(j):
                v = v - A[i][k] * A[j][k]
            A[i][j] = v / l
    return True


def solve(L, g):
    c = len(L)
    d = [0.0] * c
    for i in range(c):
        s = g[i]
        for k in range(i):
            s = s - L[i][k] * d[k]
        d[i] = s / L[i][i]
    for i in range(c - 1, -1, -1):
        s = d[i]
        for k in range(i + 1, c):
            s = s - L[k][i] * d[k]
        d[i] = s / L[i][i]
    return d


def fit(rows, beta, c):
    """Newton over the first c columns from beta, in place: (NUMERIC or 0, the first decrement, converged, the passes made)"""
    first = 0.0
    for it in range(MAX_PASSES):
        g, A, _ = a_pass(rows, beta, c)
        if not cholesky(A, 0.0):
            return NUMERIC, first, False, it + 1
        d = solve(A, g)
        dec = 0.0
        for a in range(c):
            dec = dec + g[a] * d[a]
        if it == 0:
            first = dec
        t = 0.0
        for _, _, x in rows:
            h = 0.0
            for a in range(c):
                h = h + x[a] * d[a]
            if h < 0.0:
                h = -h
            if h > t:
                t = h
        if t > STEP_MAX:
            sc = STEP_MAX / t
            for a in range(c):
                d[a] = d[a] * sc
        for a in range(c):
            beta[a] = beta[a] + d[a]
        if dec <= CONVERGED:
            return 0, first, True, it + 1
    return 0, first, False, MAX_PASSES


def site(ms, us, X, q, min_dispersion=1.0):
    """(K, M, the coefficients, the six columns of NAMES as a tuple, steps) of a site, its entries checked elsewhere"""
    p = len(X[0])
    r = p - q
    rows = [(m, u, x) for m, u, x in zip(ms, us, X) if m + u > 0]
    K, M = sum(ms), sum(us)
    nu = len(rows) - p
    zero = [0.0] * p
    if nu < 1 or K == 0 or M == 0:
        return K, M, zero, (1.0, max(nu, 0), 1.0, 0.0, 0, 0), 0
    _, A, _ = a_pass(rows, zero, p)
    if not cholesky(A, RANK_PIVOT):
        return K, M, zero, (1.0, 0, 1.0, 0.0, RANK, 0), 0
    beta = [0.0] * p
    failed, _, converged, passes = fit(rows, beta, r)
    if failed:
        return K, M, zero, (1.0, nu, 1.0, 0.0, failed, passes), 0
    flags = 0 if converged else REDUCED
    failed, X0, converged, more = fit(rows, beta, p)
    passes += more
    if failed:
        return K, M, zero, (1.0, nu, 1.0, 0.0, flags | failed, passes), 0
    if not converged:
        flags |= FULL
    if not X0 > 0.0:
        X0 = 0.0
    _, _, pearson = a_pass(rows, beta, p)
    phi = pearson / float(nu)
    if phi < min_dispersion:
        phi = min_dispersion
    W = X0 / phi
    pv, steps = tail(W, nu, q)
    return K, M, beta, (pv, nu, phi, W / float(q), flags, passes), steps


def refusal(ms, us):
    """the DIFF_E_* bits of a site: its entries, then the methylated or the unmethylated of all"""
    err = 0
    for v in list(ms) + list(us):
        err |= entry_check(v)
    if err:
        return err
    return E_MARGIN if sum(ms) >= LIMIT or sum(us) >= LIMIT else 0


def independent(X):
    """the host's test of a design over all its rows: the rank test on the unweighted Gram matrix"""
    p = len(X[0])
    A = [[0.0] * (a + 1) for a in range(p)]
    for x in X:
        for a in range(p):
            for b in range(a + 1):
                A[a][b] = A[a][b] + x[a] * x[b]
    return cholesky(A, RANK_PIVOT)


def exact(ms, us, X, q, min_dispersion=1.0, digits=50):
    """(p, phi, statistic) of a site that is not degenerate by the same estimator in mpmath at `digits` digits: Newton with the step's cap
    until the decrement is below 1e-22, one step from where the other directions are exact to 1e-44; the linear predictor is clamped
    to +- 60, so a SEPARATED fit ends there, its separated samples' residuals and weights below n e^-60 = 1e-24 of the limit's 0.  The
    score statistic at the reduced fit, Pearson's sum at the full one, the tail from betainc"""
    import mpmath as mp
    with mp.workdps(digits):
        p = len(X[0])
        r = p - q
        rows = [(mp.mpf(m), mp.mpf(m + u), [mp.mpf(v) for v in x]) for m, u, x in zip(ms, us, X) if m + u > 0]
        nu = len(rows) - p

        def moments(beta, c):
            g = mp.matrix(c, 1)
            A = mp.matrix(c, c)
            pearson = mp.mpf(0)
            for m, n, x in rows:
                eta = max(mp.mpf(-60), min(mp.mpf(60), sum(x[a] * beta[a] for a in range(c))))
                mu = 1 / (1 + mp.exp(-eta))
                w = n * mu * (1 - mu)
                res = m - n * mu
                pearson += res * res / w
                for a in range(c):
                    g[a] += x[a] * res
                    for b in range(c):
                        A[a, b] += x[a] * x[b] * w
            return g, A, pearson

        def newton(beta, c):
            first = None
            for it in range(600):
                g, A, _ = moments(beta, c)
                d = mp.lu_solve(A, g)
                dec = sum(g[a] * d[a] for a in range(c))
                if first is None:
                    first = dec
                t = max(abs(sum(x[a] * d[a] for a in range(c))) for _, _, x in rows)
                if t > 4:
                    d = d * (4 / t)
                for a in range(c):
                    beta[a] += d[a]
                if dec < mp.mpf(10) ** -22:
                    return first
            raise AssertionError("the exact fit did not converge")

        beta = [mp.mpf(0)] * p
        newton(beta, r)
        X0 = newton(beta, p)
        _, _, pearson = moments(beta, p)
        phi = max(pearson / nu, mp.mpf(min_dispersion))
        W = X0 / phi
        return mp.betainc(mp.mpf(nu) / 2, mp.mpf(q) / 2, 0, mp.mpf(nu) / (mp.mpf(nu) + W), regularized=True), phi, W / q


def design_of(rng, S, p, continuous=True):
    """a design of S rows: an intercept, then columns of several kinds -- a two-level factor, a batch dummy, a continuous variable --,
    drawn again until its columns are independent"""
    while True:
        X = []
        kinds = [rng.choice(("factor", "batch", "continuous") if continuous else ("factor", "batch")) for _ in range(p - 1)]
        if continuous and "continuous" not in kinds:
            kinds[rng.randrange(p - 1)] = "continuous"
        cols = []
        for kind in kinds:
            if kind == "factor":
                cols.append([float(s % 2 == 0) if rng.random() < 0.5 else float(rng.random() < 0.5) for s in range(S)])
            elif kind == "batch":
                cut = rng.randint(1, S - 1)
                cols.append([float(s >= cut) for s in range(S)])
            else:
                cols.append([round(rng.uniform(-2.0, 2.0), 3) for _ in range(S)])
        X = [[1.0] + [c[s] for c in cols] for s in range(S)]
        if independent(X):
            return X


def seeded(seed=20261021, per_shape=14, continuous=True):
    """sites of S = 5 .. 12 samples and p = 2 .. 8 columns (p < S), q from 1 to p - 1, depths 1 to 40, a tenth of the entries uncovered,
    now and then the samples of a factor's level all methylated or all unmethylated"""
    rng = random.Random(seed)
    out = []
    for S in range(5, 13):
        for p in range(2, 9):
            if p >= S:
                continue
            for _ in range(per_shape):
                X = design_of(rng, S, p, continuous)
                q = rng.randint(1, p - 1)
                beta = [rng.uniform(-1.0, 1.0)] + [rng.uniform(-0.8, 0.8) for _ in range(p - 1)]
                extreme = rng.random() < 0.1
                side = rng.choice((0.0, 1.0))
                ms, us = [], []
                for s in range(S):
                    n = 0 if rng.random() < 0.1 else rng.randint(1, 40)
                    eta = sum(x * b for x, b in zip(X[s], beta)) + rng.gauss(0.0, 0.4)
                    f = 1.0 / (1.0 + 2.718281828459045 ** -eta)
                    if extreme and X[s][p - 1] == 1.0:
                        f = side
                    k = sum(1 for _ in range(n) if rng.random() < f)
                    ms.append(k); us.append(n - k)
                out.append((ms, us, X, q))
    return out


def dummies(groups):
    """a site of gdiff_rule (a list of groups (ms, us)) as a site of this rule: an intercept and a dummy for every group but the first, the
    dummies tested"""
    G = len(groups)
    ms, us, X = [], [], []
    for g, (gm, gu) in enumerate(groups):
        for m, u in zip(gm, gu):
            ms.append(m); us.append(u)
            X.append([1.0] + [float(g == j) for j in range(1, G)])
    return ms, us, X, G - 1


def paired_null_sites(count=4000, pairs=6, rho=0.2, depth=30, fraction=0.6, patient_sd=1.0, seed=20261021):
    """sites without a group effect, `pairs` patients with a sample in either group, made in gdiff_rule.null_sites' manner with a patient
    effect: every patient's logit is that of `fraction` plus a normal draw of standard deviation `patient_sd`, every sample's fraction a
    beta draw of that mean and intra-class correlation rho, its depth uniform in depth +- 10, its methylated count binomial.  The
    design: an intercept, a dummy for every patient but the first, and the group, which is tested"""
    import math
    rng = random.Random(seed)
    X = [[1.0] + [float(s // 2 == j) for j in range(1, pairs)] + [float(s % 2)] for s in range(2 * pairs)]
    base = math.log(fraction / (1.0 - fraction))
    out = []
    for _ in range(count):
        ms, us = [], []
        for pair in range(pairs):
            mean = 1.0 / (1.0 + math.exp(-(base + rng.gauss(0.0, patient_sd))))
            al, be = mean * (1.0 - rho) / rho, (1.0 - mean) * (1.0 - rho) / rho
            for _ in range(2):
                n = rng.randint(depth - 10, depth + 10)
                f = rng.betavariate(al, be)
                k = sum(1 for _ in range(n) if rng.random() < f)
                ms.append(k); us.append(n - k)
        out.append((ms, us, X, 1))
    return out


BIG = 1 << 22
PLAIN = [[1.0, 0.0], [1.0, 0.0], [1.0, 0.0], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0]]
BATCH = [[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0], [1.0, 0.0, 1.0]]           # (intercept, a batch of one sample, the group)
DEGENERATE = {"pvalue": 1.0, "dispersion": 1.0, "statistic": 0.0, "flags": 0, "iterations": 0}
# (name, site, what is known by hand: a dict of column -> value)
HAND = [
    ("nu = 0", ([5, 2], [3, 7], [[1.0, 0.0], [1.0, 1.0]], 1), dict(DEGENERATE, df=0)),
    ("nu below 0", ([5, 0, 0], [3, 0, 0], [[1.0, 0.0], [1.0, 1.0], [1.0, 1.0]], 1), dict(DEGENERATE, df=0)),
    ("nothing covered", ([0] * 6, [0] * 6, PLAIN, 1), dict(DEGENERATE, df=0)),
    ("K == 0", ([0] * 6, [6, 4, 9, 5, 2, 2], PLAIN, 1), dict(DEGENERATE, df=4)),
    ("M == 0", ([6, 4, 9, 5, 2, 2], [0] * 6, PLAIN, 1), dict(DEGENERATE, df=4)),
    ("no difference", ([5] * 6, [5] * 6, PLAIN, 1), {"pvalue": 1.0, "statistic": 0.0, "dispersion": 1.0, "df": 4, "flags": 0}),
    ("two groups", ([6, 5, 7, 3, 2, 4], [4, 6, 4, 7, 9, 5], PLAIN, 1), {"df": 4, "flags": 0}),
    ("a group all methylated", ([6, 5, 7, 3, 2, 4], [0, 0, 0, 7, 9, 5], PLAIN, 1), {"df": 4, "flags": 0}),
    # the batch column's only sample has no coverage: the column is empty at the site
    ("a batch whose only sample is uncovered", ([6, 5, 7, 3, 0, 4], [4, 6, 4, 7, 0, 5], BATCH, 1), {"pvalue": 1.0, "dispersion": 1.0, "statistic": 0.0, "df": 0, "flags": RANK, "iterations": 0}),
    ("the same batch covered", ([6, 5, 7, 3, 2, 4], [4, 6, 4, 7, 9, 5], BATCH, 1), {"df": 3, "flags": 0}),
    # a reduced column's only sample is all unmethylated and deep: at the clamp the decrement stays at n e^-40, above 2^-40 (all
    # methylated it would converge: 1 / (1 + e) is 1.0 from eta = 37 on, and the residual 0.0)
    ("the reduced fit cannot converge", ([6, 5, 7, 3, 0, 4], [4, 6, 4, 7, BIG, 5], BATCH, 1), {"df": 3, "flags": REDUCED | FULL, "iterations": 80}),
    ("the full fit cannot converge", ([6, 5, 7, 0, 0, 0], [4, 6, 4, BIG, BIG, BIG], PLAIN, 1), {"df": 4, "flags": FULL}),
    ("deep and all methylated: it converges", ([6, 5, 7, BIG, BIG, BIG], [4, 6, 4, 0, 0, 0], PLAIN, 1), {"df": 4, "flags": 0}),
    # three deep samples that share both columns and one shallow, all methylated, that has the intercept alone: as its weight falls the
    # second pivot is lost among the roundings of the first
    ("a pivot is lost", ([1 << 23, 1 << 23, 1 << 23, 1], [1 << 23, 1 << 23, 1 << 23, 0], [[1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [1.0, 0.0]], 1),
     {"pvalue": 1.0, "dispersion": 1.0, "statistic": 0.0, "df": 2, "flags": NUMERIC}),
]

# (name, (ms, us), refusal bit): each just outside its bound; the design is PLAIN
REFUSED = [
    ("negative", ([3, -1, 2, 2, 1, 1], [2, 2, 1, 1, 1, 1]), E_NEGATIVE),
    ("negative", ([3, 1, 2, 2, 1, 1], [2, 2, 1, 1, 1, -1]), E_NEGATIVE),
    ("entry", ([LIMIT, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1]), E_ENTRY),
    ("entry", ([1, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, LIMIT]), E_ENTRY),
    ("the methylated of all", ([LIMIT // 2, 1, LIMIT // 4, 1, LIMIT // 4 - 2, 0], [0, 0, 1, 1, 1, 1]), E_MARGIN),
    ("the unmethylated of all", ([1, 1, 3, 3, 0, 1], [2, 2, LIMIT // 2 - 4, 0, LIMIT // 2, 0]), E_MARGIN),
    ("an entry before a margin", ([LIMIT - 1, LIMIT - 1, 1, LIMIT, 1, 1], [0, 0, 1, 1, 1, 1]), E_ENTRY),
]
ACCEPTED = [
    ([LIMIT // 2, 0, LIMIT // 4, 1, LIMIT // 4 - 3, 0], [0, 0, 1, 1, 1, 1], PLAIN, 1),                 # K = 2^26 - 2
    ([1, 1, 3, 3, 0, 1], [2, 2, LIMIT // 2 - 6, 0, LIMIT // 2, 0], PLAIN, 1),                         # M = 2^26 - 1
]
