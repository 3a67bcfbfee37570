// mdk_mdiff_core.h -- a site's counts regressed on a DESIGN MATRIX: the quasi-binomial F test of some columns of a logistic regression
// given the others -- covariates (batch, sex, age, cell-type fraction), paired designs (a dummy per patient) and continuous variables of
// interest (dose, time: the test of one slope is the trend test) --, and nothing else.  The rule alone, with its host build
// (tools/mdiff_emu.cpp) and its tests (tests/test_mdiff_cpu.py); k_mdiff of csrc/mdk_mdiff.hip runs it on the device (libmdk_stats.so:
// mdk.diff_model, Cohort.diff_model).
//
// It continues mdk_qdiff_core.h and mdk_gdiff_core.h: a binomial GLM with logit link on the covered samples of a site, Rao's score
// statistic of the reduced model against the full one over q times the dispersion of McCullagh and Nelder -- Pearson's sum of the FULL
// fit over nu --, the p-value from gdiff_tail: methylKit's calculateDiffMeth(covariates = ...) with overdispersion = "MN", test = "F",
// the score statistic in the place of the deviance.  On a design that is an intercept and group dummies the score statistic is Pearson's
// chi-square of the pooled table and the fitted values are the groups' pooled fractions: mdk_gdiff_core.h's test, within the two error
// bounds.  Not here: the deviance statistic, offsets, interactions or a formula parser, a meth_diff column, shrinkage, one-sided tests,
// more than MDIFF_MAX_COLUMNS columns.
//
// The design X[S', p] holds a row of p doubles per used sample, the r = p - q REDUCED columns first, then the q TESTED ones; 1 <= q < p <=
// 8.  Its entries are finite and at most 2^20 in magnitude (the caller checks).  The entries of the count matrices and their refusals are
// mdk_diff_core.h's (diff_entry_check).  Per site the samples are visited in the order given -- ascending index --, every entry checked
// first:
//   covered     a sample with m + u > 0, n = m + u; an uncovered sample is left out of everything at the site.  k = the covered samples,
//               K = sum m, M = sum u, nu = k - p
//   refused     DIFF_E_MARGIN: K or M of 2^26 or more (mdiff_margin_check)
//   degenerate  nu < 1, K == 0 or M == 0: statistic = 0.0, dispersion = 1.0, p = 1.0, df = max(nu, 0), every coefficient 0.0, flags 0,
//               iterations 0, steps 0
//   a pass      at a beta, over the first c columns (mdiff_pass<c>): g[a], the lower triangle A[a][b] (b <= a) and pearson start at 0.0;
//               per covered sample, in visiting order:
//                 eta = 0.0, then eta = eta + x_a * beta_a for a = 0 .. c - 1; above 40.0 it is 40.0, below -40.0 it is -40.0
//                 e = mdiff_exp(-|eta|);  ope = 1.0 + e;  mu = 1.0 / ope where eta >= 0.0, e / ope otherwise;  v = e / (ope * ope)
//                 w = double(n) * v;  res = double(m) - double(n) * mu
//                 pearson = pearson + (res * res) / w;  g[a] = g[a] + x_a * res;  A[a][b] = A[a][b] + (x_a * x_b) * w
//   mdiff_exp   e^t for t in [-40, 0]: z = t * INV_LN2 (0x1.71547652b82fep+0); kk = -(int32)(-z + 0.5), the cast truncating -- the
//               non-positive z rounded to the nearest integer --; rr = (t - kk * LN2_HI) - kk * LN2_LO (0x1.62e42fee00000p-1, whose
//               product with kk is exact, and 0x1.a39ef35793c76p-33): |rr| is below 0.3466.  Horner over the Taylor coefficients 1 / j!,
//               j = 13 .. 0, held as hex literals: s = c_13, then s = s * rr + c_j; the result is s * 2^kk -- |kk| multiplications by 0.5, every
//               one exact (kk is at least -58: no subnormal), made as one by the power's bit pattern.  The series' remainder is below
//               0.3466^14 / 14! = 4.2e-18.  Measured on the host build against mpmath at 20,173 arguments (tests/test_mdiff_cpu.py):
//               the worst error is 1.516 units of 2^-53 of the exact value (a correctly rounded one has up to 1)
//   Cholesky    of A, lower, in place (mdiff_cholesky<c>): for j = 0 .. c - 1: s = A[j][j], then s = s - L[j][k] * L[j][k] for k = 0 ..
//               j - 1; the PIVOT s must be above rel * A[j][j] and a normal double (qdiff_sqrt takes no other), or the factorisation
//               fails; L[j][j] = qdiff_sqrt(s); for i = j + 1 .. c - 1: s = A[i][j], then s = s - L[i][k] * L[j][k] for k = 0 .. j - 1,
//               L[i][j] = s / L[j][j].  rel is 0.0 in a fit -- a pivot not above 0.0 fails -- and 2^-26 in the rank test
//   solve       d = A^-1 g (mdiff_solve<c>): forward, i = 0 .. c - 1: s = g[i], then s = s - L[i][k] * y[k] for k = 0 .. i - 1, y[i] = s /
//               L[i][i]; back, i = c - 1 .. 0: s = y[i], then s = s - L[k][i] * d[k] for k = i + 1 .. c - 1, d[i] = s / L[i][i]
//   rank        one pass at beta = 0 over all p columns and its Cholesky with rel = 2^-26: a failure -- dropping the uncovered samples
//               left a column dependent on those before it, or empty -- sets MDIFF_RANK; the outputs are those of a degenerate site
//               with df 0
//   Newton      a fit over c columns from a beta (mdiff_fit<c>), at most MDIFF_MAX_PASSES = 40 times: a pass at beta; its Cholesky (a
//               failure sets MDIFF_NUMERIC and ends the site: p = 1.0, statistic = 0.0, dispersion = 1.0, df = nu, every coefficient
//               0.0, iterations the passes made); d = solve; dec = 0.0, then dec = dec + g[a] * d[a] in column order: Newton's
//               decrement; t = the largest |sum_a x_a d_a| over the covered samples (from 0.0, in column order; t starts at 0.0), and
//               where t > 4.0 every d[a] = d[a] * (4.0 / t): no sample's linear predictor moves by more than 4 in a step -- without the
//               cap a low-depth site overshoots into the clamp and comes back with a dispersion of 1e12 --; beta[a] = beta[a] + d[a];
//               the fit has CONVERGED, and ends, where dec <= 2^-40 (a NaN is not).  `iterations` counts the passes of both fits
//   reduced     Newton over the first r columns from 0.0; not converged: MDIFF_REDUCED
//   full        Newton over all p columns from (the reduced beta, 0.0, .. 0.0).  The FIRST pass's dec is the score statistic X, 0.0 where
//               it is not above 0.0.  Not converged: MDIFF_FULL, and the values are reported all the same.  One more pass at the final
//               beta gives pearson
//   result      phi = pearson / double(nu), min_dispersion where it is below; W = X / phi, statistic = W / double(q), df = nu,
//               p = gdiff_tail(W, nu, q); the coefficients are the final beta, on the logit scale
// IEEE doubles with +, -, *, / and comparisons, and conversions between integers and doubles, in ONE order -- no math-library call, no
// fused multiply-add (contraction is off in these functions) --, so the host build, the restatement in Python floats
// (tests/mdiff_rule.py) and the device give the same bits.  The functions are templates over the width c so that a lane's vectors and its
// triangle are indexed by constants alone and live in registers; the arithmetic of a width does not depend on the p it is part of.
//
// The error.  For a site with flags 0 whose exact p -- the same estimator by a 50-digit Newton fit, the tail from mpmath's betainc -- is
// at least 1e-280, the relative error of p, and those of the dispersion and the statistic, are bounded by
//     (MDIFF_C_STEPS steps + (nu + q) (MDIFF_C_NU + MDIFF_C_FIT k p) + MDIFF_C_CONST) 2^-53 + MDIFF_C_TOL (nu + q) 2^-42
// The first part is gdiff_tail's bound with a term for the fit's roundings: res = m - n mu cancels, and the triangle's condition number
// multiplies what is left.  The second is what the tolerance leaves: a fit ends at a decrement of 2^-40 or less; where the full fit is
// SEPARATED -- a column's samples all methylated or all unmethylated, the exact coefficient infinite -- the decrement falls by a factor
// of e a pass, not quadratically, and Pearson's sum keeps about the last decrement where the exact fit has 0.  The constants are
// measured (tests/test_mdiff_cpu.py).
//
// Plain C++ as mdk_gdiff_core.h: it compiles for the device and for the host (tools/mdiff_emu.cpp), which is how it is tested.
#ifndef MDK_MDIFF_CORE_H
#define MDK_MDIFF_CORE_H
#include "mdk_gdiff_core.h"

enum { MDIFF_MAX_COLUMNS = 8, MDIFF_MAX_PASSES = 40 };
enum { MDIFF_RANK = 1, MDIFF_NUMERIC = 2, MDIFF_REDUCED = 4, MDIFF_FULL = 8 };           // the bits of `flags`
enum { MDIFF_C_STEPS = 4, MDIFF_C_NU = 12, MDIFF_C_FIT = 16, MDIFF_C_CONST = 32, MDIFF_C_TOL = 1 };          // the error bound's constants
#define MDIFF_ETA_MAX 40.0                // the linear predictor is clamped to +- this
#define MDIFF_STEP_MAX 4.0                // no sample's linear predictor moves by more in a Newton step
#define MDIFF_CONVERGED 0x1p-40           // a decrement at or below it ends a fit
#define MDIFF_RANK_PIVOT 0x1p-26          // the rank test: a pivot at or below this much of its diagonal entry
#define MDIFF_NORMAL 0x1p-1022            // a pivot below it is no normal double
#define MDIFF_DESIGN_MAX 0x1p20           // the largest magnitude of a design entry
#define MDIFF_INV_LN2 0x1.71547652b82fep+0
#define MDIFF_LN2_HI 0x1.62e42fee00000p-1
#define MDIFF_LN2_LO 0x1.a39ef35793c76p-33
#if defined(__clang__)
#define MDIFF_UNROLL _Pragma("unroll")
#else
#define MDIFF_UNROLL
#endif
#define MDIFF_TRI(a, b) ((a) * ((a) + 1) / 2 + (b))                        // A[a][b], b <= a, in a triangle of c (c + 1) / 2 doubles

struct mdiff_result { double statistic, dispersion, p; int32_t df, iterations; uint32_t steps, flags; };

// what is wrong with a site's pooled counts
MDK_DIFF uint32_t mdiff_margin_check(int64_t K, int64_t M) { return K >= DIFF_LIMIT || M >= DIFF_LIMIT ? DIFF_E_MARGIN : 0u; }

// e^t, t in [-40, 0]
MDK_DIFF double mdiff_exp(double t) {
    MDK_DIFF_NO_CONTRACT
    const double z = t * MDIFF_INV_LN2;
    const int32_t kk = -(int32_t)(-z + 0.5);
    const double dk = (double)kk;
    const double rr = (t - dk * MDIFF_LN2_HI) - dk * MDIFF_LN2_LO;
    double s = 0x1.6124613a86d09p-33;
    s = s * rr + 0x1.1eed8eff8d898p-29;
    s = s * rr + 0x1.ae64567f544e4p-26;
    s = s * rr + 0x1.27e4fb7789f5cp-22;
    s = s * rr + 0x1.71de3a556c734p-19;
    s = s * rr + 0x1.a01a01a01a01ap-16;
    s = s * rr + 0x1.a01a01a01a01ap-13;
    s = s * rr + 0x1.6c16c16c16c17p-10;
    s = s * rr + 0x1.1111111111111p-7;
    s = s * rr + 0x1.5555555555555p-5;
    s = s * rr + 0x1.5555555555555p-3;
    s = s * rr + 0x1.0000000000000p-1;
    s = s * rr + 0x1.0000000000000p+0;
    s = s * rr + 0x1.0000000000000p+0;
    const uint64_t pw = (uint64_t)(kk + 1023) << 52;                         // 2^kk, kk >= -58
    double scale; __builtin_memcpy(&scale, &pw, 8);
    return s * scale;
}

// A `Site` gives a lane its site: samples() the used samples, entry(s, &m, &u) the counts of the s-th in visiting order, x(s, a) its
// design row's column a.

// a pass at beta over the first C columns
template <int C, typename Site>
MDK_DIFF void mdiff_pass(const Site &S, const double *beta, double *g, double *A, double *pearson) {
    MDK_DIFF_NO_CONTRACT
    MDIFF_UNROLL
    for(int a = 0; a < C; a++) g[a] = 0.0;
    MDIFF_UNROLL
    for(int a = 0; a < C * (C + 1) / 2; a++) A[a] = 0.0;
    double pe = 0.0;
    const int32_t all = S.samples();
    for(int32_t s = 0; s < all; s++) {
        int64_t m, u;
        S.entry(s, &m, &u);
        if(m + u <= 0) continue;
        double x[C];
        MDIFF_UNROLL
        for(int a = 0; a < C; a++) x[a] = S.x(s, a);
        double eta = 0.0;
        MDIFF_UNROLL
        for(int a = 0; a < C; a++) eta = eta + x[a] * beta[a];
        if(eta > MDIFF_ETA_MAX) eta = MDIFF_ETA_MAX;
        if(eta < -MDIFF_ETA_MAX) eta = -MDIFF_ETA_MAX;
        const double e = mdiff_exp(eta < 0.0 ? eta : -eta);
        const double ope = 1.0 + e;
        const double mu = eta >= 0.0 ? 1.0 / ope : e / ope;
        const double v = e / (ope * ope);
        const double dn = (double)(m + u);
        const double w = dn * v;
        const double res = (double)m - dn * mu;
        pe = pe + (res * res) / w;
        MDIFF_UNROLL
        for(int a = 0; a < C; a++) {
            g[a] = g[a] + x[a] * res;
            MDIFF_UNROLL
            for(int b = 0; b <= a; b++) A[MDIFF_TRI(a, b)] = A[MDIFF_TRI(a, b)] + (x[a] * x[b]) * w;
        }
    }
    *pearson = pe;
}

// A = L L' in place; false: a pivot is not above rel times its diagonal entry, or is no normal double
template <int C>
MDK_DIFF bool mdiff_cholesky(double *A, double rel) {
    MDK_DIFF_NO_CONTRACT
    bool good = true;
    MDIFF_UNROLL
    for(int j = 0; j < C; j++) {
        const double diag = A[MDIFF_TRI(j, j)];
        double s = diag;
        MDIFF_UNROLL
        for(int k = 0; k < j; k++) s = s - A[MDIFF_TRI(j, k)] * A[MDIFF_TRI(j, k)];
        if(!(s > rel * diag) || !(s >= MDIFF_NORMAL)) { good = false; s = 1.0; }          // (the rest is made of 1.0 and not used)
        const double l = qdiff_sqrt(s);
        A[MDIFF_TRI(j, j)] = l;
        MDIFF_UNROLL
        for(int i = j + 1; i < C; i++) {
            double v = A[MDIFF_TRI(i, j)];
            MDIFF_UNROLL
            for(int k = 0; k < j; k++) v = v - A[MDIFF_TRI(i, k)] * A[MDIFF_TRI(j, k)];
            A[MDIFF_TRI(i, j)] = v / l;
        }
    }
    return good;
}

// d = (L L')^-1 g
template <int C>
MDK_DIFF void mdiff_solve(const double *L, const double *g, double *d) {
    MDK_DIFF_NO_CONTRACT
    MDIFF_UNROLL
    for(int i = 0; i < C; i++) {
        double s = g[i];
        MDIFF_UNROLL
        for(int k = 0; k < i; k++) s = s - L[MDIFF_TRI(i, k)] * d[k];
        d[i] = s / L[MDIFF_TRI(i, i)];
    }
    MDIFF_UNROLL
    for(int i = C - 1; i >= 0; i--) {
        double s = d[i];
        MDIFF_UNROLL
        for(int k = i + 1; k < C; k++) s = s - L[MDIFF_TRI(k, i)] * d[k];
        d[i] = s / L[MDIFF_TRI(i, i)];
    }
}

// the largest |x d| over the covered samples
template <int C, typename Site>
MDK_DIFF double mdiff_reach(const Site &S, const double *d) {
    MDK_DIFF_NO_CONTRACT
    double t = 0.0;
    const int32_t all = S.samples();
    for(int32_t s = 0; s < all; s++) {
        int64_t m, u;
        S.entry(s, &m, &u);
        if(m + u <= 0) continue;
        double h = 0.0;
        MDIFF_UNROLL
        for(int a = 0; a < C; a++) h = h + S.x(s, a) * d[a];
        if(h < 0.0) h = -h;
        if(h > t) t = h;
    }
    return t;
}

// Newton over the first C columns from beta: 0 or MDIFF_NUMERIC; *first_dec the first pass's decrement, *passes raised by the passes made
template <int C, typename Site>
MDK_DIFF uint32_t mdiff_fit(const Site &S, double *beta, double *first_dec, bool *converged, int32_t *passes) {
    MDK_DIFF_NO_CONTRACT
    *converged = false; *first_dec = 0.0;
    for(int32_t it = 0; it < MDIFF_MAX_PASSES; it++) {
        double g[C], A[C * (C + 1) / 2], d[C], pearson;
        mdiff_pass<C>(S, beta, g, A, &pearson);
        *passes += 1;
        if(!mdiff_cholesky<C>(A, 0.0)) return MDIFF_NUMERIC;
        mdiff_solve<C>(A, g, d);
        double dec = 0.0;
        MDIFF_UNROLL
        for(int a = 0; a < C; a++) dec = dec + g[a] * d[a];
        if(it == 0) *first_dec = dec;
        const double t = mdiff_reach<C>(S, d);
        if(t > MDIFF_STEP_MAX) {
            const double sc = MDIFF_STEP_MAX / t;
            MDIFF_UNROLL
            for(int a = 0; a < C; a++) d[a] = d[a] * sc;
        }
        MDIFF_UNROLL
        for(int a = 0; a < C; a++) beta[a] = beta[a] + d[a];
        if(dec <= MDIFF_CONVERGED) { *converged = true; break; }
    }
    return 0;
}

// the reduced fit: the width is r, one of 1 .. P - 1
template <int P, int C, typename Site>
MDK_DIFF uint32_t mdiff_fit_reduced(const Site &S, int32_t r, double *beta, double *first_dec, bool *converged, int32_t *passes) {
    if constexpr(C + 1 < P) { if(r != C) return mdiff_fit_reduced<P, C + 1>(S, r, beta, first_dec, converged, passes); }
    return mdiff_fit<C>(S, beta, first_dec, converged, passes);
}

// a site's result from its covered samples k and its sums K and M, the counts checked: the design has P columns, the first r reduced
template <int P, typename Site>
MDK_DIFF void mdiff_site(const Site &S, int32_t r, int32_t k, int64_t K, int64_t M, double min_dispersion, double *coef, mdiff_result *out) {
    MDK_DIFF_NO_CONTRACT
    const int32_t nu = k - P, q = P - r;
    out->statistic = 0.0; out->dispersion = 1.0; out->p = 1.0; out->df = nu > 0 ? nu : 0; out->iterations = 0; out->steps = 0; out->flags = 0;
    MDIFF_UNROLL
    for(int a = 0; a < P; a++) coef[a] = 0.0;
    if(nu < 1 || K == 0 || M == 0) return;
    double beta[P], g[P], A[P * (P + 1) / 2], pearson, X, unused;
    bool converged;
    MDIFF_UNROLL
    for(int a = 0; a < P; a++) beta[a] = 0.0;
    mdiff_pass<P>(S, beta, g, A, &pearson);
    if(!mdiff_cholesky<P>(A, MDIFF_RANK_PIVOT)) { out->flags = MDIFF_RANK; out->df = 0; return; }
    uint32_t flags = mdiff_fit_reduced<P, 1>(S, r, beta, &unused, &converged, &out->iterations);
    if(flags) { out->flags = flags; return; }
    if(!converged) flags |= MDIFF_REDUCED;
    const uint32_t failed = mdiff_fit<P>(S, beta, &X, &converged, &out->iterations);
    if(failed) { out->flags = flags | failed; return; }
    if(!converged) flags |= MDIFF_FULL;
    if(!(X > 0.0)) X = 0.0;
    mdiff_pass<P>(S, beta, g, A, &pearson);
    double phi = pearson / (double)nu;
    if(phi < min_dispersion) phi = min_dispersion;
    const double W = X / phi;
    out->dispersion = phi; out->statistic = W / (double)q; out->flags = flags;
    out->p = gdiff_tail(W, nu, q, &out->steps);
    MDIFF_UNROLL
    for(int a = 0; a < P; a++) coef[a] = beta[a];
}
// are the columns of a design X[rows, P] independent over all its rows?  The rank test on the unweighted Gram matrix X'X, added row by row
template <int P>
MDK_DIFF bool mdiff_gram_test(const double *X, int32_t rows) {
    MDK_DIFF_NO_CONTRACT
    double A[P * (P + 1) / 2];
    MDIFF_UNROLL
    for(int a = 0; a < P * (P + 1) / 2; a++) A[a] = 0.0;
    for(int32_t s = 0; s < rows; s++) {
        MDIFF_UNROLL
        for(int a = 0; a < P; a++) {
            MDIFF_UNROLL
            for(int b = 0; b <= a; b++) A[MDIFF_TRI(a, b)] = A[MDIFF_TRI(a, b)] + X[(int64_t)s * P + a] * X[(int64_t)s * P + b];
        }
    }
    return mdiff_cholesky<P>(A, MDIFF_RANK_PIVOT);
}
MDK_DIFF bool mdiff_independent(const double *X, int32_t rows, int32_t p) {
    switch(p) {
    case 2: return mdiff_gram_test<2>(X, rows);
    case 3: return mdiff_gram_test<3>(X, rows);
    case 4: return mdiff_gram_test<4>(X, rows);
    case 5: return mdiff_gram_test<5>(X, rows);
    case 6: return mdiff_gram_test<6>(X, rows);
    case 7: return mdiff_gram_test<7>(X, rows);
    case 8: return mdiff_gram_test<8>(X, rows);
    }
    return false;
}
#endif
