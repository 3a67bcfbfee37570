// mdk_qdiff_core.h -- two groups of REPLICATE samples compared site by site: the quasi-binomial F test of a site's counts, and nothing else.
// The rule alone, with its host build (tools/qdiff_emu.cpp) and its tests (tests/test_qdiff_cpu.py); k_qdiff of csrc/mdk_qdiff.hip runs it
// on the device (libmdk_stats.so: mdk.diff_replicates, Cohort.diff_replicates).
//
// It is the quasi-likelihood score test of a logistic regression with one two-level covariate (the group), the dispersion estimated as
// McCullagh and Nelder do, from Pearson's residuals of the samples around their group's pooled fraction: the idea of methylKit's
// overdispersion = "MN", test = "F", with the score statistic in the place of the deviance.  Fisher's test of the pooled table
// (mdk_diff_core.h) takes the reads of a group for independent draws; replicates differ by more than that, and this test divides the
// pooled statistic by how much they do.  Not here: one-sided tests, the deviance statistic, shrinkage (more groups: mdk_gdiff_core.h; covariates: mdk_mdiff_core.h).
//
// The entries, limits and refusals are mdk_diff_core.h's (diff_entry_check, diff_margin_check; meth_diff is diff_meth).  Per site the
// samples are visited in ascending index, every entry checked first:
//   covered     a sample with m + u > 0; the uncovered samples of a group are left out of everything at the site.  ka, kb = the covered
//               samples of A and of B, nu = ka + kb - 2
//   pooled      a, b = A's methylated and unmethylated sums, c, d = B's; N = a + b + c + d, K = a + c, M = b + d
//   degenerate  ka == 0, kb == 0, nu < 1, K == 0 or M == 0: statistic = 0.0, dispersion = 1.0, p = 1.0, df = max(nu, 0)
//   score       det = a d - b c in int64 (exact: the margins are below 2^26);
//               X = ((double(det) * double(det)) * double(N)) / (double((a + b)(c + d)) * double(K M)) -- Pearson's chi-square of the table
//   Pearson     a group whose pooled gm == 0 or gu == 0 contributes nothing (its fitted values are its observations); otherwise every covered
//               sample (m_i, u_i) of it, n_i = m_i + u_i, gn = gm + gu: e = m_i gn - n_i gm in int64, the term
//               (double(e) * double(e)) / (double(n_i) * double(gm gu)).  The terms are added in visiting order, from 0.0
//   dispersion  phi = pearson / double(nu); min_dispersion where phi is below it (the default floor of 1.0: replicates are never taken for
//               LESS variable than independent draws, which is what makes the test conservative without over-dispersion)
//   statistic   F = X / phi; df = nu;  p = P(F(1, nu) > F) = I_x(nu / 2, 1 / 2), x = nu / (nu + F)
// The tail (qdiff_tail) is made of IEEE doubles with +, * and / and comparisons alone, in ONE order -- no math-library call, no sqrt, no
// fused multiply-add (contraction is off in these functions), sums of positive terms only, no subnormal --, so a host build of this
// header (tools/qdiff_emu.cpp) and a restatement in Python floats (tests/qdiff_rule.py) give the same bits, as a device build would:
//   the ends    F < 2^-940: p = 1.0 (F == 0.0 is such; 1 - p is below 2^-460 there).  F >= 2^1000: p = 0.0 (an infinite F is such).  X
//               is at most N, below 2^27, and where it is not 0.0 at least 16 / N^3, above 2^-77; pearson is at most 2^79.  So with a
//               min_dispersion from 2^-55 to 2^800 no site reaches either end but F == 0.0, F is between 2^-877 and 2^82, x is above
//               2^-82 and no subnormal is formed anywhere below.  Outside that range the ends keep zeros and infinities out of the
//               series, and the last product of the power may be a subnormal before it ends the site
//   the split   t = double(nu) + F, x = double(nu) / t, y = F / t
//   constant    B = B(nu / 2, 1 / 2): pi (0x1.921fb54442d18p+1), j = 1 for an odd nu, 2.0, j = 2 for an even one; while j < nu:
//               B = (B * double(j)) / double(j + 1), j += 2
//   roots       sx = qdiff_sqrt(x), sy = qdiff_sqrt(y).  qdiff_sqrt(v), v a normal double: v = f * 4^h with f in [0.5, 2) -- the
//               exponent halved, exact --, r = 0.5 * f + 0.5, five times r = 0.5 * (r + f / r), the result r * 2^h (exact).  The
//               seed is within 6.1 % and a step squares the relative error and halves it: after four it is below 2^-80
//   power       pw = x^(nu / 2): sx for an odd nu, 1.0 for an even one, then nu / 2 (rounded down) times pw = pw * x -- x is one rounding
//               from exact and sx some three, so the power is made of x as far as it can be.  A partial product below QDIFF_TINY =
//               2^-940: p = 0.0 and the site is done (p is below 2^-940 (nu + 5) / (3 (nu / 2) B), at most 9 2^-940, below 1e-280;
//               sx itself is above 2^-512)
//   tail branch x * double(nu + 5) <= double(nu + 2): pre = (pw * sy) / ((double(nu) / 2.0) * B); u_0 = 1.0,
//               u_{n+1} = ((u_n * x) * double(nu + 1 + 2n)) / double(nu + 2 + 2n); p = min(1.0, pre * sum u)
//   complement  otherwise: pre = (pw * sy) / (0.5 * B); u_{n+1} = ((u_n * y) * double(nu + 1 + 2n)) / double(3 + 2n);
//               p = 1.0 - pre * sum u, at least 0.0
//   the sums    sum = 0.0; u is added, then the next term is made, and the series ends before the first term that is below 2^-64 of the
//               sum so far.  Both series fall from their first term (x <= (nu + 2) / (nu + 5); y < 3 / (nu + 5)), so the smallest
//               term formed is above 2^-65.  `steps` counts the terms added: at most some 330 for nu <= 30 (F near 4), about 9,600
//               for nu = 1022
// The relative error of p against exact arithmetic -- X, phi and F as rationals, the tail to 60 digits -- is bounded by
// (QDIFF_C_STEPS steps + QDIFF_C_NU nu + QDIFF_C_CONST) 2^-53 wherever the exact p is at least 1e-280 (tests/test_qdiff_cpu.py measures it).
//
// Plain C++ as mdk_diff_core.h: it compiles for the device and for the host (tools/qdiff_emu.cpp), which is how it is tested.
#ifndef MDK_QDIFF_CORE_H
#define MDK_QDIFF_CORE_H
#include "mdk_diff_core.h"

#define QDIFF_TINY 0x1p-940               // an F or a partial power below it ends the site
#define QDIFF_HUGE 0x1p1000               // an F from here on: p = 0.0
#define QDIFF_NEGLIGIBLE 0x1p-64          // a term below this much of the sum ends a series
#define QDIFF_PI 0x1.921fb54442d18p+1
#define QDIFF_SQRT_STEPS 5
enum { QDIFF_C_STEPS = 4, QDIFF_C_NU = 12, QDIFF_C_CONST = 32 };          // the error bound's constants

struct qdiff_result { double statistic, dispersion, p; int32_t df; uint32_t steps; };

// the square root of a normal double, v > 0
MDK_DIFF double qdiff_sqrt(double v) {
    MDK_DIFF_NO_CONTRACT
    uint64_t w; __builtin_memcpy(&w, &v, 8);
    const int32_t E = (int32_t)((w >> 52) & 0x7ffu) - 1023;                  // v = 1.m * 2^E
    const int32_t odd = E & 1;
    const int32_t h = (E + odd) / 2;                                         // E + odd is even: v = f * 4^h, f = 1.m (E even) or 1.m / 2 (E odd)
    uint64_t fw = (w & 0x000fffffffffffffull) | ((uint64_t)(1023 - odd) << 52);
    double f; __builtin_memcpy(&f, &fw, 8);
    double r = 0.5 * f;
    r = r + 0.5;
    for(int k = 0; k < QDIFF_SQRT_STEPS; k++) {
        const double q = f / r;
        r = 0.5 * (r + q);
    }
    const uint64_t sw = (uint64_t)(h + 1023) << 52;                          // 2^h, h >= -511
    double scale; __builtin_memcpy(&scale, &sw, 8);
    return r * scale;
}

// Pearson's chi-square of the pooled table; K > 0, M > 0 and both groups covered
MDK_DIFF double qdiff_score(int64_t a, int64_t b, int64_t c, int64_t d) {
    MDK_DIFF_NO_CONTRACT
    const int64_t det = a * d - b * c;
    const double dd = (double)det * (double)det;
    const double num = dd * (double)(a + b + c + d);
    const double den = (double)((a + b) * (c + d)) * (double)((a + c) * (b + d));
    return num / den;
}

// a covered sample's term of Pearson's sum: its entries (m, u), its group's pooled counts (gm, gu), both above 0
MDK_DIFF double qdiff_term(int64_t m, int64_t u, int64_t gm, int64_t gu) {
    MDK_DIFF_NO_CONTRACT
    const int64_t e = m * (gm + gu) - (m + u) * gm;
    const double ee = (double)e * (double)e;
    const double den = (double)(m + u) * (double)(gm * gu);
    return ee / den;
}

// P(F(1, nu) > F), nu >= 1, F not negative and no NaN; *steps (if given): the terms that were added to the series
MDK_DIFF double qdiff_tail(double F, int32_t nu, uint32_t *steps) {
    MDK_DIFF_NO_CONTRACT
    if(steps) *steps = 0;
    if(F < QDIFF_TINY) return 1.0;
    if(F >= QDIFF_HUGE) return 0.0;
    const double dnu = (double)nu;
    const double t = dnu + F;
    const double x = dnu / t, y = F / t;
    double B; int32_t j;
    if(nu & 1) { B = QDIFF_PI; j = 1; } else { B = 2.0; j = 2; }
    while(j < nu) {
        B = B * (double)j;
        B = B / (double)(j + 1);
        j += 2;
    }
    const double sx = qdiff_sqrt(x), sy = qdiff_sqrt(y);
    double pw = nu & 1 ? sx : 1.0;
    for(int32_t k = 0; k < nu / 2; k++) {
        pw = pw * x;
        if(pw < QDIFF_TINY) return 0.0;
    }
    const double top = pw * sy;
    const bool tail = x * (double)(nu + 5) <= (double)(nu + 2);
    const double pre = tail ? top / ((dnu / 2.0) * B) : top / (0.5 * B);
    const double v = tail ? x : y;
    double sum = 0.0, u = 1.0; uint32_t added = 0;
    int32_t up = nu + 1, down = tail ? nu + 2 : 3;
    for(;;) {
        sum = sum + u;
        added++;
        u = u * v;
        u = u * (double)up;
        u = u / (double)down;
        up += 2; down += 2;
        if(u < QDIFF_NEGLIGIBLE * sum) break;
    }
    if(steps) *steps = added;
    const double q = pre * sum;
    if(tail) return q < 1.0 ? q : 1.0;
    const double p = 1.0 - q;
    return p > 0.0 ? p : 0.0;
}

// a site's result from its pooled counts, its covered samples and Pearson's sum (0.0 where no group contributes); the counts checked
MDK_DIFF void qdiff_site(int64_t a, int64_t b, int64_t c, int64_t d, int32_t ka, int32_t kb, double pearson, double min_dispersion, qdiff_result *r) {
    MDK_DIFF_NO_CONTRACT
    const int32_t nu = ka + kb - 2;
    r->statistic = 0.0; r->dispersion = 1.0; r->p = 1.0; r->df = nu > 0 ? nu : 0; r->steps = 0;
    if(ka == 0 || kb == 0 || nu < 1 || a + c == 0 || b + d == 0) return;
    double phi = pearson / (double)nu;
    if(phi < min_dispersion) phi = min_dispersion;
    const double F = qdiff_score(a, b, c, d) / phi;
    r->dispersion = phi; r->statistic = F;
    r->p = qdiff_tail(F, nu, &r->steps);
}
#endif
