// mdk_gdiff_core.h -- THREE OR MORE groups of replicate samples compared site by site: the quasi-binomial F test of a site's counts with
// q = groups - 1 degrees of freedom in the numerator, and nothing else.  The rule alone, with its host build (tools/gdiff_emu.cpp) and its
// tests (tests/test_gdiff_cpu.py); k_gdiff of csrc/mdk_gdiff.hip runs it on the device (libmdk_stats.so: mdk.diff_groups,
// Cohort.diff_groups).
//
// It is mdk_qdiff_core.h's test with a covariate of G levels in the place of two: the quasi-likelihood score test of "every group has one
// fraction" -- Pearson's chi-square of the pooled G x 2 table -- over q times the dispersion of McCullagh and Nelder, estimated from
// Pearson's residuals of the samples around their group's pooled fraction: methylKit's calculateDiffMeth for several treatment levels
// with overdispersion = "MN", test = "F", the score statistic in the place of the deviance.  With two covered groups every number is
// mdk_qdiff_core.h's, to the bit.  Not here: the deviance statistic, one-sided tests, a chi-square p-value for designs without
// replicates (such a site has p 1.0 and df 0), shrinkage; covariates, pairs and trend tests are mdk_mdiff_core.h's.
//
// The entries and their refusals are mdk_diff_core.h's (diff_entry_check).  Per site the groups are visited in the order given and a
// group's samples in ascending index, every entry checked first:
//   covered     a sample with m + u > 0; an uncovered sample is left out of everything at the site, and so is a group without a covered
//               sample.  g_eff = the covered groups, k = their covered samples; q = g_eff - 1, nu = k - g_eff -- and k - 2 where g_eff is
//               below 2, which is what mdk_qdiff_core.h reports for such a site: a call with two groups is its call
//   pooled      per group gm, gu = its methylated and unmethylated sums, n_g = gm + gu; K = sum gm, M = sum gu, N = K + M
//   refused     DIFF_E_MARGIN: an n_g, K or M of 2^26 or more (gdiff_margin_check; with two groups that is diff_margin_check).  Below it
//               gm N and n_g K are below 2^53 and K M below 2^52: e_g is exact in int64
//   degenerate  g_eff < 2, nu < 1, K == 0 or M == 0: statistic = 0.0, dispersion = 1.0, p = 1.0, df = max(nu, 0), df_groups = max(q, 0)
//   score       g_eff == 2: qdiff_score of the two covered groups, the lower group index first.  Otherwise e_g = gm N - n_g K in int64
//               and X = the sum over the covered groups, in order from 0.0, of (double(e_g) * double(e_g)) / (double(n_g) * double(K M))
//               (gdiff_score_term) -- Pearson's chi-square of the G x 2 table
//   Pearson     as mdk_qdiff_core.h: a group with gm == 0 or gu == 0 contributes nothing; otherwise qdiff_term of each of its covered
//               samples, added in visiting order from 0.0
//   dispersion  phi = pearson / double(nu); min_dispersion where phi is below it
//   statistic   W = X / phi; statistic = W / double(q), df = nu, df_groups = q;
//               p = P(F(q, nu) > statistic) = I_x(nu / 2, q / 2), x = nu / (nu + W)
//   effect      group_lo, group_hi = the covered groups of the smallest and of the largest fraction gm / n_g, compared exactly -- gm_i n_j
//               against gm_j n_i in int64 --, a tie to the lower group index; meth_diff = diff_meth(lo's counts, hi's counts), never
//               negative.  One covered group: both are that group and meth_diff is 0.0.  None: -1, -1 and 0.0
// The tail (gdiff_tail) is qdiff_tail with the general coefficients: IEEE doubles with +, * and / and comparisons alone, in ONE order --
// no math-library call, no fused multiply-add (contraction is off in these functions), sums of positive terms with at most one final
// 1.0 - s --, so the host build, the restatement in Python floats (tests/gdiff_rule.py) and the device give the same bits; and
// gdiff_tail(W, nu, 1) goes through qdiff_tail's operations one by one, so it gives qdiff_tail(W, nu)'s bits:
//   the ends    W < 2^-940: p = 1.0.  W >= 2^1000: p = 0.0.  As in mdk_qdiff_core.h no site reaches either but W == 0.0: X is at most
//               N, below 2^27, and pearson at most 2^79
//   the split   t = double(nu) + W, x = double(nu) / t, y = W / t
//   constant    B0 = B(nu / 2, 1 / 2) for an odd q, made as qdiff_tail makes it (pi or 2.0, then (B0 * j) / (j + 1) for j = 1 or 2, by 2,
//               below nu); B0 = B(nu / 2, 1) = 2.0 / double(nu) for an even q.  B(nu / 2, q / 2) = B0 times the FACTORS g / (nu + g), g = 1,
//               3, .. q - 2 (odd q) or 2, 4, .. q - 2 (even q), by B(a, b + 1) = B(a, b) b / (a + b).  B0 is between 2 / nu and pi;
//               the factors are below 1 and their product can be below 2^-1000 -- 1 / B(nu / 2, q / 2) is as large as the
//               binomial coefficient it is --, so they are never multiplied on their own: each is DIVIDED INTO THE POWER, below
//   branch      direct where x * double(nu + q + 4) <= double(nu + 2), the complement otherwise
//   roots       sx = qdiff_sqrt(x), sy = qdiff_sqrt(y)
//   power       top = x^(nu / 2) y^(q / 2) B0 / B(nu / 2, q / 2), as one running product: sx for an odd nu, 1.0 for an even one; nu / 2
//               (rounded down) times `* x`; for an odd q `* sy`; q / 2 (rounded down) times `* y`; then the factors that are left.
//               After every `* x` and every `* y`: while the product is below 1.0 and a factor is left, the next factor goes in -- top =
//               (top * double(nu + g)) / double(g), g += 2 -- and then, the product below GDIFF_TINY = 2^-940, the site is done: p = 0.0
//               on the direct branch, 1.0 on the complement's.
//               Why no partial product underflows while p is 1e-280 or more: x and y are at most 1 and every factor's inverse is above
//               1, so a product below 1.0 is first lifted by what can lift it.  Where it is still below 2^-940 no factor is left, all
//               that follows is x or y, and the final top is below 2^-940: on the direct branch p = top sum / ((nu / 2) B0) with sum at
//               most (nu + q + 4) / 4 -- the series' ratios are at most (nu + q) / (nu + q + 4) -- and (nu / 2) B0 at least 1, so p is
//               below 2^-940 x 513 for nu + q up to 2048, which is 5.6e-281; on the complement 1 - p is that small.  (Cutting as soon
//               as x^(nu / 2) alone is below 2^-940 would be wrong: at nu = 62, q = 15, W = 1e11 it is 1e-331 and p is 2.0e-279.)  A
//               factor's inverse is at most nu + 1, so a lifted product stays below 2^11; the factors that are left at the end are
//               multiplied into a product that rises to its final value, which is at most B0 (q / 2) (the complement's 1 - p is at
//               most 1): nothing overflows.  While a factor is left the product is at least 1.0 before it meets x or y, and x is at
//               least 2^-1000: the only product that may be a subnormal is the one that ends the site
//   direct      pre = top / ((double(nu) / 2.0) * B0); u_0 = 1.0, u_{n+1} = ((u_n * x) * double(nu + q + 2n)) / double(nu + 2 + 2n);
//               p = min(1.0, pre * sum u)
//   complement  pre = top / ((double(q) / 2.0) * B0); u_{n+1} = ((u_n * y) * double(nu + q + 2n)) / double(q + 2 + 2n);
//               p = 1.0 - pre * sum u, at least 0.0
//   the sums    as qdiff_tail's: u is added, then the next term made; the series ends before the first term below 2^-64 of the sum so
//               far.  Both fall from their first term: the first ratios are x (nu + q) / (nu + 2) and y (nu + q) / (q + 2), below 1 by
//               the branch, and the ratios move towards x and y one way.  `steps` counts the terms added
// The relative error of p against exact arithmetic -- X, phi and W as rationals, the tail from mpmath's betainc at 70 digits -- is bounded
// by (GDIFF_C_STEPS steps + GDIFF_C_NU (nu + q) + GDIFF_C_CONST) 2^-53 wherever the exact p is at least 1e-280; below that p may be 0.0.
// The constants are measured (tests/test_gdiff_cpu.py): the worst error over the test's grid is 0.307 of this bound.
//
// Plain C++ as mdk_qdiff_core.h: it compiles for the device and for the host (tools/gdiff_emu.cpp), which is how it is tested.
#ifndef MDK_GDIFF_CORE_H
#define MDK_GDIFF_CORE_H
#include "mdk_qdiff_core.h"

#define GDIFF_TINY QDIFF_TINY             // a W or a running product (no factor left) below it ends the site
#define GDIFF_HUGE QDIFF_HUGE             // a W from here on: p = 0.0
enum { GDIFF_C_STEPS = 4, GDIFF_C_NU = 12, GDIFF_C_CONST = 32 };          // the error bound's constants

struct gdiff_result { double statistic, dispersion, p; int32_t df, df_groups; uint32_t steps; };

// what is wrong with a site's pooled counts: call it with every covered group's depth (K = M = 0) and once with 0 and the sums of all
MDK_DIFF uint32_t gdiff_margin_check(int64_t n_g, int64_t K, int64_t M) { return n_g >= DIFF_LIMIT || K >= DIFF_LIMIT || M >= DIFF_LIMIT ? DIFF_E_MARGIN : 0u; }

// is the fraction gm / gn below the fraction hm / hn?  gn, hn > 0
MDK_DIFF bool gdiff_below(int64_t gm, int64_t gn, int64_t hm, int64_t hn) { return gm * hn < hm * gn; }

// a covered group's term of the pooled table's chi-square: its counts, the sums of all (K > 0, M > 0)
MDK_DIFF double gdiff_score_term(int64_t gm, int64_t gu, int64_t K, int64_t M) {
    MDK_DIFF_NO_CONTRACT
    const int64_t e = gm * (K + M) - (gm + gu) * K;
    const double ee = (double)e * (double)e;
    const double den = (double)(gm + gu) * (double)(K * M);
    return ee / den;
}

// P(F(q, nu) > W / q), nu >= 1, q >= 1, W not negative and no NaN; *steps (if given): the terms that were added to the series
MDK_DIFF double gdiff_tail(double W, int32_t nu, int32_t q, uint32_t *steps) {
    MDK_DIFF_NO_CONTRACT
    if(steps) *steps = 0;
    if(W < GDIFF_TINY) return 1.0;
    if(W >= GDIFF_HUGE) return 0.0;
    const double dnu = (double)nu, dq = (double)q;
    const double t = dnu + W;
    const double x = dnu / t, y = W / t;
    double B; int32_t g;                                                     // g: the next factor of B(nu / 2, q / 2) over B0
    if(q & 1) {
        int32_t j;
        if(nu & 1) { B = QDIFF_PI; j = 1; } else { B = 2.0; j = 2; }
        while(j < nu) {
            B = B * (double)j;
            B = B / (double)(j + 1);
            j += 2;
        }
        g = 1;
    } else { B = 2.0 / dnu; g = 2; }
    const bool tail = x * (double)(nu + q + 4) <= (double)(nu + 2);
    const double ended = tail ? 0.0 : 1.0;
    const double sx = qdiff_sqrt(x), sy = qdiff_sqrt(y);
    const int32_t last = q - 2;
    double top = nu & 1 ? sx : 1.0;
    for(int32_t k = 0; k < nu / 2; k++) {
        top = top * x;
        while(top < 1.0 && g <= last) {
            top = top * (double)(nu + g);
            top = top / (double)g;
            g += 2;
        }
        if(top < GDIFF_TINY) return ended;
    }
    if(q & 1) top = top * sy;
    for(int32_t k = 0; k < q / 2; k++) {
        top = top * y;
        while(top < 1.0 && g <= last) {
            top = top * (double)(nu + g);
            top = top / (double)g;
            g += 2;
        }
        if(top < GDIFF_TINY) return ended;
    }
    while(g <= last) {
        top = top * (double)(nu + g);
        top = top / (double)g;
        g += 2;
    }
    const double pre = tail ? top / ((dnu / 2.0) * B) : top / ((dq / 2.0) * B);
    const double v = tail ? x : y;
    double sum = 0.0, u = 1.0; uint32_t added = 0;
    int32_t up = nu + q, down = tail ? nu + 2 : q + 2;
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
    const double s = pre * sum;
    if(tail) return s < 1.0 ? s : 1.0;
    const double p = 1.0 - s;
    return p > 0.0 ? p : 0.0;
}

// a site's result from its sums: the covered groups and their covered samples, K and M of all, the score X (0.0 where the site is
// degenerate: it is not used) and Pearson's sum; the counts checked
MDK_DIFF void gdiff_site(int32_t g_eff, int32_t k, int64_t K, int64_t M, double X, double pearson, double min_dispersion, gdiff_result *r) {
    MDK_DIFF_NO_CONTRACT
    const int32_t q = g_eff - 1, nu = k - (g_eff > 2 ? g_eff : 2);
    r->statistic = 0.0; r->dispersion = 1.0; r->p = 1.0; r->df = nu > 0 ? nu : 0; r->df_groups = q > 0 ? q : 0; r->steps = 0;
    if(g_eff < 2 || nu < 1 || K == 0 || M == 0) return;
    double phi = pearson / (double)nu;
    if(phi < min_dispersion) phi = min_dispersion;
    const double W = X / phi;
    r->dispersion = phi; r->statistic = W / (double)q;
    r->p = gdiff_tail(W, nu, q, &r->steps);
}
#endif
