// mdk_diff_core.h -- two groups of samples compared site by site: the two-sided p-value of Fisher's exact test of a site's pooled 2 x 2
// table and the difference of the groups' methylation, what is refused, and nothing else (csrc/mdk_diff.hip: mdk.diff_counts,
// Cohort.diff).
//
// A site's table is four pooled counts, int64: a = methylated in group A, b = unmethylated in A, c = methylated in B, d = unmethylated in
// B -- each the sum of the site's entries over the samples of its group.  n = a + b, K = a + c, M = b + d, N = n + c + d.  The tables with
// these margins have k = lo .. hi methylated in A, lo = max(0, n - M), hi = min(n, K), with hypergeometric weight w_k; the p-value is the
// weight of the tables no likelier than the observed one (k = a) over the weight of all.
//
// The rule uses IEEE doubles with *, / and + alone, in ONE order -- no lgamma, log, exp, no fused multiply-add (contraction is off in
// these functions), no subnormal --, so the device, a host build of this header (tools/diff_emu.cpp) and a restatement in Python floats
// (tests/diff_rule.py) give the same bits:
//   degenerate  lo == hi: p = 1.0 (one table has the margins; a group without coverage is such a site)
//   the mode    mode = ((n + 1)(K + 1)) / (N + 2) in 64-bit integers, clamped to lo .. hi: the most likely table
//   the terms   r_k = DIFF_ONE * w_k / w_mode: r_mode = DIFF_ONE = 2^60, upward r_{k+1} = (r_k * double((K - k)(n - k))) / double((k + 1)
//               (M - n + k + 1)), downward r_{k-1} = (r_k * double(k (M - n + k))) / double((K - k + 1)(n - k + 1)).  The integer
//               products are formed in int64 and are exact as doubles, every margin being below 2^26: a term is one multiplication and
//               one division.  (2^60 and not 1.0: a power of two changes no significand, and it leaves room under the smallest term
//               that is kept, below)
//   the walk    from the mode to k = a, which gives r_obs.  If a term of the walk is below DIFF_TINY = 2^-900 -- 2^-960 of the mode's --
//               p = 0.0 and the site is done: its p-value is below 1e-280 (r_obs / DIFF_ONE >= p / 2^26, and 1e-280 > 2^-931)
//   the bar     thr = r_obs * (1.0 + 1e-7): the tie rule of R's fisher.test and of scipy
//   the sums    from the mode upward, then from mode - 1 downward: every term is added to total, every term <= thr to tail.  A direction
//               ends at the end of the support, and once the observed table is not ahead in it (upward a <= k, downward a >= k), the
//               term is <= thr and the term is below 2^-64 * tail.  The smallest term formed is thus above 2^-900 * 2^-64 * 2^-52
//   the result  p = min(1.0, tail / total)
// diff_pvalue is the rule, statement by statement as tests/diff_rule.py has it: a site's order of operations is its own, whatever
// lane runs it.  `steps` counts the terms added to the sums: the relative error of p against exact rational arithmetic is bounded
// by (4 steps + 8) 2^-53 (tests/test_diff_cpu.py measures it).
//
// meth_diff = 100.0 * (double(c) / double(c + d) - double(a) / double(a + b)), B minus A (treatment minus control), the two quotients
// first, then the difference, then the product; 0.0 where either group has no coverage.
//
// What is refused (DIFF_E_*): an entry of a count matrix that is negative, or 2^26 or more; a pooled margin (a + b, c + d, a + c, b + d)
// of 2^26 or more.  Below that the products above stay below 2^52.
//
// Plain C++ as mdk_unite_core.h: it compiles for the device (mdk_diff.hip) and for the host (tools/diff_emu.cpp), which is how it is
// tested without a GPU.
#ifndef MDK_DIFF_CORE_H
#define MDK_DIFF_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define MDK_DIFF __host__ __device__ __forceinline__
#else
#define MDK_DIFF static inline
#endif
#if defined(__clang__)
#define MDK_DIFF_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MDK_DIFF_NO_CONTRACT          // (gcc: built with -ffp-contract=off, tools/diff_emu)
#endif

enum { DIFF_E_NEGATIVE = 1, DIFF_E_ENTRY = 2, DIFF_E_MARGIN = 4 };
enum { DIFF_MAX_SAMPLES = 1024 };
#define DIFF_LIMIT (1ll << 26)            // entries and margins stay below
#define DIFF_MAX_SITES (1ll << 30)
#define DIFF_ONE 0x1p60                   // the mode's term
#define DIFF_TINY 0x1p-900                // a term of the walk below it: p = 0.0
#define DIFF_NEGLIGIBLE 0x1p-64           // a term below this much of the tail ends a direction

// what is wrong with one entry of a count matrix
MDK_DIFF uint32_t diff_entry_check(int64_t v) { return v < 0 ? DIFF_E_NEGATIVE : v >= DIFF_LIMIT ? DIFF_E_ENTRY : 0u; }
// ... and with a site's pooled counts (sums of checked entries: at most 1024 x 2^26, no overflow)
MDK_DIFF uint32_t diff_margin_check(int64_t a, int64_t b, int64_t c, int64_t d) {
    return a + b >= DIFF_LIMIT || c + d >= DIFF_LIMIT || a + c >= DIFF_LIMIT || b + d >= DIFF_LIMIT ? DIFF_E_MARGIN : 0u;
}

MDK_DIFF double diff_meth(int64_t a, int64_t b, int64_t c, int64_t d) {
    MDK_DIFF_NO_CONTRACT
    if(a + b == 0 || c + d == 0) return 0.0;
    const double fa = (double)a / (double)(a + b);
    const double fb = (double)c / (double)(c + d);
    const double x = fb - fa;
    return 100.0 * x;
}

// a site's margins and support.  The integers are below 2^26, so 32 bits hold them and a product of two is one widening multiplication
struct diff_site { int32_t a, n, K, M, lo, hi, mode; };
MDK_DIFF double diff_product(int32_t x, int32_t y) { return (double)((int64_t)x * (int64_t)y); }

// the term of table k + 1 from the term r of table k, and of table k - 1
MDK_DIFF double diff_up(const diff_site &s, double r, int32_t k) {
    MDK_DIFF_NO_CONTRACT
    const double t = r * diff_product(s.K - k, s.n - k);
    return t / diff_product(k + 1, s.M - s.n + k + 1);
}
MDK_DIFF double diff_down(const diff_site &s, double r, int32_t k) {
    MDK_DIFF_NO_CONTRACT
    const double t = r * diff_product(k, s.M - s.n + k);
    return t / diff_product(s.K - k + 1, s.n - k + 1);
}

// x / y of 64-bit integers, 0 <= x <= 2^52 and 0 < y < 2^28 (the mode's): the quotient of the two as doubles -- both are exact, the quotient
// is below 2^53 and at most half a unit off -- put right in integers.  The device has no 64-bit integer division: it would make one of
// some hundred instructions, as much as several terms
MDK_DIFF int64_t diff_quotient(int64_t x, int64_t y) {
    int64_t q = (int64_t)((double)x / (double)y);
    if(q * y > x) q--;
    else if((q + 1) * y <= x) q++;
    return q;
}

// the p-value of the table (a, b, c, d), its margins checked; *steps (if given): the terms that were added to the sums
MDK_DIFF double diff_pvalue(int64_t a, int64_t b, int64_t c, int64_t d, uint32_t *steps) {
    MDK_DIFF_NO_CONTRACT
    diff_site s;
    s.a = (int32_t)a; s.n = (int32_t)(a + b); s.K = (int32_t)(a + c); s.M = (int32_t)(b + d);
    s.lo = s.n - s.M > 0 ? s.n - s.M : 0; s.hi = s.n < s.K ? s.n : s.K;
    if(steps) *steps = 0;
    if(s.lo == s.hi) return 1.0;
    const int64_t mode = diff_quotient((int64_t)(s.n + 1) * (int64_t)(s.K + 1), (int64_t)s.n + c + d + 2);
    s.mode = mode < s.lo ? s.lo : mode > s.hi ? s.hi : (int32_t)mode;
    // the walk to the observed table
    int32_t k = s.mode; double r = DIFF_ONE;
    while(k != s.a) {
        if(s.a > k) { r = diff_up(s, r, k); k++; }
        else { r = diff_down(s, r, k); k--; }
        if(r < DIFF_TINY) return 0.0;
    }
    const double thr = r * (1.0 + 1e-7);
    double tail = 0.0, total = 0.0; uint32_t added = 0;
    // upward from the mode
    k = s.mode; r = DIFF_ONE;
    for(;;) {
        total = total + r;
        if(r <= thr) tail = tail + r;
        added++;
        if(k == s.hi || (s.a <= k && r <= thr && r < DIFF_NEGLIGIBLE * tail)) break;
        r = diff_up(s, r, k); k++;
    }
    // downward from mode - 1
    if(s.mode > s.lo) {
        r = diff_down(s, DIFF_ONE, s.mode); k = s.mode - 1;
        for(;;) {
            total = total + r;
            if(r <= thr) tail = tail + r;
            added++;
            if(k == s.lo || (s.a >= k && r <= thr && r < DIFF_NEGLIGIBLE * tail)) break;
            r = diff_down(s, r, k); k--;
        }
    }
    if(steps) *steps = added;
    const double q = tail / total;
    return q < 1.0 ? q : 1.0;
}
#endif
