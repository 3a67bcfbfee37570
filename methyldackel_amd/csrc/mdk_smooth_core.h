// mdk_smooth_core.h -- kernel-weighted methylation levels: every site's counts replaced by a weighted sum over the neighbouring sites of
// its contig, per sample; which rows a site's window holds, what each of them weighs, the order of the sum, and what is refused
// (csrc/mdk_smooth.hip: mdk.smooth_counts, Cohort.smooth, Calls.smooth).
//
// Inputs      contig, start: int32[n], strictly ascending in (contig, start).  nmeth, nunmeth: [S, n], sample-major, int32 or int64.
//             1 <= S <= 1024, 0 <= n <= 2^30.  half_bases in [0, 2^20], min_sites in [1, 2^16], kernel SMO_TRICUBE (0) or SMO_FLAT (1).
//
// The window of site i, in integers alone -- BSmooth's rule: at least half_bases to either side AND at least min_sites sites.  Let
// [c0, c1) be the rows of i's contig (smo_contig_run: two bounds on `contig`), x = start, k = min(min_sites, c1 - c0).
//   d_k       the distance from x_i to its k-th nearest site of the contig, i itself counted first at distance 0.  The rows ascend, so
//             the k nearest form a run that holds i: d_k = min over l in [max(c0, i - k + 1), min(i, c1 - k)] of
//             max(x_i - x_l, x_{l+k-1} - x_i).  The first falls and the second rises with l, so smo_kth_distance bisects for the first
//             l where the second is at least the first and takes the smaller of that l's value and its predecessor's
//   half_i    max(half_bases, d_k)
//   lo_i      the first row >= c0 with x >= x_i - half_i; hi_i one past the last row < c1 with x <= x_i + half_i (64-bit comparisons);
//             nsites_i = hi_i - lo_i.  A window never crosses a contig, and lo_i <= i < hi_i
// Two facts the kernels rely on (tests/test_smooth_cpu.py checks both by brute force): lo and hi are non-decreasing in i, and a window
// holds at most max(2 half_bases + 1, 2 min_sites - 1) sites (smo_window_cap).
//
// The weight of row j in window i, d = |x_j - x_i| as an integer (smo_weight):
//   flat      1.0
//   tricube   d >= half_i: 0.0, decided by the INTEGER comparison, never by the doubles; half_i == 0: 1.0 (only d = 0 occurs);
//             otherwise inv = 1.0 / (double)half_i -- ONE division per site, not one per pair: smo_inverse --, r = (double)d * inv,
//             c = (r * r) * r, t = 1.0 - c, w = (t * t) * t.  For d < half_i <= 2^20 t > 0 and nothing is subnormal;
//             |w - (1 - (d/half)^3)^3| <= 32 * 2^-53 (on a grid of half <= 2^20 the worst seen is 3.5 * 2^-53).  A half above 2^20 --
//             a sparse stretch where min_sites decides -- follows the same statements.
//
// Per sample s: M = 0.0, D = 0.0; for j = lo_i .. hi_i - 1 ASCENDING: M = M + w * (double)m_sj, then D = D + w * (double)(m_sj + u_sj),
// the sum m + u formed in int64.  level = M / D if D > 0.0, otherwise the quiet NaN 0x7ff8000000000000 (smo_level); depth = D.
// IEEE doubles with *, /, + and - alone in that one order, no fused multiply-add (contraction is off in these functions; the host
// build uses -ffp-contract=off): the device, a host build of this header (tools/smooth_emu.cpp) and a restatement in Python floats
// (tests/smooth_rule.py) give the same bits, whatever the kernels' blocking.  With the flat kernel M and D are exact integers and
// level is the correctly rounded quotient of the integer sums.
//
// Outputs     level, depth: float64 [S, n]; nsites, half: int32 [n], shared by the samples.
//
// What is refused (SMO_E_*, a bit each): of a row, looking at rows i - 1 and i alone so that every workgroup finds its own -- not
// strictly ascending behind its predecessor, a negative contig or start (smo_row_check) --; of an entry -- negative, or 2^26 or more,
// mdk_diff_core.h's limit, so that everything that can be smoothed can be tested (smo_entry_check).  Reported is the smallest refused
// site, and of its bits the lowest (smo_refusal_key: the kernels take the minimum of these keys).  A refused call fails and its outputs
// are unspecified; whatever the table holds, nothing outside it is read: every search stays inside [0, n).
//
// Plain C++ as mdk_qdiff_core.h and mdk_region_core.h: it compiles for the device (mdk_smooth.hip) and for the host
// (tools/smooth_emu.cpp runs the kernels' blocking over it), which is how it is tested without a GPU.
#ifndef MDK_SMOOTH_CORE_H
#define MDK_SMOOTH_CORE_H
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MDK_SMO __host__ __device__ __forceinline__
#else
#define MDK_SMO static inline
#endif
#if defined(__clang__)
#define MDK_SMO_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MDK_SMO_NO_CONTRACT           // (gcc: built with -ffp-contract=off, tools/smooth_emu)
#endif

enum { SMO_E_ORDER = 1, SMO_E_POSITION = 2, SMO_E_NEGATIVE = 4, SMO_E_ENTRY = 8 };
enum { SMO_TRICUBE = 0, SMO_FLAT = 1 };
enum { SMO_MAX_SAMPLES = 1024, SMO_MAX_HALF_BASES = 1 << 20, SMO_MAX_MIN_SITES = 1 << 16 };
#define SMO_LIMIT (1ll << 26)             // entries stay below (mdk_diff_core.h's DIFF_LIMIT)
#define SMO_MAX_SITES (1ll << 30)
#define SMO_NAN_BITS 0x7ff8000000000000ull

// what is wrong with row (contig, start) behind row (pcontig, pstart); has_prev 0 for the table's first row
MDK_SMO uint32_t smo_row_check(int has_prev, int32_t pcontig, int32_t pstart, int32_t contig, int32_t start) {
    uint32_t err = 0;
    if(has_prev && !(pcontig < contig || (pcontig == contig && pstart < start))) err |= SMO_E_ORDER;
    if(contig < 0 || start < 0) err |= SMO_E_POSITION;
    return err;
}
// ... and with one entry of a count matrix
MDK_SMO uint32_t smo_entry_check(int64_t v) { return v < 0 ? (uint32_t)SMO_E_NEGATIVE : v >= SMO_LIMIT ? (uint32_t)SMO_E_ENTRY : 0u; }
// what a refusal `err` (not 0) of site i is reported as: the smallest key wins -- the smallest site, and of its bits the lowest
MDK_SMO uint64_t smo_refusal_key(int64_t i, uint32_t err) {
    uint32_t bit = 0;
    while(!(err >> bit & 1u)) bit++;
    return ((uint64_t)i << 8) | bit;
}

// the most sites a window holds
MDK_SMO int64_t smo_window_cap(int32_t half_bases, int32_t min_sites) {
    const int64_t a = 2 * (int64_t)half_bases + 1, b = 2 * (int64_t)min_sites - 1;
    return a > b ? a : b;
}

// [*c0, *c1): the rows of row i's contig.  About 2 log2(n) rows of `contig` are read, all inside [0, n)
MDK_SMO void smo_contig_run(const int32_t *contig, int64_t n, int64_t i, int64_t *c0, int64_t *c1) {
    const int32_t c = contig[i];
    int64_t a = 0, b = i;                                       // the first row of [0, i] that is not below c
    while(a < b) { const int64_t mid = a + ((b - a) >> 1); if(contig[mid] < c) a = mid + 1; else b = mid; }
    *c0 = a;
    a = i + 1; b = n;                                           // the first row of [i + 1, n] that is above c
    while(a < b) { const int64_t mid = a + ((b - a) >> 1); if(contig[mid] <= c) a = mid + 1; else b = mid; }
    *c1 = a;
}

// d_k: the distance from x_i to its k-th nearest site among rows [c0, c1), 1 <= k <= c1 - c0, c0 <= i < c1.  Rows [c0, c1) alone are read
MDK_SMO int64_t smo_kth_distance(const int32_t *x, int64_t c0, int64_t c1, int64_t i, int64_t k) {
    const int64_t la = i - k + 1 > c0 ? i - k + 1 : c0, lb = i < c1 - k ? i : c1 - k;          // la <= lb: the runs of k rows that hold i
    const int64_t xi = x[i];
    int64_t a = la, b = lb + 1;                                 // the first run whose right reach is at least its left reach; lb + 1: none
    while(a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if((int64_t)x[mid + k - 1] - xi >= xi - (int64_t)x[mid]) b = mid; else a = mid + 1;
    }
    int64_t d = INT64_MAX;
    if(a <= lb) d = (int64_t)x[a + k - 1] - xi;                 // (there the right reach is the larger)
    if(a > la) { const int64_t e = xi - (int64_t)x[a - 1]; if(e < d) d = e; }                  // (and before it the left)
    return d;
}

struct smo_window { int64_t half, lo, hi; };
// the window of site i of the contig's rows [c0, c1)
MDK_SMO smo_window smo_window_of(const int32_t *x, int64_t c0, int64_t c1, int64_t i, int32_t half_bases, int32_t min_sites) {
    smo_window w;
    const int64_t k = (int64_t)min_sites < c1 - c0 ? (int64_t)min_sites : c1 - c0;
    const int64_t dk = smo_kth_distance(x, c0, c1, i, k);
    w.half = dk > (int64_t)half_bases ? dk : (int64_t)half_bases;
    const int64_t xi = x[i], left = xi - w.half, right = xi + w.half;
    int64_t a = c0, b = i;                                      // the first row of [c0, i] at or past `left`
    while(a < b) { const int64_t mid = a + ((b - a) >> 1); if((int64_t)x[mid] < left) a = mid + 1; else b = mid; }
    w.lo = a;
    a = i + 1; b = c1;                                          // the first row of [i + 1, c1] past `right`
    while(a < b) { const int64_t mid = a + ((b - a) >> 1); if((int64_t)x[mid] <= right) a = mid + 1; else b = mid; }
    w.hi = a;
    return w;
}

// a site's one division
MDK_SMO double smo_inverse(int64_t half) {
    MDK_SMO_NO_CONTRACT
    return half > 0 ? 1.0 / (double)half : 0.0;
}
// the weight of a row at distance d >= 0 from the centre of a window of half-width `half`, inv = smo_inverse(half)
MDK_SMO double smo_weight(int32_t kernel, int64_t d, int64_t half, double inv) {
    MDK_SMO_NO_CONTRACT
    if(kernel == SMO_FLAT) return 1.0;
    if(half == 0) return 1.0;
    if(d >= half) return 0.0;
    const double r = (double)d * inv;
    const double c = (r * r) * r;
    const double t = 1.0 - c;
    return (t * t) * t;
}
// one row added to a sample's two sums: m = (double)nmeth, md = (double)(nmeth + nunmeth)
MDK_SMO void smo_add(double w, double m, double md, double *M, double *D) {
    MDK_SMO_NO_CONTRACT
    const double a = w * m, b = w * md;
    *M = *M + a;
    *D = *D + b;
}
MDK_SMO double smo_level(double M, double D) {
    MDK_SMO_NO_CONTRACT
    if(D > 0.0) return M / D;
    const uint64_t bits = SMO_NAN_BITS; double x;
    memcpy(&x, &bits, 8);
    return x;
}
#endif
