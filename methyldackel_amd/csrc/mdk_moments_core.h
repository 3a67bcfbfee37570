// mdk_moments_core.h -- how alike the samples of a united table are: the pairwise sample moments, exact in integers, and their centring
// into the numerators of covariance and correlation, and nothing else (csrc/mdk_moments.hip: mdk.sample_moments, Cohort.moments).
//
// The inputs are two [S, n] count matrices, sample-major, and min_depth (1 to 2^26 - 1).
//   covered   cell (s, k) is covered if d = nmeth + nunmeth >= min_depth
//   level     its level is the integer x = (2 * nmeth * 65536 + d) / (2 * d), rounded down: the methylated fraction in units of 2^-16,
//             rounded half up, 0 <= x <= 65536.  An uncovered cell has x = 0 and takes part in nothing.  (16 bits: at any depth below
//             2^26 the level's own sampling error is thousands of times the 2^-17 rounding step)
//   refused   MOM_E_*, mdk_diff_core.h's first two: an entry that is negative, or 2^26 or more -- the first (smallest) such site is named
// Over the sites k where BOTH i and j are covered (pairwise-complete observations) four [S, S] int64 matrices are formed:
//   n[i][j]    the number of such sites (symmetric)
//   sx[i][j]   the sum of x_i over them (not symmetric: sx[j][i] is the sum of x_j over the same sites)
//   sxx[i][j]  the sum of x_i^2 over them
//   sxy[i][j]  the sum of x_i * x_j over them (symmetric)
// The diagonals are each sample's own covered count, sum and sum of squares.  With n <= 2^30 sites every sum fits an int64 with room to
// spare: sx <= 2^46, sxx and sxy <= 2^62.  The sums are integers, so any tiling and any order of accumulation -- atomic adds included --
// gives the same matrices, and the moments of disjoint site sets add cell by cell.  That is why centring is a step of its own:
//   cxy[i][j] = n[i][j] * sxy[i][j] - sx[i][j] * sx[j][i]
//   vxx[i][j] = n[i][j] * sxx[i][j] - sx[i][j]^2
// both formed exactly in 128-bit integers -- |.| < 2^93 given n <= 2^30, sx <= n * 65536, sxx and sxy <= n * 2^32, which mom_sums_check
// asks (MOM_E_SUM_*) -- and rounded ONCE to a double, to nearest and ties to even, by mom_to_double: leading zeros, a shift and the
// bits shifted out, written out here, so neither side calls a conversion routine of its runtime.  128-bit products are used, no
// 128-bit division and no cast of a 128-bit integer to a double.
// covariance = cxy / (n (n - 1)) / 2^32 and correlation = cxy / sqrt(vxx[i][j] * vxx[j][i]) are the caller's (SampleMoments).
//
// The level's one division is a quotient of two floats put right in integers, as diff_quotient puts one of doubles right: the device
// has no 64-bit integer division, and a division of doubles costs several times one of floats -- measured, it and not the sums bounded
// the kernels.  m and d as floats, their quotient, the product with 2^16 (exact) and the sum with 0.5 are each within 2^-24 of what
// they round, so the estimate is within 65536.5 * 4 * 2^-24 < 0.02 of the exact m / d * 65536 + 1 / 2 and its integer part at most one
// off the level; the two 64-bit comparisons behind it decide, so the result is the rule's integer whatever the estimate's last bits.
//
// Plain C++ as mdk_diff_core.h: it compiles for the device (mdk_moments.hip) and for the host (tools/moments_emu.cpp), which is how it
// is tested without a GPU.  No floating-point sum or product is formed, so contraction has nothing to change.
#ifndef MDK_MOMENTS_CORE_H
#define MDK_MOMENTS_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define MDK_MOM __host__ __device__ __forceinline__
#else
#define MDK_MOM static inline
#endif

enum { MOM_E_NEGATIVE = 1, MOM_E_ENTRY = 2 };                                        // of an entry of a count matrix
enum { MOM_E_SUM_NEGATIVE = 1, MOM_E_SUM_N = 2, MOM_E_SUM_SX = 4, MOM_E_SUM_SQ = 8 };   // of a cell of the four sums
enum { MOM_MAX_SAMPLES = 1024 };
#define MOM_LIMIT (1ll << 26)             // entries and min_depth stay below
#define MOM_MAX_SITES (1ll << 30)
#define MOM_ONE 65536                     // the level of a cell all methylated

MDK_MOM uint32_t mom_entry_check(int64_t v) { return v < 0 ? MOM_E_NEGATIVE : v >= MOM_LIMIT ? MOM_E_ENTRY : 0u; }
// (site << 8 | the refusal's bit number): the smallest is the refusal that is reported
MDK_MOM uint64_t mom_refusal_key(int64_t at, uint32_t err) {
    uint32_t bit = 0;
    while(!((err >> bit) & 1u)) bit++;
    return ((uint64_t)at << 8) | bit;
}

// the level of a checked, covered cell: d >= 1
MDK_MOM uint32_t mom_level(int64_t m, int64_t d) {
    const int64_t x = 2 * m * MOM_ONE + d, y = 2 * d;
    int64_t q = (int64_t)((float)m / (float)d * 65536.0f + 0.5f);
    if(q * y > x) q--;
    else if((q + 1) * y <= x) q++;
    return (uint32_t)q;
}
// a cell as the kernels keep it: the level in bits 0 to 16 and bit MOM_COVERED_BIT set if it is covered; 0 for an uncovered or a refused one
#define MOM_COVERED_BIT 20
#define MOM_LEVEL_MASK 0x1ffffu
MDK_MOM uint32_t mom_cell(int64_t m, int64_t u, int64_t min_depth, uint32_t *err) {
    const uint32_t e = mom_entry_check(m) | mom_entry_check(u);
    *err |= e;
    const int64_t d = m + u;
    if(e || d < min_depth) return 0u;
    return mom_level(m, d) | (1u << MOM_COVERED_BIT);
}

// what is wrong with a cell of the four sums: what the 128-bit bounds rest on
MDK_MOM uint32_t mom_sums_check(int64_t n, int64_t sx, int64_t sxx, int64_t sxy) {
    if(n < 0 || sx < 0 || sxx < 0 || sxy < 0) return MOM_E_SUM_NEGATIVE;
    if(n > MOM_MAX_SITES) return MOM_E_SUM_N;
    if(sx > n * MOM_ONE) return MOM_E_SUM_SX;
    if(sxx > (n << 32) || sxy > (n << 32)) return MOM_E_SUM_SQ;
    return 0u;
}

// v, |v| < 2^127, as the nearest double, ties to even.  The magnitude is held as two 64-bit halves
MDK_MOM double mom_to_double(__int128 v) {
    const uint64_t sign = v < 0 ? 1ull << 63 : 0;
    const unsigned __int128 mag = v < 0 ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
    const uint64_t hi = (uint64_t)(mag >> 64), lo = (uint64_t)mag;
    uint64_t bits = sign;
    if(hi | lo) {
        const int top = hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo);       // the leading one's place
        uint64_t mant;                                                                   // 53 bits, the leading one at bit 52
        if(top <= 52) mant = lo << (52 - top);
        else {
            const int shift = top - 52;                                                  // 1 to 75 bits go
            const unsigned __int128 kept = mag >> shift, rest = mag - (kept << shift), half = (unsigned __int128)1 << (shift - 1);
            mant = (uint64_t)kept;
            if(rest > half || (rest == half && (mant & 1))) mant++;                      // (2^53: the sum below carries into the exponent)
        }
        bits |= ((uint64_t)(top + 1023) << 52) + (mant - (1ull << 52));
    }
    double r;
    __builtin_memcpy(&r, &bits, 8);
    return r;
}

// the two centred numerators of a checked cell: its own n, sx, sxx, sxy and sx of the transposed cell
MDK_MOM double mom_cxy(int64_t n, int64_t sxy, int64_t sx, int64_t sx_t) { return mom_to_double((__int128)n * sxy - (__int128)sx * sx_t); }
MDK_MOM double mom_vxx(int64_t n, int64_t sxx, int64_t sx) { return mom_to_double((__int128)n * sxx - (__int128)sx * sx); }
#endif
