// mdk_profile_core.h -- the count profile of a table: per sample and group of sites the histogram of the depths, the histogram of the
// methylation levels, the two sums and the largest depth, exact in integers, and nothing else (csrc/mdk_profile.hip: mdk.count_profile,
// Calls.profile, Cytosines.profile, Cohort.profile).
//
// The inputs are two [S, n] count matrices, sample-major, an optional column `group` of n bytes with the group count G (1 to 4; without
// the column every site is in group 0), min_depth (1 to 2^26 - 1), depth_bins B (1 to 4096) and level_bins L (1 to 256).  Per cell
// (s, k), with m = nmeth[s][k], u = nunmeth[s][k], d = m + u and g = group[k]:
//   refused   mdk_moments_core.h's two, MOM_E_NEGATIVE and MOM_E_ENTRY -- an entry that is negative, or 2^26 or more --, and
//             PROF_E_GROUP: group[k] >= G, which refuses every cell of the site.  The first (smallest) such site is named, and at one
//             site the lowest code.  A refused cell is counted nowhere
//   depth     depth_hist[s][g][min(d, B)] += 1 for EVERY cell, d = 0 included: bin b < B holds the cells of depth exactly b, bin B, the
//             last of B + 1, the cells of depth B or more.  max_depth[s][g] is the largest d of any cell, 0 where there is none
//   covered   a cell is covered if d >= min_depth.  Then level_hist[s][g][min(L - 1, floor(m L / d))] += 1 -- L equal bins of the
//             methylated fraction, a cell all methylated in the last --, nmeth_sum[s][g] += m and nunmeth_sum[s][g] += u
// All five outputs are int64: [S, G, B + 1], [S, G, L] and three [S, G].  With n <= 2^30 sites and entries below 2^26 a bin stays below
// 2^31 and a sum below 2^56.  Counts and sums are integers and the maximum is a maximum, so any blocking and any order of accumulation
// -- atomic adds included -- gives the same tensors, and the profiles of disjoint site sets add cell by cell, max_depth by maximum.
//
// The level bin's one division is a quotient of floats put right in integers, as mom_level's is (the device has no 64-bit integer
// division): m, L and d as floats, the product and the quotient -- or the reciprocal and the product with it -- are each within 2^-23
// of what they round, so the estimate is within 257 * 5 * 2^-23 < 2^-12 of the exact m L / d and its integer part at most one off the
// floor; the two comparisons l d <= m L < (l + 1) d behind it decide, so the bin is the rule's integer whatever the estimate's last
// bits.  m L < 2^34 and (l + 1) d < 2^36: nothing here passes 64 bits.  No floating-point value reaches a result.
//
// Plain C++ as mdk_moments_core.h: it compiles for the device (mdk_profile.hip) and for the host (tools/profile_emu.cpp), which is how
// it is tested without a GPU.
#ifndef MDK_PROFILE_CORE_H
#define MDK_PROFILE_CORE_H
#include "mdk_moments_core.h"

enum { PROF_E_GROUP = 4 };                                       // after MOM_E_NEGATIVE and MOM_E_ENTRY: a site's group is G or more
enum { PROF_MAX_GROUPS = 4, PROF_MAX_DEPTH_BINS = 4096, PROF_MAX_LEVEL_BINS = 256 };

// floor(m L / d) of a checked cell with d >= 1, 0 <= m <= d < 2^27, 1 <= L <= 256: 0 to L.  Everything is 32 bits wide but the three
// products, each one multiply of two 32-bit words into 64.  On the device the quotient's estimate is a product with the reciprocal, one
// unit in the last place off at the most and so still within 2^-12 of m L / d: the comparisons make the same integer of either estimate
MDK_MOM uint32_t prof_level_floor(uint32_t m, uint32_t d, uint32_t L) {
    const uint64_t x = (uint64_t)m * L;
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t q = (uint32_t)((float)m * (float)L * __builtin_amdgcn_rcpf((float)d));
#else
    uint32_t q = (uint32_t)((float)m * (float)L / (float)d);
#endif
    if((uint64_t)q * d > x) q--;
    else if((uint64_t)(q + 1u) * d <= x) q++;
    return q;
}
// a cell as the kernels keep it: the depth bin in bits 0 to 12, the level bin in bits 16 to 23 and PROF_COVERED_BIT set if the cell is
// covered.  PROF_REFUSED, with the codes added to *err, for a cell with a refused entry, which is counted nowhere.  (Both entries
// are within 0 and 2^26 - 1 exactly if no bit from 26 up is set in either: one comparison on the way that is taken)
#define PROF_COVERED_BIT 15
#define PROF_DEPTH_MASK 0x1fffu
#define PROF_REFUSED 0xffffffffu
MDK_MOM uint32_t prof_cell(int64_t m, int64_t u, int64_t min_depth, int32_t B, int32_t L, uint32_t *err) {
    if(((uint64_t)m | (uint64_t)u) >= (uint64_t)MOM_LIMIT) { *err |= mom_entry_check(m) | mom_entry_check(u); return PROF_REFUSED; }
    const uint32_t a = (uint32_t)m, d = a + (uint32_t)u;
    const uint32_t db = d < (uint32_t)B ? d : (uint32_t)B;
    if(d < (uint32_t)min_depth) return db;
    const uint32_t l = prof_level_floor(a, d, (uint32_t)L);
    return db | (1u << PROF_COVERED_BIT) | ((l < (uint32_t)L - 1u ? l : (uint32_t)L - 1u) << 16);
}
MDK_MOM uint32_t prof_group_check(uint32_t g, int32_t G) { return g >= (uint32_t)G ? (uint32_t)PROF_E_GROUP : 0u; }
#endif
