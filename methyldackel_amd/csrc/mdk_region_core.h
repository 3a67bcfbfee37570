// mdk_region_core.h -- sums of rows over intervals: which rows an interval holds, which of them count, and what is refused
// (csrc/mdk_regions.hip: Calls.regions, Cytosines.regions).
//
// The n rows are strictly ascending in (contig, start), so the rows of one interval are one contiguous range of the table.  An interval
// (c, s, e) is half-open and 0-based, as a BED line; intervals come in any order and may overlap, nest or repeat.
//   the range     lo = the number of rows with (contig, start) < (c, s), hi = the number with (contig, start) < (c, e); its rows are [lo, hi)
//                 (rgn_lower_bound, a binary search).  A row belongs to the interval that holds its START -- a merged row, wider than one
//                 base, too --, so the windows of a tiling count every row once and their sums add up to the table's
//   which count   bit `context` of context_mask is set; the strand is allowed by strand_mask (bit 0: +1, bit 1: -1, bit 2: 0, a merged
//                 row); nmeth + nunmeth >= min_depth, the sum formed in 64 bits (rgn_counts)
//   the result    nsites (rows counted, int32: n is at most 2^30), nmeth and nunmeth (int64: a contig at high depth passes 2^31)
// What is refused (RGN_E_*): of a row, looking at rows i - 1 and i alone, so that every workgroup finds its own -- not strictly ascending,
// a contig index outside the names, a context above 2 --; of an interval -- a contig outside the names, start < 0 or end < start.  An
// empty interval (start == end) is valid and so is one without rows: zeros.
//
// Plain C++ as mdk_merge_core.h: it compiles for the device (mdk_regions.hip) and for the host (tools/region_emu.cpp runs the kernels'
// blocking over it), which is how it is tested without a GPU.
#ifndef MDK_REGION_CORE_H
#define MDK_REGION_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define MDK_RGN __host__ __device__ __forceinline__
#else
#define MDK_RGN static inline
#endif

enum { RGN_E_ORDER = 1, RGN_E_CONTIG = 2, RGN_E_CONTEXT = 4, RGN_E_IV_CONTIG = 8, RGN_E_IV_RANGE = 16 };
enum { RGN_STRAND_PLUS = 1, RGN_STRAND_MINUS = 2, RGN_STRAND_NONE = 4, RGN_ROWS = 256 };       // RGN_ROWS: rows of a block of the prefix table

struct rgn_filter { uint32_t context_mask, strand_mask; int32_t min_depth; };

// does the row count?  (a context above 2 never does: the row is refused)
MDK_RGN int rgn_counts(const rgn_filter &f, int32_t m, int32_t u, int32_t ctx, int32_t strand) {
    const uint32_t sbit = strand > 0 ? RGN_STRAND_PLUS : strand < 0 ? RGN_STRAND_MINUS : RGN_STRAND_NONE;
    return (uint32_t)ctx <= 2u && (f.context_mask >> ctx & 1u) && (f.strand_mask & sbit) && (int64_t)m + (int64_t)u >= (int64_t)f.min_depth;
}

// what is wrong with row (contig, start, ctx) behind row (pcontig, pstart); has_prev 0 for the table's first row
MDK_RGN uint32_t rgn_row_check(int has_prev, int32_t pcontig, int32_t pstart, int32_t contig, int32_t start, int32_t ctx, int32_t n_contigs) {
    uint32_t err = 0;
    if((uint32_t)ctx > 2u) err |= RGN_E_CONTEXT;
    if(contig < 0 || contig >= n_contigs) err |= RGN_E_CONTIG;
    if(has_prev && !(pcontig < contig || (pcontig == contig && pstart < start))) err |= RGN_E_ORDER;
    return err;
}

// what is wrong with an interval
MDK_RGN uint32_t rgn_interval_check(int32_t c, int32_t s, int32_t e, int32_t n_contigs) {
    return (c < 0 || c >= n_contigs ? (uint32_t)RGN_E_IV_CONTIG : 0u) | (s < 0 || e < s ? (uint32_t)RGN_E_IV_RANGE : 0u);
}

// the number of rows among [from, n) with (contig, start) < (c, s), plus `from`: rows [0, from) are known to lie below.  Reads rows of
// [from, n) only, about log2(n - from) of them; in a table that is not ascending the result is still inside [from, n]
MDK_RGN uint32_t rgn_lower_bound(const int32_t *contig, const int32_t *start, uint32_t from, uint32_t n, int32_t c, int32_t s) {
    uint32_t lo = from, hi = n;
    while(lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const int32_t mc = contig[mid];
        // (the start is loaded only where it decides)
        if(mc < c || (mc == c && start[mid] < s)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// how the range [lo, hi) is put together: whole blocks [b0, b1) of RGN_ROWS rows from the prefix table, rows [lo, a_end) and [b_beg, hi) --
// at most RGN_ROWS - 1 each -- read directly.  Without a block boundary in [lo, hi] the first of them is all of it.  lo <= hi: hi is
// searched from lo on
struct rgn_split { uint32_t a_end, b_beg, b0, b1; };
MDK_RGN rgn_split rgn_split_range(uint32_t lo, uint32_t hi) {
    rgn_split s;
    s.b0 = (lo + RGN_ROWS - 1) / RGN_ROWS; s.b1 = hi / RGN_ROWS;
    if(s.b0 <= s.b1) { s.a_end = s.b0 * RGN_ROWS; s.b_beg = s.b1 * RGN_ROWS; }
    else { s.a_end = hi; s.b_beg = hi; s.b0 = s.b1 = 0; }
    return s;
}
#endif
