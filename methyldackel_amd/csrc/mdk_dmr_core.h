// mdk_dmr_core.h -- significant neighbouring sites joined into regions: which rows are candidates, where a chain of them breaks, what a
// region reports, which regions are kept, and what is refused (csrc/mdk_dmr.hip: Diff.dmrs).
//
// The input is n rows (n at most 2^30), strictly ascending in (contig, start): contig, start, end (int32), the groups' pooled counts
// a = nmeth_a, b = nunmeth_a, c = nmeth_b, d = nunmeth_b (int64, as mdk_diff_core.h names them) and a mask sig (uint8, nonzero: the caller
// calls the row significant).  The parameters: max_gap >= 0 in bases, max_skip >= 0 in rows, min_sites >= 1, min_diff >= 0.0 in percent.
// No double of the rows is read: a row's direction comes from its four counts.
//   direction   dir(i) = the sign of c (a + b) - a (c + d), in int64: every count is below 2^26, so the products are below 2^53 and the
//               sign is exact.  +1: group B is the more methylated
//   candidates  row i is a candidate if sig[i] is set, a + b > 0, c + d > 0 and dir(i) != 0.  A significant row without coverage in a
//               group, or with equal fractions, is none: it is a skipped row like any other
//   chains      for a candidate i let p be the largest candidate row below i.  i CONTINUES p's region iff contig[i] == contig[p],
//               dir(i) == dir(p), start[i] - start[p] <= max_gap and i - p - 1 <= max_skip.  Otherwise i is a HEAD, and so is the first
//               candidate.  A raw region runs from a head f to the last candidate l before the next head, or to the last candidate of all
//   a region    contig[f], start[f], end[l]; nsites = l - f + 1, every row of the span, significant or not; nsig = the candidates of the
//               span; direction = dir(f); the four sums of a, b, c, d over ALL rows f .. l; meth_diff = diff_meth(sums) and pvalue =
//               diff_pvalue(sums) of mdk_diff_core.h: the bits mdk.diff_counts gives for the same four numbers
//   the filter  a raw region is kept iff nsig >= min_sites, |meth_diff| >= min_diff, and the sign of the pooled c (a + b) - a (c + d)
//               equals direction: pooled sums can reverse the sign of every one of their rows (Simpson's paradox), and such a region
//               is dropped, not reported against its own direction.  Kept regions come out in ascending order
// What is refused (DMR_E_*, the first three are DIFF_E_*): of a row, looking at rows i - 1 and i alone -- a negative count, a count of
// 2^26 or more, rows not strictly ascending in (contig, start), a contig index outside 0 .. n_contigs - 1 --; of a raw region, when no
// row is refused -- pooled margins that diff_margin_check refuses, checked before the filter, so that the answer does not depend on
// min_sites.  The refusal that is reported is the one of the smallest row (a region's: its first row), of a row with several the lowest
// bit.
//
// How the kernels find this (and tools/dmr_emu.cpp walks the same way): a byte of DMR_CODE_* per row; the previous candidate of a row
// from the 64 rows of its wavefront as a mask (dmr_prev_in_mask), from the wavefronts before it, from the blocks before it; the span
// [f, l] as whole blocks of DMR_ROWS rows from prefix sums plus the rows at its two ends (rgn_split_range of mdk_region_core.h).
//
// Plain C++ as mdk_diff_core.h: it compiles for the device (mdk_dmr.hip) and for the host (tools/dmr_emu.cpp), which is how it is tested
// without a GPU.
#ifndef MDK_DMR_CORE_H
#define MDK_DMR_CORE_H
#include <stdint.h>
#include "mdk_diff_core.h"
#include "mdk_region_core.h"

#if defined(__HIPCC__)
#define MDK_DMR __host__ __device__ __forceinline__
#else
#define MDK_DMR static inline
#endif

enum { DMR_E_NEGATIVE = DIFF_E_NEGATIVE, DMR_E_ENTRY = DIFF_E_ENTRY, DMR_E_MARGIN = DIFF_E_MARGIN, DMR_E_ORDER = 8, DMR_E_CONTIG = 16 };
enum { DMR_ROWS = RGN_ROWS };                                             // rows of a block of the tables
enum { DMR_CODE_NONE = 0, DMR_CODE_UP = 1, DMR_CODE_DOWN = 2 };           // a row's byte: no candidate, a candidate of direction +1, of -1
#define DMR_MAX_ROWS (1ll << 30)
#define DMR_NO_ROW (-1)                                                   // "no candidate" where a row index is expected
#define DMR_NO_PLACE 0xffffffffu                                          // a raw region that is not kept has no place in the result

// the sign of c (a + b) - a (c + d): of checked entries, or of sums whose margins are checked
MDK_DMR int dmr_dir(int64_t a, int64_t b, int64_t c, int64_t d) {
    const int64_t x = c * (a + b) - a * (c + d);
    return x > 0 ? 1 : x < 0 ? -1 : 0;
}
MDK_DMR int dmr_code_dir(uint32_t code) { return code == DMR_CODE_UP ? 1 : code == DMR_CODE_DOWN ? -1 : 0; }

// what is wrong with row i behind row (pcontig, pstart); has_prev 0 for the table's first row
MDK_DMR uint32_t dmr_row_check(int has_prev, int32_t pcontig, int32_t pstart, int32_t contig, int32_t start, int32_t n_contigs,
                               int64_t a, int64_t b, int64_t c, int64_t d) {
    uint32_t err = diff_entry_check(a) | diff_entry_check(b) | diff_entry_check(c) | diff_entry_check(d);
    if(contig < 0 || contig >= n_contigs) err |= DMR_E_CONTIG;
    if(has_prev && !(pcontig < contig || (pcontig == contig && pstart < start))) err |= DMR_E_ORDER;
    return err;
}

// the row's byte, its entries checked
MDK_DMR uint32_t dmr_code(int sig, int64_t a, int64_t b, int64_t c, int64_t d) {
    if(!sig || a + b == 0 || c + d == 0) return DMR_CODE_NONE;
    const int dir = dmr_dir(a, b, c, d);
    return dir > 0 ? DMR_CODE_UP : dir < 0 ? DMR_CODE_DOWN : DMR_CODE_NONE;
}

// of 64 neighbouring rows whose candidates are the set bits of `mask`: the highest candidate below row `lane`, or -1
MDK_DMR int dmr_prev_in_mask(uint64_t mask, int lane) {
    const uint64_t below = mask & ((1ull << lane) - 1ull);
    return below ? 63 - __builtin_clzll(below) : -1;
}
MDK_DMR int dmr_last_in_mask(uint64_t mask) { return mask ? 63 - __builtin_clzll(mask) : -1; }

// does candidate i continue the region of the candidate p before it?
MDK_DMR int dmr_continues(int32_t pcontig, int32_t pstart, uint32_t pcode, int32_t p, int32_t contig, int32_t start, uint32_t code, int32_t i,
                          int32_t max_gap, int32_t max_skip) {
    return pcontig == contig && pcode == code && (int64_t)start - (int64_t)pstart <= (int64_t)max_gap && i - p - 1 <= max_skip;
}

// is the raw region kept?  Its margins are checked
MDK_DMR int dmr_keep(int32_t nsig, int64_t a, int64_t b, int64_t c, int64_t d, int dir, int32_t min_sites, double min_diff) {
    const double x = diff_meth(a, b, c, d);
    return nsig >= min_sites && (x < 0.0 ? -x : x) >= min_diff && dmr_dir(a, b, c, d) == dir;
}
#endif
