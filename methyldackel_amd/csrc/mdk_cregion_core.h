// mdk_cregion_core.h -- every sample's sums over intervals in one pass (csrc/mdk_cregion.hip: Cohort.regions).  The rule is
// mdk_region_core.h's, applied to sample s of the [S, n] matrices: cell (s, j) is the sum over the rows of interval j whose context and
// strand pass the masks and whose nmeth[s, i] + nunmeth[s, i] >= min_depth.  This header holds what the kernels and tools/cregion_emu.cpp
// share beyond that rule: where a cell lies, how the filter is cut in two, and how the samples and the work are dealt out.
//   a cell        (s, i) of an [S, n] matrix, and (s, j) of an [S, k] result, at s * n + i: 64 bits, S * n and S * k both pass 2^32
//   the filter    the context and strand part depends on the site alone and is taken once, as a byte per site (crg_site_passes); the
//                 depth part is the cell's (crg_cell_counts).  Together they are rgn_counts, which is how crg_site_passes is written
//   block table   per sample nb + 1 entries a column, nb = ceil(n / RGN_ROWS): the totals of the blocks of RGN_ROWS rows, scanned in
//                 place into exclusive prefixes with the sum of all as entry nb.  Three columns -- nsites (uint32), nmeth, nunmeth
//                 (int64): 20 bytes per 256 cells --, entry (s, b) at s * (nb + 1) + b
//   a range       [lo, hi) split by rgn_split_range: whole blocks from two prefix entries, at most 255 + 255 rows read directly
//   the samples   dealt in batches of `sample_block`: a workgroup that takes a block of sites loads the sites' bytes once a batch
//   the scan      CRG_SCAN_ROUND entries a round with a carry between the rounds, a sample's three columns by one workgroup
// Plain C++ for the device and the host, as mdk_region_core.h, which is included and not changed.
#ifndef MDK_CREGION_CORE_H
#define MDK_CREGION_CORE_H
#include "mdk_region_core.h"

enum { CRG_SCAN_WG = 1024, CRG_SCAN_PER = 4, CRG_SCAN_ROUND = CRG_SCAN_WG * CRG_SCAN_PER, CRG_BATCH_MAX = 64 };

// the offset of cell (s, i) in a matrix of n entries a sample
MDK_RGN int64_t crg_cell(int32_t s, int64_t i, int64_t n) { return (int64_t)s * n + i; }

// blocks of RGN_ROWS rows in a table of n, and the offset of entry (s, b), b in [0, nb], of a column of the block table
MDK_RGN int64_t crg_blocks(int64_t n) { return (n + RGN_ROWS - 1) / RGN_ROWS; }
MDK_RGN int64_t crg_entry(int32_t s, int64_t b, int64_t nb) { return (int64_t)s * (nb + 1) + b; }

// the site's part of the filter: do the context and the strand pass?  (rgn_counts of a cell that no depth cuts)
MDK_RGN uint8_t crg_site_passes(const rgn_filter &f, int32_t ctx, int32_t strand) {
    rgn_filter g = f; g.min_depth = 0;
    return (uint8_t)rgn_counts(g, 0, 0, ctx, strand);
}
// the cell's part: does cell (m, u) of a site whose byte is `passes` count?
MDK_RGN int crg_cell_counts(uint8_t passes, int32_t m, int32_t u, int32_t min_depth) { return passes && (int64_t)m + (int64_t)u >= (int64_t)min_depth; }

// the batches of at most `sample_block` samples, and the samples [s0, s1) of batch t
MDK_RGN int32_t crg_batches(int32_t S, int32_t sample_block) { return (S + sample_block - 1) / sample_block; }
MDK_RGN void crg_batch(int32_t t, int32_t S, int32_t sample_block, int32_t &s0, int32_t &s1) {
    s0 = t * sample_block; s1 = s0 + sample_block < S ? s0 + sample_block : S;
}

// a launch of `items` work items under the grid cap: the workgroups (at least one), each taking items w, w + grid, ...
MDK_RGN int64_t crg_grid(int64_t items, int32_t max_workgroups) { return items < 1 ? 1 : items < max_workgroups ? items : max_workgroups; }

// what the sum kernel keeps of an interval across its sample loop
struct crg_range { uint32_t lo, hi; rgn_split sp; };
MDK_RGN crg_range crg_range_of(uint32_t lo, uint32_t hi) { crg_range r; r.lo = lo; r.hi = hi; r.sp = rgn_split_range(lo, hi); return r; }
#endif
