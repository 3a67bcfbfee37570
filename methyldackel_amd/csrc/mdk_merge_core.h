// mdk_merge_core.h -- the `mergeContext` command's rule over ROWS instead of text: what happens to one per-strand call, given the row before
// it and the row after it (csrc/mdk_merge.hip: Calls.merge_context, Cytosines.merge_context).
//
// The rows are strictly ascending in (contig, start), each the call of one cytosine: [start, start + 1), its counts, its context t (0 CpG,
// 1 CHG, 2 CHH) and its strand (+1 a C, -1 a G).  The host tool (csrc/host/mdk_mergecontext.c) looks both up in the FASTA; a row carries
// them.  d = t + 1 is the distance from a site's C to its G.
//   t == 2          the row as it is, strand kept
//   t < 2, a C at p its partner is the NEXT row if that is the G of the same contig and context at p + d; the row (contig, p, p + d + 1, the
//                   counts, of both if there is a partner, t, strand 0) takes the C's place
//   t < 2, a G at q no row if the row BEFORE it is its C by the same test; otherwise the lone row (contig, q - d, q + 1, its counts, t, 0)
// and a row made this way is dropped if nmeth + nunmeth < min_depth (CHH rows too, as `extract -d` does).
//
// Only the adjacent row is looked at, and that is exact: in ascending input nothing can lie between a C and the G of its site.  For CpG they
// are neighbouring bases.  For CHG the base p + 1 between them is no G (the C would be a CpG's), and if it is a C then ITS next base is that G:
// the G belongs to that C's CpG and is no CHG row at all.  So where a CHG C has its G as a row, p + 1 is no cytosine and has no row; rows
// taken out of the table (a filter) only bring the two closer.  This is why the kernels need a halo of one row on each side and no search.
//
// What is refused (MRG_E_*), found by looking at rows i - 1 and i alone, so that every workgroup finds its own: a CpG / CHG row without a
// strand or any row wider than one base (the table was merged already), a context above 2, a contig index outside the name table, rows
// not strictly ascending, a lone G with q < d (its site would start before the contig), a sum of counts above INT32_MAX.
//
// Plain C++ as mdk_text_core.h: it compiles for the device (mdk_merge.hip) and for the host (tools/merge_emu.cpp runs the kernels' blocking
// over it), which is how it is tested without a GPU.
#ifndef MDK_MERGE_CORE_H
#define MDK_MERGE_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define MDK_MRG __host__ __device__ __forceinline__
#else
#define MDK_MRG static inline
#endif

enum { MRG_E_MERGED = 1, MRG_E_CONTEXT = 2, MRG_E_CONTIG = 4, MRG_E_ORDER = 8, MRG_E_LONE_G = 16, MRG_E_SUM = 32, MRG_E_CHANGED = 64 };

// a row; `has` is 0 for the neighbour of the table's first or last row
struct mrg_row { int32_t contig, start, end, m, u, ctx, strand, has; };

// is g the G of c's CpG / CHG site?
MDK_MRG int mrg_pair(const mrg_row &c, const mrg_row &g) {
    return c.has && g.has && (uint32_t)c.ctx < 2u && c.strand > 0 && g.strand < 0 && g.contig == c.contig && g.ctx == c.ctx && (int64_t)g.start == (int64_t)c.start + c.ctx + 1;
}

// the row that `cur` gives between `prev` and `next`: 1 and `out`, or 0 (the G of a pair, a row below min_depth, a refused row: err |= MRG_E_*)
MDK_MRG int mrg_row_out(const mrg_row &prev, const mrg_row &cur, const mrg_row &next, int32_t n_contigs, int32_t min_depth, mrg_row &out, uint32_t &err) {
    if((uint32_t)cur.ctx > 2u) { err |= MRG_E_CONTEXT; return 0; }
    if(cur.contig < 0 || cur.contig >= n_contigs) { err |= MRG_E_CONTIG; return 0; }
    if(prev.has && !(prev.contig < cur.contig || (prev.contig == cur.contig && prev.start < cur.start))) { err |= MRG_E_ORDER; return 0; }
    if((int64_t)cur.end != (int64_t)cur.start + 1 || (cur.ctx < 2 && cur.strand == 0)) { err |= MRG_E_MERGED; return 0; }
    // (every field of `out` is written once, from values: a field written on one path only costs the device code a stack slot)
    int64_t m = cur.m, u = cur.u;
    int32_t start = cur.start, end = cur.end, strand = cur.strand;
    if(cur.ctx < 2) {
        const int32_t d = cur.ctx + 1;
        strand = 0;
        if(cur.strand > 0) {
            if(mrg_pair(cur, next)) { m += next.m; u += next.u; }
            if(m > INT32_MAX || u > INT32_MAX) { err |= MRG_E_SUM; return 0; }
            end = (int32_t)((uint32_t)cur.start + (uint32_t)d + 1u);
        } else {
            if(mrg_pair(prev, cur)) return 0;
            if(cur.start < d) { err |= MRG_E_LONE_G; return 0; }
            start = cur.start - d;
        }
    }
    out.contig = cur.contig; out.start = start; out.end = end; out.m = (int32_t)m; out.u = (int32_t)u; out.ctx = cur.ctx; out.strand = strand; out.has = 1;
    return m + u >= (int64_t)min_depth;
}
#endif
