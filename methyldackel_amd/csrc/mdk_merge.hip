// mdk_merge.hip -- `mergeContext` over rows on the device (include/mdk_hip.h, "mergeContext on the device"): the per-strand calls of a
// session's Calls, or the rows of its Cytosines, folded into per-CpG / per-CHG rows without a FASTA, a file or the host.
//
// The rule is mdk_merge_core.h's: what a row gives depends on the row before it and the row after it alone (why that is exact is argued
// there), so a workgroup needs a halo of one row on each side, no search, and nothing of another workgroup.  Measure first, fill second, on the
// md_text handle -- its stream, its table of one entry per 256 rows, its status block and its contig count are what this needs:
//   k_merge_len    a row per lane, 256 per workgroup.  Every lane loads its own row once (coalesced); rows i - 1 and i + 1 come from the
//                  neighbouring lanes (__shfl_up / __shfl_down).  Only lanes 0 and 63 of a wavefront load their outer neighbour from global
//                  memory -- the row before the workgroup's first and after its last among them --, and nothing before row 0 or past row n - 1.
//                  "Gives a row" scanned inside the workgroup (block_excl_scan), the workgroup's total to the table, the refusals to the status
//   k_merge_blocks one workgroup: the exclusive scan of those totals as int64 offsets and the row count of the result (text_scan_blocks,
//                  k_text_blocks' loop)
//   k_merge_fill   the same rows, flags and scan again -- 22 bytes per row read a second time, against a per-row offset of 4 bytes written,
//                  read back and kept --, then every lane that gives a row writes its seven columns at the workgroup's offset + its scanned place
// k_merge_fill re-checks every workgroup's total against what k_merge_len recorded: columns that changed between the two calls end the fill
// with an error and never with a write past the columns.  Integer work at 22 + 22 + 22 bytes per row: HBM-bound, no LDS beyond the scan's
// four words.
#include "mdk_text_internal.hpp"
#include "mdk_merge_core.h"

// row i's own columns (i < K.n)
__device__ __forceinline__ mrg_row merge_load(const KMerge &K, uint32_t i) {
    mrg_row r;
    r.contig = K.contig[i]; r.start = K.start[i]; r.end = K.end[i]; r.m = K.m[i]; r.u = K.u[i]; r.ctx = K.ctx[i]; r.strand = K.strand[i]; r.has = 1;
    return r;
}
// what the pair test and the order test read of a neighbour (no end; counts only of the row after)
__device__ __forceinline__ mrg_row merge_load_nbr(const KMerge &K, uint32_t i, bool counts) {
    mrg_row r;
    r.contig = K.contig[i]; r.start = K.start[i]; r.end = 0; r.m = counts ? K.m[i] : 0; r.u = counts ? K.u[i] : 0; r.ctx = K.ctx[i]; r.strand = K.strand[i]; r.has = 1;
    return r;
}

// the row lane threadIdx.x's row i gives (0 / 1 and `out`): its own row from global memory, its neighbours from the lanes beside it
__device__ __forceinline__ uint32_t merge_row(const KMerge &K, uint32_t i, mrg_row &out, uint32_t &err) {
    const int lane = threadIdx.x & 63;
    mrg_row cur; cur.contig = cur.start = cur.end = cur.m = cur.u = cur.ctx = cur.strand = cur.has = 0;
    if(i < K.n) cur = merge_load(K, i);
    // (every lane of the wavefront takes part in the moves, rows or not)
    mrg_row prev, next;
    prev.contig = __shfl_up(cur.contig, 1, 64); prev.start = __shfl_up(cur.start, 1, 64); prev.ctx = __shfl_up(cur.ctx, 1, 64); prev.strand = __shfl_up(cur.strand, 1, 64);
    prev.has = __shfl_up(cur.has, 1, 64); prev.end = prev.m = prev.u = 0;
    next.contig = __shfl_down(cur.contig, 1, 64); next.start = __shfl_down(cur.start, 1, 64); next.ctx = __shfl_down(cur.ctx, 1, 64); next.strand = __shfl_down(cur.strand, 1, 64);
    next.m = __shfl_down(cur.m, 1, 64); next.u = __shfl_down(cur.u, 1, 64); next.has = __shfl_down(cur.has, 1, 64); next.end = 0;
    if(i >= K.n) return 0;
    if(lane == 0) { prev.has = 0; if(i > 0) prev = merge_load_nbr(K, i - 1, false); }
    if(lane == 63) { next.has = 0; if(i + 1 < K.n) next = merge_load_nbr(K, i + 1, true); }
    return (uint32_t)mrg_row_out(prev, cur, next, K.n_contigs, K.min_depth, out, err);
}

__global__ __launch_bounds__(TEXT_WG) void k_merge_len(const KMerge K) {
    __shared__ uint32_t wtot[TEXT_WG / 64];
    mrg_row out; uint32_t err = 0, total;
    const uint32_t has = merge_row(K, blockIdx.x * TEXT_WG + threadIdx.x, out, err);
    if(err) atomicOr(&K.st->err, err);
    (void)block_excl_scan<TEXT_WG>(has, wtot, total);
    if(threadIdx.x == 0) K.btot[blockIdx.x] = total;
}

__global__ __launch_bounds__(TEXT_SCAN_WG) void k_merge_blocks(const KMerge K) {
    __shared__ int64_t wtot[TEXT_SCAN_WG / 64];
    text_scan_blocks(K.btot, K.boff, K.st, (K.n + TEXT_WG - 1) / TEXT_WG, wtot);
}

__global__ __launch_bounds__(TEXT_WG) void k_merge_fill(const KMerge K) {
    __shared__ uint32_t wtot[TEXT_WG / 64];
    mrg_row out; uint32_t err = 0, total;
    const uint32_t has = merge_row(K, blockIdx.x * TEXT_WG + threadIdx.x, out, err);
    const uint32_t ex = block_excl_scan<TEXT_WG>(has, wtot, total);
    const int64_t off = K.boff[blockIdx.x];
    // a row the measuring pass would have refused, another total than it recorded, or a place outside the result: the columns are not the measured ones
    if(__syncthreads_or(err != 0) || total != K.btot[blockIdx.x] || off < 0 || off + (int64_t)total > K.rows) { if(threadIdx.x == 0) atomicOr(&K.st->err, (uint32_t)MRG_E_CHANGED); return; }
    if(!has) return;
    const int64_t o = off + ex;
    K.dst.contig[o] = out.contig; K.dst.start[o] = out.start; K.dst.end[o] = out.end; K.dst.nmeth[o] = out.m; K.dst.nunmeth[o] = out.u;
    K.dst.context[o] = (uint8_t)out.ctx; K.dst.strand[o] = (int8_t)out.strand;
}

// the status block back on the host; what the kernels flagged as this call's error
static int merge_status(md_text *t, const char *what) {
    HIPCHK(hipMemcpyAsync(t->h_st, t->d_st, sizeof(TextStatus), hipMemcpyDeviceToHost, t->st));
    HIPCHK(hipStreamSynchronize(t->st));
    const uint32_t err = t->h_st->err;
    if(!err) return 0;
    snprintf(mdk_err_buf(), MDK_ERR_BYTES, "%s: %s", what,
             err & MRG_E_CHANGED ? "the columns are not the ones that were measured" :
             err & MRG_E_CONTIG ? "a row's contig is not an index into the contig names" :
             err & MRG_E_CONTEXT ? "a row's context is not 0, 1 or 2" :
             err & MRG_E_MERGED ? "a CpG / CHG row has strand 0 or a row is wider than one base: the rows are merged already" :
             err & MRG_E_ORDER ? "the rows are not ascending in (contig, start), strictly" :
             err & MRG_E_LONE_G ? "a G without its C lies closer to the contig's start than its site is long" : "the counts of a merged row add up to more than INT32_MAX");
    return MDK_ERR_ARG;
}

extern "C" int md_text_merge_measure(md_text *t, const md_calls_cols *c, int64_t n, int32_t min_depth, int64_t *rows) {
    const char *const what = "md_text_merge_measure";
    if(!t || !c || !rows || n < 0 || n > TEXT_MAX_ROWS || min_depth < 0) return fail(MDK_ERR_ARG, what, hipSuccess);
    *rows = 0; t->measured = false; t->merge_measured = false; t->parse_measured = false;
    if(n && (!c->contig || !c->start || !c->end || !c->nmeth || !c->nunmeth || !c->context || !c->strand)) return fail(MDK_ERR_ARG, what, hipSuccess);
    const uint32_t nb = (uint32_t)((n + TEXT_WG - 1) / TEXT_WG);
    HIPCHK(hipSetDevice(t->device));
    { const int rc = text_blocks_reserve(t, nb); if(rc) return rc; }
    KMerge &M = t->M;
    M.contig = c->contig; M.start = c->start; M.end = c->end; M.m = c->nmeth; M.u = c->nunmeth; M.ctx = c->context; M.strand = c->strand;
    M.n = (uint32_t)n; M.n_contigs = t->n_contigs; M.min_depth = min_depth; M.btot = t->d_btot; M.boff = t->d_boff; M.st = t->d_st;
    M.dst = md_calls_cols(); M.rows = 0;
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    if(nb) {
        hipLaunchKernelGGL(k_merge_len, dim3(nb), dim3(TEXT_WG), 0, t->st, M);
        hipLaunchKernelGGL(k_merge_blocks, dim3(1), dim3(TEXT_SCAN_WG), 0, t->st, M);
        HIPCHK(hipGetLastError());
    }
    { const int rc = merge_status(t, what); if(rc) return rc; }
    M.rows = t->h_st->total; t->merge_measured = true;
    *rows = M.rows;
    return 0;
}

extern "C" int md_text_merge_fill(md_text *t, const md_calls_cols *dst, int64_t rows) {
    if(!t || !t->merge_measured || !dst || rows != t->M.rows) return fail(MDK_ERR_ARG, "md_text_merge_fill: md_text_merge_measure first, then columns of exactly the measured number of rows", hipSuccess);
    if(!rows) return 0;
    if(!dst->contig || !dst->start || !dst->end || !dst->nmeth || !dst->nunmeth || !dst->context || !dst->strand) return fail(MDK_ERR_ARG, "md_text_merge_fill", hipSuccess);
    HIPCHK(hipSetDevice(t->device));
    KMerge &M = t->M; M.dst = *dst;
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    hipLaunchKernelGGL(k_merge_fill, dim3((M.n + TEXT_WG - 1) / TEXT_WG), dim3(TEXT_WG), 0, t->st, M);
    HIPCHK(hipGetLastError());
    return merge_status(t, "md_text_merge_fill");
}
