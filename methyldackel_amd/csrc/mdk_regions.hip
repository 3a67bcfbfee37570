// mdk_regions.hip -- sums of rows over intervals on the device (include/mdk_hip.h, "sums over intervals"): the calls of a session's Calls,
// or the rows of its Cytosines, added up per CpG island, promoter, candidate DMR or fixed tile, without a file or the host.
//
// The rule is mdk_region_core.h's: the rows are strictly ascending in (contig, start), so the rows of an interval are the contiguous range
// [lo, hi) between two lower bounds, and a row counts if its context, its strand and its depth pass the filter.  One synchronous call on the
// md_text handle -- its stream, its status block and its contig count are what this needs; the prefix table is this file's own, so a measure
// of the text, merge or parse kind that waits for its fill is left as it is:
//   k_region_rows   a row per lane, 256 per workgroup.  Every lane loads its own row once (coalesced); row i - 1 comes from the lane beside it
//                   (__shfl_up), for lane 0 of a wavefront from global memory, and nothing is loaded before row 0.  The refusals go to the
//                   status, the filter is applied, and the workgroup's (nsites, nmeth, nunmeth) go to the table: 20 bytes per 256 rows
//   k_region_blocks one workgroup: the three columns of totals scanned in place into exclusive prefixes, 4096 blocks a round with a carry,
//                   and the grand totals as entry nb
//   k_region_sum    64 intervals per wavefront.  First a lane per interval: the interval checked, lo and hi by two binary searches (the second
//                   from lo on), the whole 256-row blocks inside [lo, hi) as the difference of two prefix entries.  Then the wavefront
//                   together, one of its intervals after the other: the rows of the two partial blocks at the ends -- at most 255 + 255,
//                   or just [lo, hi) where both lie in one block -- read coalesced with the filter applied again, reduced over the
//                   lanes and added to the owner's sums.  Every lane writes its interval's three results, coalesced
// The work per interval is bounded whatever its length: two searches of at most 31 steps, six prefix entries, at most 510 rows.  Nothing is
// read before row 0, past row n - 1 or past interval k - 1.  Integer work, plain C++, vector loads and stores: 18 bytes per row read once, 10
// bytes per row of a partial block read again.
#include "mdk_text_internal.hpp"
#include "mdk_region_core.h"

__device__ __forceinline__ rgn_filter region_filter(const KRegion &K) {
    rgn_filter f; f.context_mask = K.context_mask; f.strand_mask = K.strand_mask; f.min_depth = K.min_depth;
    return f;
}

// the sum of (s, m, u) over the wavefront, in every lane
__device__ __forceinline__ void region_wave_sum(uint32_t &s, long long &m, long long &u) {
    for(int d = 32; d; d >>= 1) { s += __shfl_xor(s, d, 64); m += __shfl_xor(m, d, 64); u += __shfl_xor(u, d, 64); }
}

__global__ __launch_bounds__(TEXT_WG) void k_region_rows(const KRegion K) {
    __shared__ uint32_t ws[TEXT_WG / 64];
    __shared__ long long wm[TEXT_WG / 64], wu[TEXT_WG / 64];
    const uint32_t i = blockIdx.x * TEXT_WG + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool has = i < K.n;
    int32_t contig = 0, start = 0, m = 0, u = 0, ctx = 0, strand = 0;
    if(has) { contig = K.contig[i]; start = K.start[i]; m = K.m[i]; u = K.u[i]; ctx = K.ctx[i]; strand = K.strand[i]; }
    // (every lane of the wavefront takes part in the moves, rows or not)
    int32_t pcontig = __shfl_up(contig, 1, 64), pstart = __shfl_up(start, 1, 64);
    uint32_t s = 0; long long sm = 0, su = 0;
    if(has) {
        int has_prev = 1;
        if(lane == 0) { has_prev = i > 0; if(has_prev) { pcontig = K.contig[i - 1]; pstart = K.start[i - 1]; } }
        const uint32_t err = rgn_row_check(has_prev, pcontig, pstart, contig, start, ctx, K.n_contigs);
        if(err) atomicOr(&K.st->err, err);
        if(rgn_counts(region_filter(K), m, u, ctx, strand)) { s = 1; sm = m; su = u; }
    }
    region_wave_sum(s, sm, su);
    if(lane == 0) { ws[wave] = s; wm[wave] = sm; wu[wave] = su; }
    __syncthreads();
    if(threadIdx.x == 0) {
        for(int w = 1; w < TEXT_WG / 64; w++) { s += ws[w]; sm += wm[w]; su += wu[w]; }
        K.pre_sites[blockIdx.x] = s; K.pre_m[blockIdx.x] = sm; K.pre_u[blockIdx.x] = su;
    }
}

// text_scan_blocks' loop over one column of totals, in place: entry b becomes the sum of the totals of the blocks before b, entry nb the sum
// of all.  A thread takes REGION_SCAN_PER neighbouring entries a round -- a quarter of the rounds, each a barrier pair, of one entry per
// thread --, and one column comes after the other: the three scans side by side want more registers than a workgroup of 1024 has
#define REGION_SCAN_PER 4
template <typename T>
__device__ __forceinline__ void region_scan_column(T *col, uint32_t nb, int64_t *wtot) {
    int64_t carry = 0;
    for(uint32_t b0 = 0; b0 < nb; b0 += TEXT_SCAN_WG * REGION_SCAN_PER) {          // (uniform trip count: every thread takes part in every scan)
        const uint32_t b = b0 + threadIdx.x * REGION_SCAN_PER;
        int64_t v[REGION_SCAN_PER], sum = 0, total;
#pragma unroll
        for(int q = 0; q < REGION_SCAN_PER; q++) { v[q] = b + q < nb ? (int64_t)col[b + q] : 0; sum += v[q]; }
        int64_t run = carry + block_excl_scan<TEXT_SCAN_WG>(sum, wtot, total);
#pragma unroll
        for(int q = 0; q < REGION_SCAN_PER; q++) { if(b + q < nb) col[b + q] = (T)run; run += v[q]; }
        carry += total;
    }
    if(threadIdx.x == 0) col[nb] = (T)carry;
}

__global__ __launch_bounds__(TEXT_SCAN_WG) void k_region_blocks(const KRegion K) {
    __shared__ int64_t wtot[TEXT_SCAN_WG / 64];
    const uint32_t nb = (K.n + TEXT_WG - 1) / TEXT_WG;
    region_scan_column(K.pre_sites, nb, wtot);
    region_scan_column(K.pre_m, nb, wtot);
    region_scan_column(K.pre_u, nb, wtot);
}

__global__ __launch_bounds__(TEXT_WG) void k_region_sum(const KRegion K) {
    const int lane = threadIdx.x & 63;
    const uint32_t j0 = (blockIdx.x * (TEXT_WG / 64) + (threadIdx.x >> 6)) * 64;          // the wavefront's first interval
    if(j0 >= K.k) return;                                                                  // (the whole wavefront; there is no barrier below)
    const uint32_t j = j0 + lane;
    const bool has = j < K.k;
    const rgn_filter F = region_filter(K);
    // a lane per interval: its range, and what whole blocks give
    uint32_t lo = 0, hi = 0, sites = 0; long long sm = 0, su = 0;
    rgn_split sp; sp.a_end = sp.b_beg = sp.b0 = sp.b1 = 0;
    if(has) {
        const int32_t c = K.iv_contig[j], s = K.iv_start[j], e = K.iv_end[j];
        const uint32_t err = rgn_interval_check(c, s, e, K.n_contigs);
        if(err) atomicOr(&K.st->err, err);
        else {
            lo = rgn_lower_bound(K.contig, K.start, 0, K.n, c, s);
            hi = rgn_lower_bound(K.contig, K.start, lo, K.n, c, e);
            sp = rgn_split_range(lo, hi);
            if(sp.b0 < sp.b1) { sites = K.pre_sites[sp.b1] - K.pre_sites[sp.b0]; sm = K.pre_m[sp.b1] - K.pre_m[sp.b0]; su = K.pre_u[sp.b1] - K.pre_u[sp.b0]; }
        }
    }
    // the wavefront per interval: rows [lo, a_end) and [b_beg, hi), 64 at a time (a refused interval has none)
    const uint32_t mine = K.k - j0 < 64u ? K.k - j0 : 64u;
    for(uint32_t t = 0; t < mine; t++) {
        const uint32_t a0 = __shfl(lo, t, 64), a1 = __shfl(sp.a_end, t, 64), b0 = __shfl(sp.b_beg, t, 64), b1 = __shfl(hi, t, 64);
        const uint32_t la = a1 - a0, len = la + (b1 - b0);
        if(!len) continue;
        uint32_t ps = 0; long long pm = 0, pu = 0;
        for(uint32_t r = lane; r < len; r += 64) {
            const uint32_t i = r < la ? a0 + r : b0 + (r - la);
            const int32_t m = K.m[i], u = K.u[i];
            if(rgn_counts(F, m, u, K.ctx[i], K.strand[i])) { ps++; pm += m; pu += u; }
        }
        region_wave_sum(ps, pm, pu);
        if(lane == (int)t) { sites += ps; sm += pm; su += pu; }
    }
    if(has) { K.nsites[j] = (int32_t)sites; K.nmeth[j] = sm; K.nunmeth[j] = su; }
}

void text_regions_free(md_text *t) {
    (void)hipFree(t->d_rsites); (void)hipFree(t->d_rm); (void)hipFree(t->d_ru);
    t->d_rsites = nullptr; t->d_rm = t->d_ru = nullptr; t->cap_rblocks = 0;
}

// the prefix table for nb blocks: nb + 1 entries a column (as text_blocks_reserve)
static int regions_reserve(md_text *t, uint32_t nb) {
    if((size_t)nb + 1 > t->cap_rblocks) {
        text_regions_free(t);
        const size_t want = (size_t)nb + nb / 4 + 64;
        hipError_t e = hipMalloc((void **)&t->d_rsites, want * 4);
        if(e == hipSuccess) e = hipMalloc((void **)&t->d_rm, want * 8);
        if(e == hipSuccess) e = hipMalloc((void **)&t->d_ru, want * 8);
        if(e != hipSuccess) { text_regions_free(t); return fail(MDK_ERR_NOMEM, "hipMalloc(region prefix table)", e); }
        t->cap_rblocks = want;
    }
    return 0;
}

extern "C" int md_text_regions(md_text *t, const md_calls_cols *c, int64_t n, const int32_t *iv_contig, const int32_t *iv_start, const int32_t *iv_end, int64_t k,
                               uint32_t context_mask, uint32_t strand_mask, int32_t min_depth, int32_t *nsites, int64_t *nmeth, int64_t *nunmeth) {
    const char *const what = "md_text_regions";
    if(!t || !c || n < 0 || n > TEXT_MAX_ROWS || k < 0 || k > TEXT_MAX_ROWS || context_mask > 7u || strand_mask > 7u || min_depth < 0) return fail(MDK_ERR_ARG, what, hipSuccess);
    if(n && (!c->contig || !c->start || !c->nmeth || !c->nunmeth || !c->context || !c->strand)) return fail(MDK_ERR_ARG, what, hipSuccess);
    if(k && (!iv_contig || !iv_start || !iv_end || !nsites || !nmeth || !nunmeth)) return fail(MDK_ERR_ARG, what, hipSuccess);
    const uint32_t nb = (uint32_t)((n + TEXT_WG - 1) / TEXT_WG);
    HIPCHK(hipSetDevice(t->device));
    { const int rc = regions_reserve(t, nb); if(rc) return rc; }
    KRegion K;
    K.contig = c->contig; K.start = c->start; K.m = c->nmeth; K.u = c->nunmeth; K.ctx = c->context; K.strand = c->strand;
    K.n = (uint32_t)n; K.n_contigs = t->n_contigs;
    K.iv_contig = iv_contig; K.iv_start = iv_start; K.iv_end = iv_end; K.k = (uint32_t)k;
    K.context_mask = context_mask; K.strand_mask = strand_mask; K.min_depth = min_depth;
    K.pre_sites = t->d_rsites; K.pre_m = t->d_rm; K.pre_u = t->d_ru; K.st = t->d_st;
    K.nsites = nsites; K.nmeth = nmeth; K.nunmeth = nunmeth;
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    if(nb) {
        hipLaunchKernelGGL(k_region_rows, dim3(nb), dim3(TEXT_WG), 0, t->st, K);
        hipLaunchKernelGGL(k_region_blocks, dim3(1), dim3(TEXT_SCAN_WG), 0, t->st, K);
    }
    if(k) hipLaunchKernelGGL(k_region_sum, dim3((uint32_t)((k + TEXT_WG - 1) / TEXT_WG)), dim3(TEXT_WG), 0, t->st, K);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(t->h_st, t->d_st, sizeof(TextStatus), hipMemcpyDeviceToHost, t->st));
    HIPCHK(hipStreamSynchronize(t->st));
    const uint32_t err = t->h_st->err;
    if(!err) return 0;
    snprintf(mdk_err_buf(), MDK_ERR_BYTES, "%s: %s", what,
             err & RGN_E_CONTIG ? "a row's contig is not an index into the contig names" :
             err & RGN_E_CONTEXT ? "a row's context is not 0, 1 or 2" :
             err & RGN_E_ORDER ? "the rows are not ascending in (contig, start), strictly" :
             err & RGN_E_IV_CONTIG ? "an interval's contig is not an index into the contig names" : "an interval has start < 0 or end < start");
    return MDK_ERR_ARG;
}
