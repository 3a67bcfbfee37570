// mdk_cregion.hip -- every sample's sums over intervals in one pass: md_cohort_regions of include/mdk_cohort.h (Cohort.regions).  A part
// of libmdk_cohort.so: csrc/mdk_cohort.hip includes this file behind its own host code, so the library stays one source and one code object.
//
// The rule is mdk_region_core.h's applied to sample s of the [S, n] matrices; what the kernels share with tools/cregion_emu.cpp is
// mdk_cregion_core.h's.  What depends on the sites or on the intervals alone is done once, not once a sample:
//   k_cregion_sites   a row per lane, blocks of 256 rows in a grid-stride loop.  Row i - 1 comes from the lane beside (__shfl_up), for lane 0
//                     of a wavefront from global memory, nothing before row 0.  The row's refusals go to the status and the context and
//                     strand part of the filter becomes a byte per site: 10 bytes per site read, 1 written
//   k_cregion_ranges  a lane per interval: the interval checked, lo and hi by two binary searches (the second from lo on), 8 bytes written
//   k_cregion_totals  a WAVEFRONT takes a block of 256 sites and a batch of `sample_block` samples: the sites' four bytes per lane are
//                     loaded once and kept in registers, then per sample four coalesced loads of each matrix along the site axis, the
//                     depth cut, one reduction over the lanes and the block's (nsites, nmeth, nunmeth) into the sample's table: 8 bytes per
//                     cell read, 20 per 256 cells written.  No LDS and no barrier
//   k_cregion_scan    a workgroup of 1024 per sample: its three columns of totals into exclusive prefixes in place, CRG_SCAN_ROUND entries
//                     a round with a carry, the sum of all as entry nb
//   k_cregion_sum     a wavefront takes 64 intervals, a lane each, and a batch of samples.  lo, hi and the split are loaded once and stay in
//                     registers across the sample loop.  Per sample: the whole blocks as the difference of two prefix entries of that
//                     sample; then the rows of the two partial blocks -- at most 255 + 255 --, CRG_LANES lanes per interval and 64 /
//                     CRG_LANES intervals at a time, read along the site axis, reduced over the group's lanes and handed to the owner;
//                     every lane writes its interval's three results along the interval axis
// Every launch is capped at the handle's max_workgroups and strides over its items, every cell offset is crg_cell's 64 bits, and no result
// depends on the limits.  Nothing is read before row 0, past row n - 1, past sample S - 1 or past interval k - 1.  Integer work, plain C++,
// vector loads and stores, no atomics but the status word's atomicOr.
#include "mdk_cregion_core.h"

#define CRG_WG 256
#define CRG_WAVES (CRG_WG / 64)
#define CRG_LANES 16                     // lanes that read an interval's partial blocks together (64, the wavefront an interval, was 3.5 to 4.7 times slower)

struct KCrg {
    const int32_t *contig, *start; const uint8_t *ctx; const int8_t *strand;
    const int32_t *m, *u; int32_t S, sblock, n_contigs; int64_t n, nb;
    const int32_t *iv_contig, *iv_start, *iv_end; int64_t k;
    rgn_filter F;
    uint8_t *pass; uint32_t *lo, *hi; uint32_t *pre_sites; int64_t *pre_m, *pre_u;
    int32_t *nsites; int64_t *nmeth, *nunmeth;
    CohStatus *st;
};

__global__ __launch_bounds__(CRG_WG) void k_cregion_sites(const KCrg K) {
    const int lane = threadIdx.x & 63;
    for(int64_t b = blockIdx.x; b < K.nb; b += gridDim.x) {                // (uniform trip count: every lane takes part in the moves)
        const int64_t i = b * RGN_ROWS + threadIdx.x;
        const bool has = i < K.n;
        int32_t contig = 0, start = 0, ctx = 0, strand = 0;
        if(has) { contig = K.contig[i]; start = K.start[i]; ctx = K.ctx[i]; strand = K.strand[i]; }
        int32_t pcontig = __shfl_up(contig, 1, 64), pstart = __shfl_up(start, 1, 64);
        if(has) {
            int has_prev = 1;
            if(lane == 0) { has_prev = i > 0; if(has_prev) { pcontig = K.contig[i - 1]; pstart = K.start[i - 1]; } }
            const uint32_t err = rgn_row_check(has_prev, pcontig, pstart, contig, start, ctx, K.n_contigs);
            if(err) atomicOr(&K.st->first, (unsigned long long)err);
            K.pass[i] = crg_site_passes(K.F, ctx, strand);
        }
    }
}

__global__ __launch_bounds__(CRG_WG) void k_cregion_ranges(const KCrg K) {
    for(int64_t j = (int64_t)blockIdx.x * CRG_WG + threadIdx.x; j < K.k; j += (int64_t)gridDim.x * CRG_WG) {
        const int32_t c = K.iv_contig[j], s = K.iv_start[j], e = K.iv_end[j];
        const uint32_t err = rgn_interval_check(c, s, e, K.n_contigs);
        uint32_t lo = 0, hi = 0;
        if(err) atomicOr(&K.st->first, (unsigned long long)err);
        else {
            lo = rgn_lower_bound(K.contig, K.start, 0, (uint32_t)K.n, c, s);
            hi = rgn_lower_bound(K.contig, K.start, lo, (uint32_t)K.n, c, e);
        }
        K.lo[j] = lo; K.hi[j] = hi;
    }
}

// the sums of m and u over the lanes of a group of `width` neighbouring lanes, in every lane of the group
__device__ __forceinline__ void crg_group_sum(long long &m, long long &u, int width) {
    for(int d = width >> 1; d; d >>= 1) { m += __shfl_xor(m, d, 64); u += __shfl_xor(u, d, 64); }
}

__global__ __launch_bounds__(CRG_WG) void k_cregion_totals(const KCrg K) {
    const int lane = threadIdx.x & 63;
    const int32_t nbt = crg_batches(K.S, K.sblock);
    const int64_t items = K.nb * nbt, stride = (int64_t)gridDim.x * CRG_WAVES;
    for(int64_t item = (int64_t)blockIdx.x * CRG_WAVES + (threadIdx.x >> 6); item < items; item += stride) {      // (a wavefront's own loop: no barrier below)
        const int32_t t = (int32_t)(item / K.nb);
        const int64_t b = item - (int64_t)t * K.nb, i0 = b * RGN_ROWS + lane;
        int32_t s0, s1;
        crg_batch(t, K.S, K.sblock, s0, s1);
        uint8_t pass[RGN_ROWS / 64];
#pragma unroll
        for(int q = 0; q < RGN_ROWS / 64; q++) pass[q] = i0 + 64 * q < K.n ? K.pass[i0 + 64 * q] : (uint8_t)0;
        for(int32_t s = s0; s < s1; s++) {
            uint32_t sites = 0; long long sm = 0, su = 0;
#pragma unroll
            for(int q = 0; q < RGN_ROWS / 64; q++) {
                const int64_t i = i0 + 64 * q;
                int32_t m = 0, u = 0;
                if(i < K.n) { m = K.m[crg_cell(s, i, K.n)]; u = K.u[crg_cell(s, i, K.n)]; }
                const int c = i < K.n && crg_cell_counts(pass[q], m, u, K.F.min_depth);
                sites += (uint32_t)__popcll(__ballot(c));
                if(c) { sm += m; su += u; }
            }
            crg_group_sum(sm, su, 64);
            if(lane == 0) { const int64_t e = crg_entry(s, b, K.nb); K.pre_sites[e] = sites; K.pre_m[e] = sm; K.pre_u[e] = su; }
        }
    }
}

// v's exclusive prefix over the workgroup's threads and the sum of all (wtot: an entry per wavefront)
__device__ __forceinline__ int64_t crg_block_excl_scan(int64_t v, int64_t *wtot, int64_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long incl = v;
#pragma unroll
    for(int d = 1; d < 64; d <<= 1) { const long long o = __shfl_up(incl, d, 64); if(lane >= d) incl += o; }
    if(lane == 63) wtot[wave] = incl;
    __syncthreads();
    int64_t before = 0, all = 0;
    for(int w = 0; w < CRG_SCAN_WG / 64; w++) { const int64_t x = wtot[w]; if(w < wave) before += x; all += x; }
    __syncthreads();                                                        // (wtot is written again by the next scan)
    total = all;
    return before + incl - v;
}

// one column of one sample, in place: entry b becomes the sum of the totals of the blocks before b, entry nb the sum of all
template <typename T>
__device__ __forceinline__ void crg_scan_column(T *col, int64_t nb, int64_t *wtot) {
    int64_t carry = 0;
    for(int64_t b0 = 0; b0 < nb; b0 += CRG_SCAN_ROUND) {                    // (uniform trip count: every thread takes part in every scan)
        const int64_t b = b0 + (int64_t)threadIdx.x * CRG_SCAN_PER;
        int64_t v[CRG_SCAN_PER], sum = 0, total;
#pragma unroll
        for(int q = 0; q < CRG_SCAN_PER; q++) { v[q] = b + q < nb ? (int64_t)col[b + q] : 0; sum += v[q]; }
        int64_t run = carry + crg_block_excl_scan(sum, wtot, total);
#pragma unroll
        for(int q = 0; q < CRG_SCAN_PER; q++) { if(b + q < nb) col[b + q] = (T)run; run += v[q]; }
        carry += total;
    }
    if(threadIdx.x == 0) col[nb] = (T)carry;
}

__global__ __launch_bounds__(CRG_SCAN_WG) void k_cregion_scan(const KCrg K) {
    __shared__ int64_t wtot[CRG_SCAN_WG / 64];
    for(int32_t s = blockIdx.x; s < K.S; s += gridDim.x) {
        const int64_t e = crg_entry(s, 0, K.nb);
        crg_scan_column(K.pre_sites + e, K.nb, wtot);
        crg_scan_column(K.pre_m + e, K.nb, wtot);
        crg_scan_column(K.pre_u + e, K.nb, wtot);
    }
}

__global__ __launch_bounds__(CRG_WG) void k_cregion_sum(const KCrg K) {
    const int lane = threadIdx.x & 63, sub = lane / CRG_LANES, part = lane % CRG_LANES;
    constexpr int TOGETHER = 64 / CRG_LANES;                                // intervals whose partial blocks are read at a time
    const int32_t nbt = crg_batches(K.S, K.sblock);
    const int64_t groups = (K.k + 63) / 64, items = groups * nbt, stride = (int64_t)gridDim.x * CRG_WAVES;
    for(int64_t item = (int64_t)blockIdx.x * CRG_WAVES + (threadIdx.x >> 6); item < items; item += stride) {      // (a wavefront's own loop: no barrier below)
        const int32_t t = (int32_t)(item / groups);
        const int64_t j0 = (item - (int64_t)t * groups) * 64, j = j0 + lane;
        const bool has = j < K.k;
        int32_t s0, s1;
        crg_batch(t, K.S, K.sblock, s0, s1);
        crg_range R = crg_range_of(0, 0);
        if(has) R = crg_range_of(K.lo[j], K.hi[j]);
        const int mine = K.k - j0 < 64 ? (int)(K.k - j0) : 64;
        for(int32_t s = s0; s < s1; s++) {
            uint32_t sites = 0; long long sm = 0, su = 0;
            if(has && R.sp.b0 < R.sp.b1) {
                const int64_t e0 = crg_entry(s, R.sp.b0, K.nb), e1 = crg_entry(s, R.sp.b1, K.nb);
                sites = K.pre_sites[e1] - K.pre_sites[e0]; sm = K.pre_m[e1] - K.pre_m[e0]; su = K.pre_u[e1] - K.pre_u[e0];
            }
            // group `sub` reads rows [lo, a_end) and [b_beg, hi) of interval t0 + sub, CRG_LANES at a time (a lane past the wavefront's
            // intervals, like a refused interval, has none)
            for(int t0 = 0; t0 < mine; t0 += TOGETHER) {
                const int src = (t0 + sub) & 63;
                const uint32_t a0 = __shfl(R.lo, src, 64), a1 = __shfl(R.sp.a_end, src, 64), b0 = __shfl(R.sp.b_beg, src, 64), b1 = __shfl(R.hi, src, 64);
                const uint32_t la = a1 - a0, len = t0 + sub < mine ? la + (b1 - b0) : 0u;
                if(!__any(len != 0)) continue;
                uint32_t ps = 0; long long pm = 0, pu = 0;
                for(uint32_t r = part; r < len; r += CRG_LANES) {
                    const uint32_t i = r < la ? a0 + r : b0 + (r - la);
                    const int32_t m = K.m[crg_cell(s, i, K.n)], u = K.u[crg_cell(s, i, K.n)];
                    if(crg_cell_counts(K.pass[i], m, u, K.F.min_depth)) { ps++; pm += m; pu += u; }
                }
                long long pc = ps;
                crg_group_sum(pm, pu, CRG_LANES);
                for(int d = CRG_LANES >> 1; d; d >>= 1) pc += __shfl_xor(pc, d, 64);
                // the owner of interval t0 + q takes group q's sums from the group's first lane
                const int q = lane - t0, from = (q * CRG_LANES) & 63;
                const long long gc = __shfl(pc, from, 64), gm = __shfl(pm, from, 64), gu = __shfl(pu, from, 64);
                if(q >= 0 && q < TOGETHER) { sites += (uint32_t)gc; sm += gm; su += gu; }
            }
            if(has) { const int64_t o = crg_cell(s, j, K.k); K.nsites[o] = (int32_t)sites; K.nmeth[o] = sm; K.nunmeth[o] = su; }
        }
    }
}

// ---- host side: the entry point, on the handle's stream, status block and temporaries ----
extern "C" int md_cohort_regions(md_cohort *h, const void *contig, const void *start, const void *context, const void *strand,
                                 const int32_t *nmeth, const int32_t *nunmeth, int32_t n_samples, int64_t n,
                                 const int32_t *iv_contig, const int32_t *iv_start, const int32_t *iv_end, int64_t k,
                                 uint32_t context_mask, uint32_t strand_mask, int32_t min_depth,
                                 int32_t *out_nsites, int64_t *out_nmeth, int64_t *out_nunmeth) {
    const char *const what = "md_cohort_regions";
    const int64_t top = (int64_t)1 << 30;
    if(!h || n_samples < 1 || n_samples > COH_MAX_SAMPLES || n < 0 || n > top || k < 0 || k > top || context_mask > 7u || strand_mask > 7u || min_depth < 0)
        return fail(MD_COHORT_ERR_ARG, what, hipSuccess);
    if(n && (!contig || !start || !context || !strand || !nmeth || !nunmeth)) return fail(MD_COHORT_ERR_ARG, what, hipSuccess);
    if(k && (!iv_contig || !iv_start || !iv_end || !out_nsites || !out_nmeth || !out_nunmeth)) return fail(MD_COHORT_ERR_ARG, what, hipSuccess);
    if(!h->d_name_off) return fail(MD_COHORT_ERR_ARG, "md_cohort_regions: no contig names (md_cohort_names)", hipSuccess);
    SIDECHK(hipSetDevice(h->device));
    KCrg K;
    memset(&K, 0, sizeof K);
    K.S = n_samples; K.n = n; K.nb = crg_blocks(n); K.k = k; K.n_contigs = h->n_contigs;
    K.sblock = n_samples < h->sblock ? n_samples : h->sblock;
    K.F.context_mask = context_mask; K.F.strand_mask = strand_mask; K.F.min_depth = min_depth;
    const size_t entries = (size_t)crg_entry(n_samples, 0, K.nb);
    if(int rc = h->d_rpass.need((size_t)(n ? n : 1), "md_cohort_regions: the sites' bytes")) return rc;
    if(int rc = h->d_rlo.need((size_t)(k ? k : 1), "md_cohort_regions: the intervals' ranges")) return rc;
    if(int rc = h->d_rhi.need((size_t)(k ? k : 1), "md_cohort_regions: the intervals' ranges")) return rc;
    if(int rc = h->d_rsites.need(entries, "md_cohort_regions: the block table")) return rc;
    if(int rc = h->d_rm.need(entries, "md_cohort_regions: the block table")) return rc;
    if(int rc = h->d_ru.need(entries, "md_cohort_regions: the block table")) return rc;
    K.contig = (const int32_t *)contig; K.start = (const int32_t *)start; K.ctx = (const uint8_t *)context; K.strand = (const int8_t *)strand;
    K.m = nmeth; K.u = nunmeth; K.iv_contig = iv_contig; K.iv_start = iv_start; K.iv_end = iv_end;
    K.pass = h->d_rpass; K.lo = h->d_rlo; K.hi = h->d_rhi; K.pre_sites = h->d_rsites; K.pre_m = h->d_rm; K.pre_u = h->d_ru;
    K.nsites = out_nsites; K.nmeth = out_nmeth; K.nunmeth = out_nunmeth; K.st = h->d_st;
    const int32_t nbt = crg_batches(K.S, K.sblock);
    auto waves = [](int64_t items) { return (items + CRG_WAVES - 1) / CRG_WAVES; };
    h->pin->first = 0;                                                      // the refusals' bits (RGN_E_*), gathered by atomicOr
    SIDECHK(hipMemcpyAsync(h->d_st, h->pin, sizeof(CohStatus), hipMemcpyHostToDevice, h->st));
    if(K.nb) {
        hipLaunchKernelGGL(k_cregion_sites, dim3((uint32_t)crg_grid(K.nb, h->grid)), dim3(CRG_WG), 0, h->st, K);
        hipLaunchKernelGGL(k_cregion_totals, dim3((uint32_t)crg_grid(waves(K.nb * nbt), h->grid)), dim3(CRG_WG), 0, h->st, K);
        hipLaunchKernelGGL(k_cregion_scan, dim3((uint32_t)crg_grid(K.S, h->grid)), dim3(CRG_SCAN_WG), 0, h->st, K);
    }
    if(k) {
        hipLaunchKernelGGL(k_cregion_ranges, dim3((uint32_t)crg_grid((k + CRG_WG - 1) / CRG_WG, h->grid)), dim3(CRG_WG), 0, h->st, K);
        hipLaunchKernelGGL(k_cregion_sum, dim3((uint32_t)crg_grid(waves((k + 63) / 64 * nbt), h->grid)), dim3(CRG_WG), 0, h->st, K);
    }
    SIDECHK(hipGetLastError());
    SIDECHK(hipMemcpyAsync(h->pin, h->d_st, sizeof(CohStatus), hipMemcpyDeviceToHost, h->st));
    SIDECHK(hipStreamSynchronize(h->st));
    const uint32_t err = (uint32_t)h->pin->first;
    if(!err) return 0;
    snprintf(g_err, sizeof g_err, "%s: %s", what,
             err & RGN_E_CONTIG ? "a row's contig is not an index into the contig names" :
             err & RGN_E_CONTEXT ? "a row's context is not 0, 1 or 2" :
             err & RGN_E_ORDER ? "the rows are not ascending in (contig, start), strictly" :
             err & RGN_E_IV_CONTIG ? "an interval's contig is not an index into the contig names" : "an interval has start < 0 or end < start");
    return MD_COHORT_ERR_ARG;
}
