// mdk_unite.hip -- samples' rows joined into one site table on the device (include/mdk_hip.h, "samples joined into one site table"):
// the table of the sites at least min_samples of S Calls hold, with the counts of every sample per site, without a key per row, a
// sort or the host -- what methylKit calls `unite`.
//
// The rule is mdk_unite_core.h's: (contig, start) is a bounded integer domain and every sample ascends in it, so the union of the
// samples' sites is a bitmap and a site's place in the union the rank of its bit.  Measure first, fill second, on the md_text handle --
// its stream, its status block and its contig count are what this needs; the tables are this file's own, so a measure of the text, merge
// or parse kind that waits for its fill is left as it is.  A row per lane and 256 per workgroup; blockIdx.y is the sample:
//   k_unite_rows     the row check of k_region_rows (row i - 1 from the lane beside it, for lane 0 of a wavefront from global memory,
//                    nothing before row 0 of a sample), and the last row of a contig in a sample -- the row before a row of another
//                    contig, and the sample's last -- gives atomicMax(extent[contig], start + 1)
//   k_unite_offsets  one workgroup: the extents rounded up to whole words and scanned, in 64 bits, into the contigs' first words
//   (the host reads the word count: more than 2^30 words is refused before anything is allocated; the bitmap is set to zero)
//   k_unite_mark     every present row sets its bit.  The rows ascend, so the lanes of a wavefront that share a word are neighbours: their
//                    bits are combined by a segmented OR over the lanes, and the last lane of a run issues ONE atomicOr whose result
//                    nobody reads -- at CpG density a handful of atomics a wavefront instead of 64
//   k_unite_count    four words a lane (one 16-byte load): the bits set per block of 16 words, to the block table
//   k_unite_blocks   one workgroup: a block table scanned in place into exclusive prefixes, 1024 entries a round with a carry in 64
//                    bits, the grand total to the status block (text_scan_blocks' loop; used for the words' blocks and for the sites')
//   k_unite_ranks    four words a lane again: the exclusive rank of every word, as uint32
//   (the host reads n_union)
//   k_unite_tally    every present row finds its site (uni_locate) and adds 1 to its count; the row whose add returned 0 is the site's
//                    writer: its sample's index goes to owner[site]
//   k_unite_keep     keep = count >= min_samples, scanned inside the workgroup: map[site] = the place among the workgroup's kept sites,
//                    the workgroup's total to the sites' block table; then k_unite_blocks over that table gives n_out
//   (the host reads n_out: the end of the measure)
//   k_unite_sites    the writer's row of every kept site writes contig, start, end, context, strand and nsamples at the site's place
//   k_unite_fill     every present row of a kept site writes its two counts at [sample, place], indexed in 64 bits, and compares its
//                    end, context and strand with what k_unite_sites wrote: a difference is UNI_E_DISAGREE
// The host waits three times in a measure, each time for one number it must have to size the next table (words, n_union, n_out).
// Temporaries: bitmap + ranks (the extent / 4 bytes together) + 1/16 of either for the block table + 12 bytes per union site; nothing
// grows with S x n but the result.  Integer atomics only, so the result is the same from run to run; which row is a site's writer is
// not, and does not matter: every other row of the site is compared with it.
// Nothing is read before row 0 or past row n - 1 of a sample.  The fill locates every row anew with every index checked (uni_word,
// uni_locate, uni_place): columns that changed since the measure end it with an error or give other numbers, never a write outside
// the result.
#include "mdk_text_internal.hpp"
#include "mdk_unite_core.h"

__device__ __forceinline__ uni_tables unite_tables(const KUnite &K) {
    uni_tables T; T.extent = K.extent; T.base = K.base; T.bits = K.bits; T.rankw = K.rankw; T.n_contigs = K.n_contigs; T.n_words = K.n_words; T.n_union = K.n_union;
    return T;
}

__global__ __launch_bounds__(UNI_ROWS) void k_unite_rows(const KUnite K) {
    const UniSample s = K.S[blockIdx.y];
    const uint32_t i = blockIdx.x * UNI_ROWS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool has = i < s.n;
    int32_t contig = 0, start = 0, ctx = 0;
    if(has) { contig = s.contig[i]; start = s.start[i]; ctx = s.ctx[i]; }
    // (every lane of the wavefront takes part in the moves, rows or not)
    int32_t pcontig = __shfl_up(contig, 1, 64), pstart = __shfl_up(start, 1, 64);
    if(!has) return;
    int has_prev = 1;
    if(lane == 0) { has_prev = i > 0; if(has_prev) { pcontig = s.contig[i - 1]; pstart = s.start[i - 1]; } }
    const uint32_t err = uni_row_check(has_prev, pcontig, pstart, contig, start, ctx, K.n_contigs);
    if(err) atomicOr(&K.st->err, err);
    // the last row of a contig in this sample (a row that is refused for its contig or start names no entry)
    if(has_prev && pcontig != contig && pcontig >= 0 && pcontig < K.n_contigs && pstart >= 0) atomicMax(&K.extent[pcontig], (uint32_t)pstart + 1u);
    if(i == s.n - 1 && !(err & (UNI_E_CONTIG | UNI_E_START))) atomicMax(&K.extent[contig], (uint32_t)start + 1u);
}

__global__ __launch_bounds__(UNI_SCAN) void k_unite_offsets(const KUnite K) {
    __shared__ int64_t wtot[UNI_SCAN / 64];
    int64_t carry = 0;
    for(int32_t c0 = 0; c0 < K.n_contigs; c0 += UNI_SCAN) {          // (uniform trip count: every thread takes part in every scan)
        const int32_t c = c0 + (int32_t)threadIdx.x;
        const int64_t v = c < K.n_contigs ? (int64_t)uni_words(K.extent[c]) : 0;
        int64_t total;
        const int64_t ex = block_excl_scan<UNI_SCAN>(v, wtot, total);
        if(c < K.n_contigs) K.base[c] = carry + ex;
        carry += total;
    }
    if(threadIdx.x == 0) K.st->total = carry;
}

__global__ __launch_bounds__(UNI_ROWS) void k_unite_mark(const KUnite K) {
    const UniSample s = K.S[blockIdx.y];
    const uint32_t i = blockIdx.x * UNI_ROWS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t w = UNI_NONE, bit = 0;
    if(i < s.n) {
        const int32_t start = s.start[i];
        const int64_t at = uni_word(unite_tables(K), s.contig[i], start);
        if(at >= 0) { w = (uint32_t)at; if(uni_present(s.m[i], s.u[i], K.min_depth)) bit = uni_bit(start); }
    }
    // the OR of the bits of the lanes at and below this one that share its word: equal words are neighbours
    for(int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(bit, d, 64), yw = __shfl_up(w, d, 64);
        if(lane >= d && yw == w) bit |= y;
    }
    const uint32_t nw = __shfl_down(w, 1, 64);
    if(bit && (lane == 63 || nw != w)) atomicOr(&K.bits[w], bit);          // (w is a word: a lane without one has no bit)
}

// the sum of v over the 4 lanes that share a block of UNI_BLOCK_WORDS words, in each of them
__device__ __forceinline__ uint32_t unite_words_popc(const KUnite &K, uint32_t t, uint32_t &p0, uint32_t &p1, uint32_t &p2, uint32_t &p3) {
    p0 = p1 = p2 = p3 = 0;
    if((int64_t)t * 4 < K.n_words) { const uint4 v = ((const uint4 *)K.bits)[t]; p0 = uni_popc(v.x); p1 = uni_popc(v.y); p2 = uni_popc(v.z); p3 = uni_popc(v.w); }
    return p0 + p1 + p2 + p3;
}

__global__ __launch_bounds__(UNI_ROWS) void k_unite_count(const KUnite K) {
    const uint32_t t = blockIdx.x * UNI_ROWS + threadIdx.x;
    uint32_t p0, p1, p2, p3;
    uint32_t sum = unite_words_popc(K, t, p0, p1, p2, p3);
    sum += __shfl_xor(sum, 1, 64); sum += __shfl_xor(sum, 2, 64);
    if((t & 3u) == 0 && (int64_t)t * 4 < K.n_words) K.btot[t >> 2] = sum;
}

__global__ __launch_bounds__(UNI_SCAN) void k_unite_blocks(uint32_t *tot, uint32_t nb, TextStatus *st) {
    __shared__ int64_t wtot[UNI_SCAN / 64];
    int64_t carry = 0;
    for(uint32_t b0 = 0; b0 < nb; b0 += UNI_SCAN) {                  // (uniform trip count: every thread takes part in every scan)
        const uint32_t b = b0 + threadIdx.x;
        const int64_t v = b < nb ? (int64_t)tot[b] : 0;
        int64_t total;
        const int64_t ex = block_excl_scan<UNI_SCAN>(v, wtot, total);
        if(b < nb) tot[b] = (uint32_t)(carry + ex);                  // (a total above 2^30 is refused by the host: these are not used then)
        carry += total;
    }
    if(threadIdx.x == 0) st->total = carry;
}

__global__ __launch_bounds__(UNI_ROWS) void k_unite_ranks(const KUnite K) {
    const uint32_t t = blockIdx.x * UNI_ROWS + threadIdx.x;
    const int sub = threadIdx.x & 3;
    uint32_t p0, p1, p2, p3;
    const uint32_t sum = unite_words_popc(K, t, p0, p1, p2, p3);
    uint32_t x = sum;
    for(int d = 1; d < 4; d <<= 1) { const uint32_t y = __shfl_up(x, d, 64); if(sub >= d) x += y; }
    if((int64_t)t * 4 >= K.n_words) return;
    const uint32_t r = K.btot[t >> 2] + x - sum;
    ((uint4 *)K.rankw)[t] = make_uint4(r, r + p0, r + p0 + p1, r + p0 + p1 + p2);
}

// the site of row i of sample s if the row is present: UNI_NONE for a row that is not; a present row without a site flags UNI_E_CHANGED
__device__ __forceinline__ uint32_t unite_site(const KUnite &K, const UniSample &s, uint32_t i, int32_t &contig, int32_t &start) {
    if(i >= s.n || !uni_present(s.m[i], s.u[i], K.min_depth)) return UNI_NONE;
    contig = s.contig[i]; start = s.start[i];
    const uint32_t r = uni_locate(unite_tables(K), contig, start);
    if(r == UNI_NONE) atomicOr(&K.st->err, (uint32_t)UNI_E_CHANGED);
    return r;
}

__global__ __launch_bounds__(UNI_ROWS) void k_unite_tally(const KUnite K) {
    const UniSample s = K.S[blockIdx.y];
    int32_t contig, start;
    const uint32_t r = unite_site(K, s, blockIdx.x * UNI_ROWS + threadIdx.x, contig, start);
    if(r == UNI_NONE) return;
    if(atomicAdd(&K.count[r], 1u) == 0u) K.owner[r] = blockIdx.y;
}

__global__ __launch_bounds__(UNI_ROWS) void k_unite_keep(const KUnite K) {
    __shared__ uint32_t wtot[UNI_ROWS / 64];
    const uint32_t r = blockIdx.x * UNI_ROWS + threadIdx.x;
    const uint32_t keep = r < K.n_union && K.count[r] >= (uint32_t)K.min_samples;
    uint32_t total;
    const uint32_t ex = block_excl_scan<UNI_ROWS>(keep, wtot, total);
    if(r < K.n_union) K.map[r] = keep ? ex : UNI_NONE;
    if(threadIdx.x == 0) K.ktot[blockIdx.x] = total;
}

__global__ __launch_bounds__(UNI_ROWS) void k_unite_sites(const KUnite K) {
    const UniSample s = K.S[blockIdx.y];
    const uint32_t i = blockIdx.x * UNI_ROWS + threadIdx.x;
    int32_t contig, start;
    const uint32_t r = unite_site(K, s, i, contig, start);
    if(r == UNI_NONE || K.owner[r] != blockIdx.y) return;
    const int64_t o = uni_place(K.ktot, K.map, r);
    if(o < 0) return;
    if(o >= K.n_out) { atomicOr(&K.st->err, (uint32_t)UNI_E_CHANGED); return; }
    K.o_contig[o] = contig; K.o_start[o] = start; K.o_end[o] = s.end[i]; K.o_ctx[o] = s.ctx[i]; K.o_strand[o] = s.strand[i];
    K.o_nsamples[o] = (int32_t)K.count[r];
}

__global__ __launch_bounds__(UNI_ROWS) void k_unite_fill(const KUnite K) {
    const UniSample s = K.S[blockIdx.y];
    const uint32_t i = blockIdx.x * UNI_ROWS + threadIdx.x;
    int32_t contig, start;
    const uint32_t r = unite_site(K, s, i, contig, start);
    if(r == UNI_NONE) return;
    const int64_t o = uni_place(K.ktot, K.map, r);
    if(o < 0) return;
    if(o >= K.n_out) { atomicOr(&K.st->err, (uint32_t)UNI_E_CHANGED); return; }
    const int64_t at = (int64_t)blockIdx.y * K.n_out + o;
    K.o_m[at] = s.m[i]; K.o_u[at] = s.u[i];
    if(!uni_agree(s.end[i], s.ctx[i], s.strand[i], K.o_end[o], K.o_ctx[o], K.o_strand[o])) atomicOr(&K.st->err, (uint32_t)UNI_E_DISAGREE);
}

// a device buffer that only grows (as regions_reserve's table)
template <typename T> struct UniBuf {
    T *p = nullptr; size_t cap = 0;
    int need(size_t n, const char *what) {
        if(n <= cap) return 0;
        release();
        const size_t want = n + n / 8 + 64;
        const hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if(e != hipSuccess) { p = nullptr; return fail(MDK_ERR_NOMEM, what, e); }
        cap = want; return 0;
    }
    void release() { if(p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct UniteState {
    std::vector<UniSample> samples; UniBuf<UniSample> d_samples;
    UniBuf<uint32_t> extent, bits, rankw, btot, count, owner, map, ktot; UniBuf<int64_t> base;
    KUnite K; uint32_t max_rows = 0; bool measured = false;
};

void text_unite_free(md_text *t) {
    UniteState *u = t->unite;
    if(!u) return;
    u->d_samples.release(); u->extent.release(); u->bits.release(); u->rankw.release(); u->btot.release();
    u->count.release(); u->owner.release(); u->map.release(); u->ktot.release(); u->base.release();
    delete u; t->unite = nullptr;
}

// the status block back on the host; what the kernels flagged as this call's error
static int unite_status(md_text *t, const char *what) {
    HIPCHK(hipMemcpyAsync(t->h_st, t->d_st, sizeof(TextStatus), hipMemcpyDeviceToHost, t->st));
    HIPCHK(hipStreamSynchronize(t->st));
    const uint32_t err = t->h_st->err;
    if(!err) return 0;
    snprintf(mdk_err_buf(), MDK_ERR_BYTES, "%s: %s", what,
             err & UNI_E_CHANGED ? "the columns are not the ones that were measured" :
             err & UNI_E_CONTIG ? "a row's contig is not an index into the contig names" :
             err & UNI_E_CONTEXT ? "a row's context is not 0, 1 or 2" :
             err & UNI_E_START ? "a row's start is negative" :
             err & UNI_E_ORDER ? "the rows of a sample are not ascending in (contig, start), strictly" : "samples disagree about a site: its end, context or strand");
    return MDK_ERR_ARG;
}

static dim3 unite_grid(const UniteState *u) { return dim3((u->max_rows + UNI_ROWS - 1) / UNI_ROWS, (uint32_t)u->K.n_samples); }

extern "C" int md_text_unite_measure(md_text *t, const md_calls_cols *samples, int32_t n_samples, const int64_t *n_rows, int32_t min_samples, int32_t min_depth,
                                     int64_t *n_union, int64_t *n_out) {
    const char *const what = "md_text_unite_measure";
    if(!t || !samples || !n_rows || !n_union || !n_out || n_samples < 1 || n_samples > UNI_MAX_SAMPLES || min_samples < 1 || min_samples > n_samples || min_depth < 0)
        return fail(MDK_ERR_ARG, what, hipSuccess);
    *n_union = *n_out = 0;
    if(!t->unite) t->unite = new UniteState();
    UniteState *u = t->unite;
    u->measured = false; u->max_rows = 0;
    u->samples.resize((size_t)n_samples);
    for(int32_t k = 0; k < n_samples; k++) {
        const md_calls_cols &c = samples[k];
        if(n_rows[k] < 0 || n_rows[k] > TEXT_MAX_ROWS) return fail(MDK_ERR_ARG, what, hipSuccess);
        if(n_rows[k] && (!c.contig || !c.start || !c.end || !c.nmeth || !c.nunmeth || !c.context || !c.strand)) return fail(MDK_ERR_ARG, what, hipSuccess);
        UniSample &s = u->samples[(size_t)k];
        s.contig = c.contig; s.start = c.start; s.end = c.end; s.m = c.nmeth; s.u = c.nunmeth; s.ctx = c.context; s.strand = c.strand; s.n = (uint32_t)n_rows[k]; s.pad = 0;
        if(s.n > u->max_rows) u->max_rows = s.n;
    }
    HIPCHK(hipSetDevice(t->device));
    const size_t nc = (size_t)(t->n_contigs > 0 ? t->n_contigs : 1);
    { int rc = u->d_samples.need((size_t)n_samples, "hipMalloc(unite samples)"); if(!rc) rc = u->extent.need(nc, "hipMalloc(unite extents)"); if(!rc) rc = u->base.need(nc, "hipMalloc(unite bases)"); if(rc) return rc; }
    KUnite &K = u->K;
    K = KUnite();
    K.S = u->d_samples.p; K.n_samples = n_samples; K.n_contigs = t->n_contigs; K.min_samples = min_samples; K.min_depth = min_depth;
    K.extent = u->extent.p; K.base = u->base.p; K.st = t->d_st;
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    HIPCHK(hipMemsetAsync(K.extent, 0, nc * sizeof(uint32_t), t->st));
    HIPCHK(hipMemcpyAsync(u->d_samples.p, u->samples.data(), (size_t)n_samples * sizeof(UniSample), hipMemcpyHostToDevice, t->st));
    if(u->max_rows) hipLaunchKernelGGL(k_unite_rows, unite_grid(u), dim3(UNI_ROWS), 0, t->st, K);
    hipLaunchKernelGGL(k_unite_offsets, dim3(1), dim3(UNI_SCAN), 0, t->st, K);
    HIPCHK(hipGetLastError());
    { const int rc = unite_status(t, what); if(rc) return rc; }
    const int64_t words = t->h_st->total;
    if(words > UNI_MAX_WORDS) {
        snprintf(mdk_err_buf(), MDK_ERR_BYTES, "%s: the contigs' covered extents add up to more than 2^35 bits (%lld words of 32)", what, (long long)words);
        return MDK_ERR_ARG;
    }
    if(!words) { u->measured = true; return 0; }                     // no rows at all
    // the bitmap, its ranks and its block table
    K.n_words = (words + UNI_BLOCK_WORDS - 1) / UNI_BLOCK_WORDS * UNI_BLOCK_WORDS;
    const uint32_t nb = (uint32_t)(K.n_words / UNI_BLOCK_WORDS), quads = (uint32_t)(K.n_words / 4);
    { int rc = u->bits.need((size_t)K.n_words, "hipMalloc(unite bitmap)"); if(!rc) rc = u->rankw.need((size_t)K.n_words, "hipMalloc(unite ranks)"); if(!rc) rc = u->btot.need(nb, "hipMalloc(unite block table)"); if(rc) return rc; }
    K.bits = u->bits.p; K.rankw = u->rankw.p; K.btot = u->btot.p;
    HIPCHK(hipMemsetAsync(K.bits, 0, (size_t)K.n_words * sizeof(uint32_t), t->st));
    hipLaunchKernelGGL(k_unite_mark, unite_grid(u), dim3(UNI_ROWS), 0, t->st, K);
    hipLaunchKernelGGL(k_unite_count, dim3((quads + UNI_ROWS - 1) / UNI_ROWS), dim3(UNI_ROWS), 0, t->st, K);
    hipLaunchKernelGGL(k_unite_blocks, dim3(1), dim3(UNI_SCAN), 0, t->st, K.btot, nb, K.st);
    hipLaunchKernelGGL(k_unite_ranks, dim3((quads + UNI_ROWS - 1) / UNI_ROWS), dim3(UNI_ROWS), 0, t->st, K);
    HIPCHK(hipGetLastError());
    { const int rc = unite_status(t, what); if(rc) return rc; }
    const int64_t sites = t->h_st->total;
    if(sites > UNI_MAX_SITES) {
        snprintf(mdk_err_buf(), MDK_ERR_BYTES, "%s: %lld sites in the union: more than 2^30", what, (long long)sites);
        return MDK_ERR_ARG;
    }
    *n_union = sites;
    if(!sites) { u->measured = true; return 0; }                     // rows, none of them present
    // the tally and the kept sites' places
    K.n_union = (uint32_t)sites;
    const uint32_t nkb = (K.n_union + UNI_ROWS - 1) / UNI_ROWS;
    { int rc = u->count.need(K.n_union, "hipMalloc(unite counts)"); if(!rc) rc = u->owner.need(K.n_union, "hipMalloc(unite writers)"); if(!rc) rc = u->map.need(K.n_union, "hipMalloc(unite places)");
      if(!rc) rc = u->ktot.need(nkb, "hipMalloc(unite site block table)"); if(rc) return rc; }
    K.count = u->count.p; K.owner = u->owner.p; K.map = u->map.p; K.ktot = u->ktot.p;
    HIPCHK(hipMemsetAsync(K.count, 0, (size_t)K.n_union * sizeof(uint32_t), t->st));
    hipLaunchKernelGGL(k_unite_tally, unite_grid(u), dim3(UNI_ROWS), 0, t->st, K);
    hipLaunchKernelGGL(k_unite_keep, dim3(nkb), dim3(UNI_ROWS), 0, t->st, K);
    hipLaunchKernelGGL(k_unite_blocks, dim3(1), dim3(UNI_SCAN), 0, t->st, K.ktot, nkb, K.st);
    HIPCHK(hipGetLastError());
    { const int rc = unite_status(t, what); if(rc) return rc; }
    K.n_out = t->h_st->total; u->measured = true;
    *n_out = K.n_out;
    return 0;
}

extern "C" int md_text_unite_fill(md_text *t, int32_t *contig, int32_t *start, int32_t *end, uint8_t *context, int8_t *strand, int32_t *nsamples, int32_t *nmeth, int32_t *nunmeth, int64_t n_out) {
    const char *const what = "md_text_unite_fill";
    UniteState *u = t ? t->unite : nullptr;
    if(!u || !u->measured || n_out != u->K.n_out) return fail(MDK_ERR_ARG, "md_text_unite_fill: md_text_unite_measure first, then columns of exactly the measured number of sites", hipSuccess);
    if(!n_out) return 0;
    if(!contig || !start || !end || !context || !strand || !nsamples || !nmeth || !nunmeth) return fail(MDK_ERR_ARG, what, hipSuccess);
    HIPCHK(hipSetDevice(t->device));
    KUnite &K = u->K;
    K.o_contig = contig; K.o_start = start; K.o_end = end; K.o_ctx = context; K.o_strand = strand; K.o_nsamples = nsamples; K.o_m = nmeth; K.o_u = nunmeth;
    const size_t cells = (size_t)K.n_samples * (size_t)n_out;
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    HIPCHK(hipMemsetAsync(nmeth, 0, cells * sizeof(int32_t), t->st));
    HIPCHK(hipMemsetAsync(nunmeth, 0, cells * sizeof(int32_t), t->st));
    hipLaunchKernelGGL(k_unite_sites, unite_grid(u), dim3(UNI_ROWS), 0, t->st, K);
    hipLaunchKernelGGL(k_unite_fill, unite_grid(u), dim3(UNI_ROWS), 0, t->st, K);
    HIPCHK(hipGetLastError());
    return unite_status(t, what);
}
