// mdk_dmr.hip -- significant neighbouring sites joined into regions on the device (include/mdk_hip.h, "sites joined into regions"): the
// rows of a Diff and a mask of the significant ones become differentially methylated regions -- chains of significant rows of one
// direction, each with the pooled counts of its whole span and their Fisher test --, without a file or the host.
//
// The rule is mdk_dmr_core.h's.  Measure first, fill second, on the md_text handle -- its stream, its status block and its contig count
// are what this needs; the tables are this file's own, so a measure of the text, merge, parse or unite kind that waits for its fill is
// left as it is.  A row per lane and 256 per workgroup where the work is per row; NB = the blocks of 256 rows, R = the raw regions:
//   k_dmr_rows     every lane loads its own row once (coalesced); row i - 1 comes from the lane beside it (__shfl_up), for lane 0 of a
//                  wavefront from global memory, and nothing is loaded before row 0.  The row checks (a refusal: its bit into the
//                  status, the smallest refused row by atomicMin), the row's byte of DMR_CODE_* -- candidate or not, and its direction
//                  -- to the code table, and per workgroup the block table: its last candidate row (or none), its candidates and
//                  its four count sums
//   k_dmr_blocks   one workgroup: the five sums scanned in place into exclusive prefixes and the last candidates into "the last
//                  candidate before block b" (a max-scan), 4096 blocks a round with a carry; entry NB holds the totals
//   k_dmr_heads    a candidate's previous candidate: inside its wavefront the highest set bit below its lane of the 64-bit ballot of
//                  the candidate flags, else the last candidate of an earlier wavefront (LDS), else the block table's entry.  The head
//                  flag per the rule; a wavefront's heads go out as ONE 64-bit mask, a workgroup's count to the head table
//   k_dmr_scan     one workgroup: the head table scanned (text_scan_blocks) -- the raw regions before each block, and R
//   (the host reads the status and R: a refused row ends the call here, and the tables per region are sized)
//   k_dmr_bounds   a row per lane again: a head's ordinal r is its block's offset plus the heads before it (popcount of the masks); it
//                  writes first[r] = i and, with its previous candidate p found as above, last[r - 1] = p.  last[R - 1] is the last
//                  candidate of all.  Every entry has one writer: no atomics
//   k_dmr_sum      64 raw regions per wavefront.  First a lane per region: the whole blocks inside [f, l] as the difference of two
//                  prefix entries.  Then the wavefront together, one of its regions after the other: the rows of the two partial blocks
//                  at the ends -- at most 255 + 255 -- read coalesced, reduced over the lanes and added to the owner's sums.  Then the
//                  margin check, the keep flag, and the kept regions' places inside the workgroup (ballot and popcount)
//   k_dmr_scan     again, over the kept per workgroup: the kept before each, and n_out
//   (the host reads the status and n_out: the end of the measure)
//   k_dmr_fill     a lane per raw region; a kept one writes its twelve columns at its place, diff_pvalue among them
// Apart from the issue's five kernels: the ordinals of the heads need the scan of the blocks' head counts, and that needs every block's
// count first -- so the heads take two row kernels (k_dmr_heads, k_dmr_bounds) with the one-workgroup scan between them; and a byte per
// row carries candidate and direction from k_dmr_rows on, so that the later kernels read one byte a row and not its four counts again.
// Bounded by: k_dmr_rows 45 bytes read and 1 written per row; k_dmr_heads and k_dmr_bounds a byte per row, 9 more per candidate and
// its predecessor; k_dmr_sum per region, whatever its span, ten prefix entries and at most 510 rows of 33 bytes; k_dmr_fill the
// divisions of diff_pvalue per kept region.  Temporaries: 1 1/8 bytes per row, 56 per block, 48 per raw region.
// Integer work apart from diff_meth and diff_pvalue, whose doubles are under mdk_diff_core.h's no-contract rule.  Nothing is read
// before row 0 or past row n - 1; first and last are this file's own, so a fill reads no row the measure did not.  Plain C++, vector
// loads and stores.
#include "mdk_text_internal.hpp"
#include "mdk_dmr_core.h"

#define DMR_WAVES (TEXT_WG / 64)
static_assert(TEXT_WG == DMR_ROWS, "a workgroup of rows is a block of the tables");

// the sum of the five over the wavefront, in every lane
__device__ __forceinline__ void dmr_wave_sum(uint32_t &k, long long &a, long long &b, long long &c, long long &d) {
    for(int s = 32; s; s >>= 1) { k += __shfl_xor(k, s, 64); a += __shfl_xor(a, s, 64); b += __shfl_xor(b, s, 64); c += __shfl_xor(c, s, 64); d += __shfl_xor(d, s, 64); }
}

__global__ __launch_bounds__(TEXT_WG) void k_dmr_rows(const KDmr K) {
    __shared__ int32_t wl[DMR_WAVES];
    __shared__ uint32_t wk[DMR_WAVES];
    __shared__ long long ws[4][DMR_WAVES];
    const uint32_t i = blockIdx.x * TEXT_WG + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool has = i < K.n;
    int32_t contig = 0, start = 0; long long a = 0, b = 0, c = 0, d = 0; int sig = 0;
    if(has) { contig = K.contig[i]; start = K.start[i]; a = K.a[i]; b = K.b[i]; c = K.c[i]; d = K.d[i]; sig = K.sig[i]; }
    // (every lane of the wavefront takes part in the moves, rows or not)
    int32_t pcontig = __shfl_up(contig, 1, 64), pstart = __shfl_up(start, 1, 64);
    uint32_t code = DMR_CODE_NONE;
    if(has) {
        int has_prev = 1;
        if(lane == 0) { has_prev = i > 0; if(has_prev) { pcontig = K.contig[i - 1]; pstart = K.start[i - 1]; } }
        const uint32_t err = dmr_row_check(has_prev, pcontig, pstart, contig, start, K.n_contigs, a, b, c, d);
        if(err) {
            atomicOr(&K.st->err, err);
            atomicMin(&K.st->first, ((unsigned long long)i << 8) | (unsigned long long)(__ffs(err) - 1));
        }
        if(err & (DMR_E_NEGATIVE | DMR_E_ENTRY)) a = b = c = d = 0;          // (a refused row's counts are not added: the sums stay below 2^56)
        else code = dmr_code(sig, a, b, c, d);
        K.code[i] = (uint8_t)code;
    }
    const unsigned long long m = __ballot(code != DMR_CODE_NONE);
    uint32_t k = code != DMR_CODE_NONE;
    dmr_wave_sum(k, a, b, c, d);
    if(lane == 0) {
        const int top = dmr_last_in_mask(m);
        wl[wave] = top < 0 ? DMR_NO_ROW : (int32_t)(blockIdx.x * TEXT_WG + wave * 64 + top);
        wk[wave] = k; ws[0][wave] = a; ws[1][wave] = b; ws[2][wave] = c; ws[3][wave] = d;
    }
    __syncthreads();
    if(threadIdx.x == 0) {
        int32_t top = wl[0];
        for(int w = 1; w < DMR_WAVES; w++) { if(wl[w] > top) top = wl[w]; k += wk[w]; a += ws[0][w]; b += ws[1][w]; c += ws[2][w]; d += ws[3][w]; }
        K.blast[blockIdx.x] = top; K.bcand[blockIdx.x] = k;
        K.ba[blockIdx.x] = a; K.bb[blockIdx.x] = b; K.bc[blockIdx.x] = c; K.bd[blockIdx.x] = d;
    }
}

// one column of block totals, in place: entry b becomes the sum of the totals of the blocks before b, entry nb the sum of all.  A thread
// takes DMR_SCAN_PER neighbouring entries a round, and one column comes after the other (as k_region_blocks, for its reasons)
#define DMR_SCAN_PER 4
template <typename T>
__device__ __forceinline__ void dmr_scan_sums(T *col, uint32_t nb, int64_t *wtot) {
    int64_t carry = 0;
    for(uint32_t b0 = 0; b0 < nb; b0 += TEXT_SCAN_WG * DMR_SCAN_PER) {          // (uniform trip count: every thread takes part in every scan)
        const uint32_t b = b0 + threadIdx.x * DMR_SCAN_PER;
        int64_t v[DMR_SCAN_PER], sum = 0, total;
#pragma unroll
        for(int q = 0; q < DMR_SCAN_PER; q++) { v[q] = b + q < nb ? (int64_t)col[b + q] : 0; sum += v[q]; }
        int64_t run = carry + block_excl_scan<TEXT_SCAN_WG>(sum, wtot, total);
#pragma unroll
        for(int q = 0; q < DMR_SCAN_PER; q++) { if(b + q < nb) col[b + q] = (T)run; run += v[q]; }
        carry += total;
    }
    if(threadIdx.x == 0) col[nb] = (T)carry;
}

// the largest of the values of the threads before this one in the workgroup (DMR_NO_ROW: none), and of all of them
__device__ __forceinline__ int32_t dmr_excl_max(int32_t v, int32_t *wtop, int32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t x = v;
    for(int s = 1; s < 64; s <<= 1) { const int32_t y = __shfl_up(x, s, 64); if(lane >= s && y > x) x = y; }
    int32_t ex = __shfl_up(x, 1, 64);
    if(lane == 0) ex = DMR_NO_ROW;
    if(lane == 63) wtop[wave] = x;
    __syncthreads();
    total = DMR_NO_ROW;
    for(int w = 0; w < TEXT_SCAN_WG / 64; w++) { const int32_t t = wtop[w]; if(w < wave && t > ex) ex = t; if(t > total) total = t; }
    __syncthreads();                 // (wtop is rewritten by the next round)
    return ex;
}

// the blocks' last candidates, in place: entry b becomes the last candidate of the blocks before b, entry nb the last of all
__device__ __forceinline__ void dmr_scan_last(int32_t *col, uint32_t nb, int32_t *wtop) {
    int32_t carry = DMR_NO_ROW;
    for(uint32_t b0 = 0; b0 < nb; b0 += TEXT_SCAN_WG * DMR_SCAN_PER) {
        const uint32_t b = b0 + threadIdx.x * DMR_SCAN_PER;
        int32_t v[DMR_SCAN_PER], top = DMR_NO_ROW, total;
#pragma unroll
        for(int q = 0; q < DMR_SCAN_PER; q++) { v[q] = b + q < nb ? col[b + q] : DMR_NO_ROW; if(v[q] > top) top = v[q]; }
        int32_t run = dmr_excl_max(top, wtop, total);
        if(carry > run) run = carry;
#pragma unroll
        for(int q = 0; q < DMR_SCAN_PER; q++) { if(b + q < nb) col[b + q] = run; if(v[q] > run) run = v[q]; }
        if(total > carry) carry = total;
    }
    if(threadIdx.x == 0) col[nb] = carry;
}

__global__ __launch_bounds__(TEXT_SCAN_WG) void k_dmr_blocks(const KDmr K) {
    __shared__ int64_t wtot[TEXT_SCAN_WG / 64];
    __shared__ int32_t wtop[TEXT_SCAN_WG / 64];
    const uint32_t nb = (K.n + TEXT_WG - 1) / TEXT_WG;
    dmr_scan_last(K.blast, nb, wtop);
    dmr_scan_sums(K.bcand, nb, wtot);
    dmr_scan_sums(K.ba, nb, wtot);
    dmr_scan_sums(K.bb, nb, wtot);
    dmr_scan_sums(K.bc, nb, wtot);
    dmr_scan_sums(K.bd, nb, wtot);
}

// the previous candidate of this lane's row, or DMR_NO_ROW; `code` is the row's byte (DMR_CODE_NONE past row n - 1).  Every thread of the
// workgroup calls it: there is a barrier inside, which also publishes what the caller wrote to LDS before
__device__ __forceinline__ int32_t dmr_prev_candidate(const KDmr &K, uint32_t code, int32_t *wl) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t base = (int32_t)(blockIdx.x * TEXT_WG + wave * 64);
    const unsigned long long m = __ballot(code != DMR_CODE_NONE);
    if(lane == 0) { const int top = dmr_last_in_mask(m); wl[wave] = top < 0 ? DMR_NO_ROW : base + top; }
    __syncthreads();
    const int near = dmr_prev_in_mask(m, lane);
    if(near >= 0) return base + near;
    for(int w = wave - 1; w >= 0; w--) if(wl[w] != DMR_NO_ROW) return wl[w];
    return K.blast[blockIdx.x];
}

__global__ __launch_bounds__(TEXT_WG) void k_dmr_heads(const KDmr K) {
    __shared__ int32_t wl[DMR_WAVES];
    __shared__ uint32_t wh[DMR_WAVES];
    const uint32_t i = blockIdx.x * TEXT_WG + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t code = i < K.n ? K.code[i] : (uint32_t)DMR_CODE_NONE;
    const int32_t p = dmr_prev_candidate(K, code, wl);
    bool head = false;
    if(code != DMR_CODE_NONE)
        head = p == DMR_NO_ROW || !dmr_continues(K.contig[p], K.start[p], K.code[p], p, K.contig[i], K.start[i], code, (int32_t)i, K.max_gap, K.max_skip);
    const unsigned long long hm = __ballot(head);
    if(lane == 0) { K.hmask[blockIdx.x * DMR_WAVES + wave] = hm; wh[wave] = (uint32_t)__popcll(hm); }
    __syncthreads();
    if(threadIdx.x == 0) { uint32_t h = 0; for(int w = 0; w < DMR_WAVES; w++) h += wh[w]; K.htot[blockIdx.x] = h; }
}

// one workgroup: a table of totals into the int64 offsets before each entry, their sum into the status block
__global__ __launch_bounds__(TEXT_SCAN_WG) void k_dmr_scan(const uint32_t *tot, int64_t *off, TextStatus *st, uint32_t nb) {
    __shared__ int64_t wtot[TEXT_SCAN_WG / 64];
    text_scan_blocks(tot, off, st, nb, wtot);
}

__global__ __launch_bounds__(TEXT_WG) void k_dmr_bounds(const KDmr K) {
    __shared__ int32_t wl[DMR_WAVES];
    __shared__ uint32_t wh[DMR_WAVES];
    const uint32_t i = blockIdx.x * TEXT_WG + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t code = i < K.n ? K.code[i] : (uint32_t)DMR_CODE_NONE;
    const unsigned long long hm = K.hmask[blockIdx.x * DMR_WAVES + wave];
    if(lane == 0) wh[wave] = (uint32_t)__popcll(hm);
    const int32_t p = dmr_prev_candidate(K, code, wl);                   // (its barrier stands between wh's writers and readers, too)
    if(hm >> lane & 1ull) {
        int64_t r = K.hoff[blockIdx.x] + (int64_t)__popcll(hm & ((1ull << lane) - 1ull));
        for(int w = 0; w < wave; w++) r += wh[w];
        if(r >= 0 && r < (int64_t)K.n_raw) {                             // (it is: n_raw is the sum of what is counted here)
            K.first[r] = (int32_t)i;
            if(r > 0) K.last[r - 1] = p;                                 // (a head that is not the first candidate has a candidate before it)
        }
    }
    if(i == 0) K.last[K.n_raw - 1] = K.blast[(K.n + TEXT_WG - 1) / TEXT_WG];
}

__global__ __launch_bounds__(TEXT_WG) void k_dmr_sum(const KDmr K) {
    __shared__ uint32_t wk[DMR_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t r0 = (blockIdx.x * DMR_WAVES + wave) * 64;          // the wavefront's first region
    const uint32_t r = r0 + lane;
    const bool has = r < K.n_raw;
    // a lane per region: its span [f, l] as the half-open [lo, hi), and what whole blocks give
    uint32_t lo = 0, hi = 0, nsig = 0; long long a = 0, b = 0, c = 0, d = 0;
    rgn_split sp; sp.a_end = sp.b_beg = sp.b0 = sp.b1 = 0;
    if(has) {
        const int32_t f = K.first[r], l = K.last[r];
        if(f >= 0 && l >= f && (uint32_t)l < K.n) {                      // (they are: both are rows k_dmr_bounds wrote)
            lo = (uint32_t)f; hi = (uint32_t)l + 1u;
            sp = rgn_split_range(lo, hi);
            if(sp.b0 < sp.b1) {
                nsig = K.bcand[sp.b1] - K.bcand[sp.b0];
                a = K.ba[sp.b1] - K.ba[sp.b0]; b = K.bb[sp.b1] - K.bb[sp.b0]; c = K.bc[sp.b1] - K.bc[sp.b0]; d = K.bd[sp.b1] - K.bd[sp.b0];
            }
        }
    }
    // the wavefront per region: rows [lo, a_end) and [b_beg, hi), 64 at a time
    const uint32_t mine = r0 < K.n_raw ? (K.n_raw - r0 < 64u ? K.n_raw - r0 : 64u) : 0u;
    for(uint32_t t = 0; t < mine; t++) {
        const uint32_t a0 = __shfl(lo, t, 64), a1 = __shfl(sp.a_end, t, 64), b0 = __shfl(sp.b_beg, t, 64), b1 = __shfl(hi, t, 64);
        const uint32_t la = a1 - a0, len = la + (b1 - b0);
        if(!len) continue;
        uint32_t pk = 0; long long pa = 0, pb = 0, pc = 0, pd = 0;
        for(uint32_t q = lane; q < len; q += 64) {
            const uint32_t i = q < la ? a0 + q : b0 + (q - la);
            pk += K.code[i] != DMR_CODE_NONE; pa += K.a[i]; pb += K.b[i]; pc += K.c[i]; pd += K.d[i];
        }
        dmr_wave_sum(pk, pa, pb, pc, pd);
        if(lane == (int)t) { nsig += pk; a += pa; b += pb; c += pc; d += pd; }
    }
    // the margins, the filter, and the kept regions' places among the workgroup's
    bool keep = false;
    if(has && hi > lo) {
        const uint32_t err = diff_margin_check(a, b, c, d);
        if(err) {
            atomicOr(&K.st->err, err);
            atomicMin(&K.st->first, ((unsigned long long)lo << 8) | (unsigned long long)(__ffs(err) - 1));
        } else keep = dmr_keep((int32_t)nsig, a, b, c, d, dmr_code_dir(K.code[lo]), K.min_sites, K.min_diff);
        K.rnsig[r] = (int32_t)nsig; K.ra[r] = a; K.rb[r] = b; K.rc[r] = c; K.rd[r] = d;
    }
    const unsigned long long km = __ballot(keep);
    if(lane == 0) wk[wave] = (uint32_t)__popcll(km);
    __syncthreads();
    uint32_t place = (uint32_t)__popcll(km & ((1ull << lane) - 1ull));
    for(int w = 0; w < wave; w++) place += wk[w];
    if(has) K.rpos[r] = keep ? place : DMR_NO_PLACE;
    if(threadIdx.x == 0) { uint32_t kept = 0; for(int w = 0; w < DMR_WAVES; w++) kept += wk[w]; K.ktot[blockIdx.x] = kept; }
}

__global__ __launch_bounds__(TEXT_WG) void k_dmr_fill(const KDmr K) {
    const uint32_t r = blockIdx.x * TEXT_WG + threadIdx.x;
    if(r >= K.n_raw) return;
    const uint32_t place = K.rpos[r];
    if(place == DMR_NO_PLACE) return;
    const int64_t o = K.koff[blockIdx.x] + (int64_t)place;
    if(o < 0 || o >= K.n_out) return;                                    // (it is inside: n_out is the sum of what was placed)
    const int32_t f = K.first[r], l = K.last[r];
    const int64_t a = K.ra[r], b = K.rb[r], c = K.rc[r], d = K.rd[r];
    K.o_contig[o] = K.contig[f]; K.o_start[o] = K.start[f]; K.o_end[o] = K.end[l];
    K.o_nsites[o] = l - f + 1; K.o_nsig[o] = K.rnsig[r]; K.o_dir[o] = (int8_t)dmr_code_dir(K.code[f]);
    K.o_a[o] = a; K.o_b[o] = b; K.o_c[o] = c; K.o_d[o] = d;
    K.o_diff[o] = diff_meth(a, b, c, d);
    K.o_p[o] = diff_pvalue(a, b, c, d, nullptr);
}

// a device buffer that grows and is kept (as mdk_unite.hip's)
template <typename T> struct DmrBuf {
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

struct DmrState {
    DmrBuf<uint8_t> code; DmrBuf<unsigned long long> hmask;
    DmrBuf<int32_t> blast, first, last, rnsig; DmrBuf<uint32_t> bcand, htot, rpos, ktot;
    DmrBuf<int64_t> ba, bb, bc, bd, hoff, ra, rb, rc, rd, koff;
    KDmr K; bool measured = false;
};

void text_dmr_free(md_text *t) {
    DmrState *s = t->dmr;
    if(!s) return;
    s->code.release(); s->hmask.release(); s->blast.release(); s->first.release(); s->last.release(); s->rnsig.release();
    s->bcand.release(); s->htot.release(); s->rpos.release(); s->ktot.release();
    s->ba.release(); s->bb.release(); s->bc.release(); s->bd.release(); s->hoff.release();
    s->ra.release(); s->rb.release(); s->rc.release(); s->rd.release(); s->koff.release();
    delete s; t->dmr = nullptr;
}

// the status block back on the host; what the kernels flagged as this call's error
static int dmr_status(md_text *t, const char *what) {
    HIPCHK(hipMemcpyAsync(t->h_st, t->d_st, sizeof(TextStatus), hipMemcpyDeviceToHost, t->st));
    HIPCHK(hipStreamSynchronize(t->st));
    if(!t->h_st->err) return 0;
    const uint32_t bit = 1u << (t->h_st->first & 0xffu);
    snprintf(mdk_err_buf(), MDK_ERR_BYTES, "%s: %s (row %lld)", what,
             bit == DMR_E_NEGATIVE ? "a count is negative" :
             bit == DMR_E_ENTRY ? "a count is 2^26 or more" :
             bit == DMR_E_ORDER ? "the rows are not ascending in (contig, start), strictly" :
             bit == DMR_E_CONTIG ? "a row's contig is not an index into the contig names" :
             "a region's pooled margin (a group's depth, or the methylated or the unmethylated of both) is 2^26 or more: the region begins at the row named",
             (long long)(t->h_st->first >> 8));
    return MDK_ERR_ARG;
}

extern "C" int md_text_dmr_measure(md_text *t, const int32_t *contig, const int32_t *start, const int32_t *end, const uint8_t *context, const int8_t *strand,
                                   const int64_t *nmeth_a, const int64_t *nunmeth_a, const int64_t *nmeth_b, const int64_t *nunmeth_b, const uint8_t *significant,
                                   int64_t n, int32_t n_contigs, int32_t max_gap, int32_t max_skip, int32_t min_sites, double min_diff, int64_t *n_regions) {
    const char *const what = "md_text_dmr_measure";
    (void)context; (void)strand;                                        // (a Diff's columns; the rule reads neither)
    if(!t || !n_regions || n < 0 || n > DMR_MAX_ROWS || n_contigs < 0 || max_gap < 0 || max_skip < 0 || min_sites < 1 || !(min_diff >= 0.0) || min_diff > 1.7976931348623157e308)
        return fail(MDK_ERR_ARG, what, hipSuccess);
    if(n && (!contig || !start || !end || !nmeth_a || !nunmeth_a || !nmeth_b || !nunmeth_b || !significant)) return fail(MDK_ERR_ARG, what, hipSuccess);
    *n_regions = 0;
    if(!t->dmr) t->dmr = new DmrState();
    DmrState *s = t->dmr;
    s->measured = false;
    KDmr &K = s->K;
    K = KDmr();
    K.contig = contig; K.start = start; K.end = end; K.a = nmeth_a; K.b = nunmeth_a; K.c = nmeth_b; K.d = nunmeth_b; K.sig = significant;
    K.n = (uint32_t)n; K.n_contigs = n_contigs; K.max_gap = max_gap; K.max_skip = max_skip; K.min_sites = min_sites; K.min_diff = min_diff;
    K.st = t->d_st;
    if(!n) { s->measured = true; return 0; }
    HIPCHK(hipSetDevice(t->device));
    const uint32_t nb = (uint32_t)((n + TEXT_WG - 1) / TEXT_WG);
    { int rc = s->code.need((size_t)n, "hipMalloc(dmr row codes)"); if(!rc) rc = s->hmask.need((size_t)nb * DMR_WAVES, "hipMalloc(dmr head masks)");
      if(!rc) rc = s->blast.need((size_t)nb + 1, "hipMalloc(dmr block table)"); if(!rc) rc = s->bcand.need((size_t)nb + 1, "hipMalloc(dmr block table)");
      if(!rc) rc = s->ba.need((size_t)nb + 1, "hipMalloc(dmr block table)"); if(!rc) rc = s->bb.need((size_t)nb + 1, "hipMalloc(dmr block table)");
      if(!rc) rc = s->bc.need((size_t)nb + 1, "hipMalloc(dmr block table)"); if(!rc) rc = s->bd.need((size_t)nb + 1, "hipMalloc(dmr block table)");
      if(!rc) rc = s->htot.need(nb, "hipMalloc(dmr head table)"); if(!rc) rc = s->hoff.need(nb, "hipMalloc(dmr head table)"); if(rc) return rc; }
    K.code = s->code.p; K.hmask = s->hmask.p; K.blast = s->blast.p; K.bcand = s->bcand.p; K.ba = s->ba.p; K.bb = s->bb.p; K.bc = s->bc.p; K.bd = s->bd.p;
    K.htot = s->htot.p; K.hoff = s->hoff.p;
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    HIPCHK(hipMemsetAsync(&t->d_st->first, 0xff, sizeof(t->d_st->first), t->st));
    hipLaunchKernelGGL(k_dmr_rows, dim3(nb), dim3(TEXT_WG), 0, t->st, K);
    hipLaunchKernelGGL(k_dmr_blocks, dim3(1), dim3(TEXT_SCAN_WG), 0, t->st, K);
    hipLaunchKernelGGL(k_dmr_heads, dim3(nb), dim3(TEXT_WG), 0, t->st, K);
    hipLaunchKernelGGL(k_dmr_scan, dim3(1), dim3(TEXT_SCAN_WG), 0, t->st, (const uint32_t *)K.htot, K.hoff, K.st, nb);
    HIPCHK(hipGetLastError());
    { const int rc = dmr_status(t, what); if(rc) return rc; }
    const int64_t raw = t->h_st->total;
    if(raw < 0 || raw > n) return fail(MDK_ERR_HIP, "md_text_dmr_measure: the head count is outside the rows", hipSuccess);
    if(!raw) { s->measured = true; return 0; }                         // no candidate at all
    // the raw regions: their bounds, their sums, the kept ones' places
    K.n_raw = (uint32_t)raw;
    const uint32_t nrb = (K.n_raw + TEXT_WG - 1) / TEXT_WG;
    { int rc = s->first.need(K.n_raw, "hipMalloc(dmr regions)"); if(!rc) rc = s->last.need(K.n_raw, "hipMalloc(dmr regions)"); if(!rc) rc = s->rnsig.need(K.n_raw, "hipMalloc(dmr regions)");
      if(!rc) rc = s->rpos.need(K.n_raw, "hipMalloc(dmr regions)"); if(!rc) rc = s->ra.need(K.n_raw, "hipMalloc(dmr regions)"); if(!rc) rc = s->rb.need(K.n_raw, "hipMalloc(dmr regions)");
      if(!rc) rc = s->rc.need(K.n_raw, "hipMalloc(dmr regions)"); if(!rc) rc = s->rd.need(K.n_raw, "hipMalloc(dmr regions)");
      if(!rc) rc = s->ktot.need(nrb, "hipMalloc(dmr kept table)"); if(!rc) rc = s->koff.need(nrb, "hipMalloc(dmr kept table)"); if(rc) return rc; }
    K.first = s->first.p; K.last = s->last.p; K.rnsig = s->rnsig.p; K.rpos = s->rpos.p; K.ra = s->ra.p; K.rb = s->rb.p; K.rc = s->rc.p; K.rd = s->rd.p;
    K.ktot = s->ktot.p; K.koff = s->koff.p;
    hipLaunchKernelGGL(k_dmr_bounds, dim3(nb), dim3(TEXT_WG), 0, t->st, K);
    hipLaunchKernelGGL(k_dmr_sum, dim3(nrb), dim3(TEXT_WG), 0, t->st, K);
    hipLaunchKernelGGL(k_dmr_scan, dim3(1), dim3(TEXT_SCAN_WG), 0, t->st, (const uint32_t *)K.ktot, K.koff, K.st, nrb);
    HIPCHK(hipGetLastError());
    { const int rc = dmr_status(t, what); if(rc) return rc; }
    K.n_out = t->h_st->total; s->measured = true;
    *n_regions = K.n_out;
    return 0;
}

extern "C" int md_text_dmr_fill(md_text *t, int32_t *contig, int32_t *start, int32_t *end, int32_t *nsites, int32_t *nsig, int8_t *direction,
                                int64_t *nmeth_a, int64_t *nunmeth_a, int64_t *nmeth_b, int64_t *nunmeth_b, double *meth_diff, double *pvalue, int64_t n_regions) {
    const char *const what = "md_text_dmr_fill";
    DmrState *s = t ? t->dmr : nullptr;
    if(!s || !s->measured || n_regions != s->K.n_out) return fail(MDK_ERR_ARG, "md_text_dmr_fill: md_text_dmr_measure first, then columns of exactly the measured number of regions", hipSuccess);
    if(!n_regions) return 0;
    if(!contig || !start || !end || !nsites || !nsig || !direction || !nmeth_a || !nunmeth_a || !nmeth_b || !nunmeth_b || !meth_diff || !pvalue) return fail(MDK_ERR_ARG, what, hipSuccess);
    HIPCHK(hipSetDevice(t->device));
    KDmr &K = s->K;
    K.o_contig = contig; K.o_start = start; K.o_end = end; K.o_nsites = nsites; K.o_nsig = nsig; K.o_dir = direction;
    K.o_a = nmeth_a; K.o_b = nunmeth_a; K.o_c = nmeth_b; K.o_d = nunmeth_b; K.o_diff = meth_diff; K.o_p = pvalue;
    hipLaunchKernelGGL(k_dmr_fill, dim3((K.n_raw + TEXT_WG - 1) / TEXT_WG), dim3(TEXT_WG), 0, t->st, K);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(t->st));
    return 0;
}
