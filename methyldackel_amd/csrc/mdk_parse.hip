// mdk_parse.hip -- text read back into columns on the device (include/mdk_hip.h, "text read back into columns"): the lines of a per-cytosine
// bedGraph become md_calls_cols, those of a cytosine_report.txt md_cytosines_cols.  The inverse of k_text_len / k_text_fill.
//
// The rule is mdk_parse_core.h's: every line that does not begin with `track` is a row, so the row count follows from the line starts alone
// and what is wrong with a line is found when it is parsed.  Measure first, fill second, on the md_text handle -- its stream, its block table
// (one entry per workgroup), its status block and its name table:
//   k_parse_len    a workgroup of 256 owns a span of 4096 bytes of the text, 16 per lane, read as one 16-byte load (the text is 16-byte
//                  aligned; the bytes of the text's last, partial quad singly: nothing past `bytes` is read).  A lane finds the newlines among
//                  its bytes with word arithmetic (prs_newlines); "the byte before my first is a newline" comes from the lane below
//                  (__shfl_up), for lane 0 of a wavefront from global memory -- the byte before the span among them --, and byte 0 starts a
//                  line.  The marks of `track` lines are cleared: their five bytes may run past the lane or the span, so they are read from the
//                  LDS copy of the span and one quad of look-ahead.  Rows = popcount, scanned in the workgroup, the total to the table
//   k_parse_blocks the exclusive scan of those totals as int64 offsets and the row count (text_scan_blocks)
//   k_parse_fill   the same marks and scan again, checked against the recorded total (a text that changed between the two calls ends the fill
//                  with PRS_E_CHANGED and never with a write past the columns).  The span's line starts then go, in order, into a list in
//                  LDS -- a span of newlines has 4096 of them, so the list has 4096 entries and is worked off in rounds of 256 --, and one lane
//                  per line parses from LDS: the span plus PARSE_MAX_LINE bytes of look-ahead, loaded only as far as the text goes.  A line
//                  belongs to the workgroup its first byte lies in.  A lane writes its seven columns at the workgroup's offset + the line's rank
//                  (consecutive lanes, consecutive rows); the contig comes from a binary search over the name index (global memory, the
//                  same few cache lines for every lane), a bedGraph row's strand and context from the five bases around its start in the
//                  resident contig.  A refused line ORs its bit into the status and leaves (its offset << 8 | the refusal's number) in a 64-bit
//                  atomicMin, so the caller learns the refusal of the line that starts earliest
// Integer work on bytes: per row the line itself twice (~25 bytes each for a human bedGraph), five reference bases and 22 bytes of columns.
#include "mdk_text_internal.hpp"
#include "mdk_parse_core.h"
#include <algorithm>
#include <string>

#define PARSE_AHEAD PARSE_MAX_LINE
static_assert(PARSE_SPAN == TEXT_WG * PARSE_LANE, "a span is 16 bytes per lane");

// the 16 bytes of the text at `at` (a multiple of 16), zero past its end
__device__ __forceinline__ uint4 parse_quad(const KParse &K, int64_t at) {
    if(at + PARSE_LANE <= K.bytes) return *(const uint4 *)(K.text + at);
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    for(int i = 0; i < 4; i++) {
        if(at + i < K.bytes) w0 |= (uint32_t)K.text[at + i] << (8 * i);
        if(at + 4 + i < K.bytes) w1 |= (uint32_t)K.text[at + 4 + i] << (8 * i);
        if(at + 8 + i < K.bytes) w2 |= (uint32_t)K.text[at + 8 + i] << (8 * i);
        if(at + 12 + i < K.bytes) w3 |= (uint32_t)K.text[at + 12 + i] << (8 * i);
    }
    return make_uint4(w0, w1, w2, w3);
}

// the workgroup's span, and `ahead` bytes (a multiple of 16) behind it, into img; returns the rows that start among this lane's 16 bytes, a bit each
__device__ __forceinline__ uint32_t parse_marks(const KParse &K, uint8_t *img, uint32_t ahead) {
    const uint32_t t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * PARSE_SPAN, at = base + PARSE_LANE * t;
    const uint4 q = parse_quad(K, at);
    *(uint4 *)(img + PARSE_LANE * t) = q;
    for(uint32_t k = t; k < ahead / PARSE_LANE; k += TEXT_WG) {
        const int64_t a = base + PARSE_SPAN + PARSE_LANE * k;
        if(a < K.bytes) *(uint4 *)(img + PARSE_SPAN + PARSE_LANE * k) = parse_quad(K, a);
    }
    const uint32_t nl = prs_newlines(q.x, q.y, q.z, q.w);
    const uint32_t below = __shfl_up(nl >> 15, 1, 64);           // (every lane of the wavefront takes part)
    bool prev_nl = (below & 1u) != 0;
    if((t & 63u) == 0) prev_nl = at == 0 || (at <= K.bytes && K.text[at - 1] == '\n');
    uint32_t starts = prs_starts(nl, prev_nl, at, K.bytes);
    __syncthreads();
    for(uint32_t m = starts; m; m &= m - 1) {
        const uint32_t k = (uint32_t)__ffs(m) - 1u;
        if(prs_is_track(img + PARSE_LANE * t + k, K.bytes - (at + k))) starts &= ~(1u << k);
    }
    return starts;
}

__global__ __launch_bounds__(TEXT_WG) void k_parse_len(const KParse K) {
    __shared__ uint32_t wtot[TEXT_WG / 64];
    __shared__ __attribute__((aligned(16))) uint8_t img[PARSE_SPAN + PARSE_LANE];
    uint32_t total;
    const uint32_t starts = parse_marks(K, img, PARSE_LANE);
    (void)block_excl_scan<TEXT_WG>((uint32_t)__popc(starts), wtot, total);
    if(threadIdx.x == 0) K.btot[blockIdx.x] = total;
}

__global__ __launch_bounds__(TEXT_SCAN_WG) void k_parse_blocks(const KParse K) {
    __shared__ int64_t wtot[TEXT_SCAN_WG / 64];
    text_scan_blocks(K.btot, K.boff, K.st, (uint32_t)((K.bytes + PARSE_SPAN - 1) / PARSE_SPAN), wtot);
}

__global__ __launch_bounds__(TEXT_WG) void k_parse_fill(const KParse K) {
    __shared__ uint32_t wtot[TEXT_WG / 64];
    __shared__ __attribute__((aligned(16))) uint8_t img[PARSE_SPAN + PARSE_AHEAD];
    __shared__ uint16_t list[PARSE_SPAN];
    uint32_t total;
    const uint32_t starts = parse_marks(K, img, PARSE_AHEAD);
    const uint32_t ex = block_excl_scan<TEXT_WG>((uint32_t)__popc(starts), wtot, total);
    const int64_t off = K.boff[blockIdx.x];
    // another total than the measure recorded, or a place outside the columns: the text is not the measured one
    if(total != K.btot[blockIdx.x] || off < 0 || off + (int64_t)total > K.rows) { if(threadIdx.x == 0) atomicOr(&K.st->err, (uint32_t)PRS_E_CHANGED); return; }
    {
        uint32_t j = ex;
        for(uint32_t m = starts; m; m &= m - 1) list[j++] = (uint16_t)(PARSE_LANE * threadIdx.x + (uint32_t)__ffs(m) - 1u);
    }
    __syncthreads();
    const prs_tab T = {K.name_off, K.names, K.sorted, K.n_contigs, K.ref, K.ref_len};
    const int64_t base = (int64_t)blockIdx.x * PARSE_SPAN;
    for(uint32_t r0 = 0; r0 < total; r0 += TEXT_WG) {
        const uint32_t r = r0 + threadIdx.x;
        if(r >= total) continue;
        const uint32_t s = list[r];
        const int64_t at = base + s;
        prs_row row;
        const uint32_t e = prs_line(img + s, K.bytes - at, K.fmt, T, row);
        if(e) {
            atomicOr(&K.st->err, e);
            atomicMin(&K.st->first, ((unsigned long long)at << 8) | (unsigned long long)(__ffs(e) - 1));
            continue;
        }
        const int64_t o = off + r;
        if(K.fmt == MD_PARSE_CYTOSINE_REPORT) {
            K.cyto.contig[o] = row.contig; K.cyto.pos[o] = row.a; K.cyto.strand[o] = (int8_t)row.strand; K.cyto.nmeth[o] = row.m; K.cyto.nunmeth[o] = row.u;
            K.cyto.context[o] = (uint8_t)row.ctx;
            uint8_t *const tr = K.cyto.trinucleotide + 3 * o;
            tr[0] = row.tri[0]; tr[1] = row.tri[1]; tr[2] = row.tri[2];
        } else {
            K.calls.contig[o] = row.contig; K.calls.start[o] = row.a; K.calls.end[o] = row.b; K.calls.nmeth[o] = row.m; K.calls.nunmeth[o] = row.u;
            K.calls.context[o] = (uint8_t)row.ctx; K.calls.strand[o] = (int8_t)row.strand;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
void text_parse_free(md_text *t) {
    (void)hipFree(t->d_sorted); t->d_sorted = nullptr;
    for(uint8_t *p : t->ref) (void)hipFree(p);
    t->ref.clear(); t->ref_len.clear();
    (void)hipFree(t->d_ref); (void)hipFree(t->d_ref_len); t->d_ref = nullptr; t->d_ref_len = nullptr;
}

// the index of the names, made once: the handle keeps its names on the device alone, so they come back from there
static int parse_index(md_text *t) {
    if(t->d_sorted) return 0;
    const size_t n = (size_t)t->n_contigs;
    std::vector<uint32_t> off(n + 1, 0u), idx(n);
    HIPCHK(hipMemcpy(off.data(), t->d_name_off, (n + 1) * 4, hipMemcpyDeviceToHost));
    std::string names(off[n], '\0');
    if(off[n]) HIPCHK(hipMemcpy(&names[0], t->d_names, off[n], hipMemcpyDeviceToHost));
    for(size_t i = 0; i < n; i++) idx[i] = (uint32_t)i;
    const uint8_t *const b = (const uint8_t *)names.data();
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return prs_name_cmp(b + off[x], off[x + 1] - off[x], b + off[y], off[y + 1] - off[y]) < 0; });
    hipError_t e = hipMalloc((void **)&t->d_sorted, (n + 1) * 4);
    if(e != hipSuccess) { t->d_sorted = nullptr; return fail(MDK_ERR_NOMEM, "hipMalloc(name index)", e); }
    if(n) HIPCHK(hipMemcpy(t->d_sorted, idx.data(), n * 4, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int md_text_reference(md_text *t, int32_t contig, const char *bases, int64_t len) {
    const char *const what = "md_text_reference";
    if(!t || contig < 0 || contig >= t->n_contigs || (bases && len < 0)) return fail(MDK_ERR_ARG, what, hipSuccess);
    HIPCHK(hipSetDevice(t->device));
    const size_t n = (size_t)t->n_contigs;
    if(!t->d_ref) {
        if(!bases) return 0;
        t->ref.assign(n, nullptr); t->ref_len.assign(n, -1);
        hipError_t e = hipMalloc((void **)&t->d_ref, n * sizeof(uint8_t *));
        if(e == hipSuccess) e = hipMalloc((void **)&t->d_ref_len, n * 8);
        if(e == hipSuccess) e = hipMemset(t->d_ref, 0, n * sizeof(uint8_t *));
        if(e == hipSuccess) e = hipMemcpy(t->d_ref_len, t->ref_len.data(), n * 8, hipMemcpyHostToDevice);
        if(e != hipSuccess) { (void)hipFree(t->d_ref); (void)hipFree(t->d_ref_len); t->d_ref = nullptr; t->d_ref_len = nullptr; t->ref.clear(); t->ref_len.clear(); return fail(MDK_ERR_NOMEM, what, e); }
    }
    HIPCHK(hipStreamSynchronize(t->st));
    // the tables first say "none", then the old bases go, then the new ones come
    if(t->ref_len[contig] >= 0) {
        const int64_t none = -1; uint8_t *const null = nullptr;
        HIPCHK(hipMemcpy(t->d_ref_len + contig, &none, 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(t->d_ref + contig, &null, sizeof(null), hipMemcpyHostToDevice));
        (void)hipFree(t->ref[contig]); t->ref[contig] = nullptr; t->ref_len[contig] = -1;
    }
    if(!bases) return 0;
    uint8_t *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, (size_t)len + 16);
    if(e != hipSuccess) return fail(MDK_ERR_NOMEM, "hipMalloc(reference bases)", e);
    if(len) e = hipMemcpy(d, bases, (size_t)len, hipMemcpyHostToDevice);
    if(e == hipSuccess) e = hipMemcpy(t->d_ref + contig, &d, sizeof(d), hipMemcpyHostToDevice);
    if(e == hipSuccess) e = hipMemcpy(t->d_ref_len + contig, &len, 8, hipMemcpyHostToDevice);
    if(e != hipSuccess) { (void)hipFree(d); return fail(MDK_ERR_HIP, what, e); }
    t->ref[contig] = d; t->ref_len[contig] = len;
    return 0;
}

extern "C" int md_text_parse_measure(md_text *t, const uint8_t *text, int64_t bytes, int fmt, int64_t *rows) {
    const char *const what = "md_text_parse_measure";
    if(!t || !rows || bytes < 0 || bytes > (int64_t)INT32_MAX || (bytes && !text) || (fmt != MD_PARSE_BEDGRAPH && fmt != MD_PARSE_CYTOSINE_REPORT)) return fail(MDK_ERR_ARG, what, hipSuccess);
    *rows = 0; t->measured = false; t->merge_measured = false; t->parse_measured = false; t->parse_error_offset = -1;
    if((uintptr_t)text & 15u) return fail(MDK_ERR_ARG, "md_text_parse_measure: the text must be 16-byte aligned", hipSuccess);
    const uint32_t nb = (uint32_t)((bytes + PARSE_SPAN - 1) / PARSE_SPAN);
    HIPCHK(hipSetDevice(t->device));
    { const int rc = parse_index(t); if(rc) return rc; }
    { const int rc = text_blocks_reserve(t, nb); if(rc) return rc; }
    KParse &P = t->P;
    P.text = text; P.bytes = bytes; P.fmt = fmt; P.n_contigs = t->n_contigs; P.name_off = t->d_name_off; P.names = t->d_names; P.sorted = t->d_sorted;
    P.ref = t->d_ref; P.ref_len = t->d_ref_len; P.btot = t->d_btot; P.boff = t->d_boff; P.st = t->d_st;
    P.calls = md_calls_cols(); P.cyto = md_cytosines_cols(); P.rows = 0;
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    if(nb) {
        hipLaunchKernelGGL(k_parse_len, dim3(nb), dim3(TEXT_WG), 0, t->st, P);
        hipLaunchKernelGGL(k_parse_blocks, dim3(1), dim3(TEXT_SCAN_WG), 0, t->st, P);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(t->h_st, t->d_st, sizeof(TextStatus), hipMemcpyDeviceToHost, t->st));
    HIPCHK(hipStreamSynchronize(t->st));
    P.rows = t->h_st->total; t->parse_measured = true;
    *rows = P.rows;
    return 0;
}

static int parse_fill(md_text *t, int fmt, int64_t rows, const char *what) {
    if(!rows) return 0;
    HIPCHK(hipSetDevice(t->device));
    KParse &P = t->P;
    P.ref = t->d_ref; P.ref_len = t->d_ref_len;             // (a reference set after the measure counts)
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    HIPCHK(hipMemsetAsync(&t->d_st->first, 0xff, sizeof(t->d_st->first), t->st));
    hipLaunchKernelGGL(k_parse_fill, dim3((uint32_t)((P.bytes + PARSE_SPAN - 1) / PARSE_SPAN)), dim3(TEXT_WG), 0, t->st, P);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(t->h_st, t->d_st, sizeof(TextStatus), hipMemcpyDeviceToHost, t->st));
    HIPCHK(hipStreamSynchronize(t->st));
    const uint32_t err = t->h_st->err;
    if(!err) return 0;
    if(err & PRS_E_CHANGED || t->h_st->first == ~0ull) { snprintf(mdk_err_buf(), MDK_ERR_BYTES, "%s: %s", what, prs_error_text(PRS_E_CHANGED)); return MDK_ERR_ARG; }
    t->parse_error_offset = (long long)(t->h_st->first >> 8);
    snprintf(mdk_err_buf(), MDK_ERR_BYTES, "%s: %s (the line at byte %lld)", what, prs_error_text(1u << (t->h_st->first & 0xffu)), t->parse_error_offset);
    return MDK_ERR_ARG;
}

extern "C" int md_text_parse_fill_calls(md_text *t, const md_calls_cols *dst, int64_t rows) {
    if(t) t->parse_error_offset = -1;
    if(!t || !t->parse_measured || t->P.fmt != MD_PARSE_BEDGRAPH || !dst || rows != t->P.rows)
        return fail(MDK_ERR_ARG, "md_text_parse_fill_calls: md_text_parse_measure of a bedGraph first, then columns of exactly the measured number of rows", hipSuccess);
    if(rows && (!dst->contig || !dst->start || !dst->end || !dst->nmeth || !dst->nunmeth || !dst->context || !dst->strand)) return fail(MDK_ERR_ARG, "md_text_parse_fill_calls", hipSuccess);
    t->P.calls = *dst;
    return parse_fill(t, MD_PARSE_BEDGRAPH, rows, "md_text_parse_fill_calls");
}

extern "C" int md_text_parse_fill_cytosines(md_text *t, const md_cytosines_cols *dst, int64_t rows) {
    if(t) t->parse_error_offset = -1;
    if(!t || !t->parse_measured || t->P.fmt != MD_PARSE_CYTOSINE_REPORT || !dst || rows != t->P.rows)
        return fail(MDK_ERR_ARG, "md_text_parse_fill_cytosines: md_text_parse_measure of a cytosine report first, then columns of exactly the measured number of rows", hipSuccess);
    if(rows && (!dst->contig || !dst->pos || !dst->strand || !dst->nmeth || !dst->nunmeth || !dst->context || !dst->trinucleotide)) return fail(MDK_ERR_ARG, "md_text_parse_fill_cytosines", hipSuccess);
    t->P.cyto = *dst;
    return parse_fill(t, MD_PARSE_CYTOSINE_REPORT, rows, "md_text_parse_fill_cytosines");
}

extern "C" int64_t md_text_parse_error_offset(const md_text *t) { return t ? (int64_t)t->parse_error_offset : -1; }
