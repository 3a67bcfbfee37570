// mdk_text.hip -- the text of `extract`'s files made on the device from columns (include/mdk_hip.h, "text on the device").
//
// The rows of a session's Calls or Cytosines -- or any column tensors in those layouts, filtered or re-ordered -- become the bytes of a
// bedGraph, a methylKit file or a cytosine report without leaving the device: one device-to-host copy per block of rows then goes to disk.
// The characters are those of csrc/host/mdk_emit.c put_site, from the integer arithmetic of mdk_text_core.h (exact %f and %6.2f included).
// Measure first, fill second, as k_cyto_count / k_cyto_fill size the report's rows:
//   k_text_len     a row per lane, 256 rows per workgroup: the length of the row's line (name length + digit counts + constants; 0 for a row
//                  of another context, or without coverage in a format that prints none), scanned inside the workgroup (wave64 __shfl_up,
//                  wave totals through LDS); the workgroup's total to a table
//   k_text_blocks  one workgroup: the exclusive scan of those totals as int64 offsets, and the byte count of the whole text
//   k_text_fill    the same lengths and scan again (cheaper than a per-row offset written and read back), then the workgroup ASSEMBLES ITS
//                  LINES IN LDS -- every lane writes its line at its scanned offset -- and the whole workgroup streams that image out: 16-byte
//                  stores to 16-byte aligned addresses, consecutive lanes consecutive 16 bytes.  The image sits in LDS at the destination's
//                  misalignment, so an LDS quad IS a global quad; the up to 15 bytes before the first and after the last full quad of a
//                  workgroup's text go out as bytes.  (k_reads_names' form -- a byte per lane, each found by a binary search -- measured
//                  ~41 GB/s.)  A workgroup whose text is longer than the image (contig names of hundreds of bytes) writes its lines straight
//                  to global memory instead.
// perRead's file (MD_TEXT_PERREAD: a row is a read, and carries its own name) goes the same way with kernels of its own:
//   k_rtext_len    the lengths as k_text_len, and the checks of the ragged name columns: offsets inside [0, n_name_bytes], not decreasing,
//                  no name longer than MD_TEXT_NAME_MAX.  It reads the offsets only, never a name
//   k_rtext_fill   the names of a workgroup's 256 rows are ONE span of name_bytes (offsets do not decrease): the workgroup loads that span
//                  into LDS as aligned 16-byte quads (staged at the span's own misalignment, head and tail bytes singly: nothing outside the
//                  span is read), then every lane moves its name from there into the image four bytes at a time (txt_copy_words) and writes
//                  the rest of its line behind it; the image streams out as k_text_fill's does.  Image 30 KB (120 bytes per row) + stage 22 KB
//                  (88 bytes of name per row): three workgroups per CU.  A workgroup whose text or names exceed them writes straight to
//                  global memory, a byte at a time.
//   k_rtext_gather the ragged gather behind Reads.select: name index[i] of the source to dst_off[i] of the destination, assembled in the
//                  image and streamed out in the same way
// k_text_fill re-checks every workgroup's total against what k_text_len recorded: columns that changed between the two calls end the fill
// with an error instead of a write past the buffer.
// The handle, the argument blocks and the scan of the block table are in mdk_text_internal.hpp: mdk_merge.hip (mergeContext over rows) and
// mdk_parse.hip (text read back into columns) work on the same handle.
#include "mdk_text_internal.hpp"
#include "mdk_text_core.h"
#include <string>

#define TEXT_LDS_BYTES (24 * 1024)        // the image: 96 bytes per row (a default bedGraph line of a human contig is ~35, a methylKit one ~55)
#define READS_IMG_BYTES (30 * 1024)       // the reads image: 120 bytes per row (an 80-byte name, a 5-byte contig name and the longest digits: 120)
#define READS_STAGE_BYTES (22 * 1024)     // the staged names: 88 bytes per row.  With the image 53,312 bytes of LDS: three workgroups in a CU's 160 KiB
enum { TEXT_E_CONTIG = 1, TEXT_E_STRAND0 = 2, TEXT_E_CONTEXT = 4, TEXT_E_CHANGED = 8, TEXT_E_OFFSET = 16, TEXT_E_DECREASING = 32, TEXT_E_NAME = 64, TEXT_E_INDEX = 128, TEXT_E_DST = 256 };

struct KGather {
    const int64_t *src_off; const uint8_t *src_bytes; int64_t n_src, n_src_bytes;
    const int64_t *index; uint32_t n; const int64_t *dst_off; uint8_t *dst; int64_t n_dst_bytes; TextStatus *st;
};

// row i of the range: the length of its line (0: no line) and what txt_put_line needs
__device__ __forceinline__ uint32_t text_row(const KText &K, uint32_t i, txt_row &r, const uint8_t *&name, uint32_t &name_len, uint32_t &err) {
    if(i >= K.n) return 0;
    const int64_t at = K.r0 + i;
    const uint32_t ctx = K.v.ctx[at];
    if(K.context >= 0 && ctx != (uint32_t)K.context) return 0;
    const int32_t c = K.v.contig[at];
    if(c < 0 || c >= K.n_contigs) { err |= TEXT_E_CONTIG; return 0; }
    r.a = K.v.a[at]; r.b = K.v.b ? K.v.b[at] : 0; r.m = (uint32_t)K.v.m[at]; r.u = (uint32_t)K.v.u[at];
    r.strand = K.v.strand[at]; r.context = ctx; r.tri = K.v.tri ? K.v.tri + 3 * at : nullptr;
    if(!txt_row_printed(K.fmt, r)) return 0;
    if(K.fmt == MD_TEXT_METHYLKIT && r.strand == 0) { err |= TEXT_E_STRAND0; return 0; }
    if(K.fmt == MD_TEXT_CYTOSINE_REPORT && ctx > 2u) { err |= TEXT_E_CONTEXT; return 0; }
    const uint32_t o = K.name_off[c];
    name = K.names + o; name_len = K.name_off[c + 1] - o;
    return txt_line_len(K.fmt, name_len, r);
}

__global__ __launch_bounds__(TEXT_WG) void k_text_len(const KText K) {
    __shared__ uint32_t wtot[TEXT_WG / 64];
    txt_row r; const uint8_t *name = nullptr; uint32_t name_len = 0, err = 0, total;
    const uint32_t len = text_row(K, blockIdx.x * TEXT_WG + threadIdx.x, r, name, name_len, err);
    if(err) atomicOr(&K.st->err, err);
    (void)block_excl_scan<TEXT_WG>(len, wtot, total);
    if(threadIdx.x == 0) K.btot[blockIdx.x] = total;
}

__global__ __launch_bounds__(TEXT_SCAN_WG) void k_text_blocks(const KText K) {
    __shared__ int64_t wtot[TEXT_SCAN_WG / 64];
    text_scan_blocks(K.btot, K.boff, K.st, (K.n + TEXT_WG - 1) / TEXT_WG, wtot);
}

// a workgroup's image out to g (img[P.sh + i] is g[i]): the whole quads as 16-byte stores, consecutive lanes consecutive quads; the bytes that
// share a quad with the neighbouring workgroups' text singly (at most 15 before and 15 after: one pass of the workgroup each)
__device__ __forceinline__ void text_stream_out(uint8_t *g, const uint8_t *img, const txt_image_plan &P) {
    uint8_t *const g0 = g - P.sh;
    uint4 *const gq = (uint4 *)g0; const uint4 *const lq = (const uint4 *)img;
    for(uint32_t k = P.quad0 + threadIdx.x; k < P.quad1; k += TEXT_WG) gq[k] = lq[k];
    if(P.sh + threadIdx.x < P.head_end) g0[P.sh + threadIdx.x] = img[P.sh + threadIdx.x];
    if(P.tail0 + threadIdx.x < P.end) g0[P.tail0 + threadIdx.x] = img[P.tail0 + threadIdx.x];
}

__global__ __launch_bounds__(TEXT_WG) void k_text_fill(const KText K) {
    __shared__ uint32_t wtot[TEXT_WG / 64];
    __shared__ __attribute__((aligned(16))) uint8_t img[TEXT_LDS_BYTES + 16];
    txt_row r; const uint8_t *name = nullptr; uint32_t name_len = 0, err = 0, total;
    const uint32_t len = text_row(K, blockIdx.x * TEXT_WG + threadIdx.x, r, name, name_len, err);
    const uint32_t ex = block_excl_scan<TEXT_WG>(len, wtot, total);
    const int64_t off = K.boff[blockIdx.x];
    // what k_text_len measured for this workgroup, inside the buffer: anything else means the columns are not the measured ones
    if(total != K.btot[blockIdx.x] || off < 0 || off + (int64_t)total > K.bytes) { if(threadIdx.x == 0) atomicOr(&K.st->err, (uint32_t)TEXT_E_CHANGED); return; }
    if(total == 0) return;
    uint8_t *const g = K.dst + off;
    if(total > TEXT_LDS_BYTES) {             // longer than the image: every lane its own line, straight to global memory
        if(len) txt_put_line((char *)g + ex, K.fmt, name, name_len, r);
        return;
    }
    const txt_image_plan P = txt_plan_image((uint64_t)(uintptr_t)g, total);         // img[P.sh + i] is g[i]: img quad k is the aligned global quad k of g - P.sh
    if(len) txt_put_line((char *)img + P.sh + ex, K.fmt, name, name_len, r);
    __syncthreads();
    text_stream_out(g, img, P);
}

// ---- perRead ----
struct ReadRow { int64_t o; uint32_t name_len, clen, m, u; int32_t pos; const uint8_t *cname; };
// are [o0, o1) the bytes of a name inside n_bytes?
__device__ __forceinline__ uint32_t name_range_error(int64_t o0, int64_t o1, int64_t n_bytes) {
    if(o0 < 0 || o1 < 0 || o0 > n_bytes || o1 > n_bytes) return TEXT_E_OFFSET;
    if(o1 < o0) return TEXT_E_DECREASING;
    return o1 - o0 > MD_TEXT_NAME_MAX ? (uint32_t)TEXT_E_NAME : 0u;
}
// row i of the range: the length of its line (every read has one) and what the fill needs; 0 past the range or for a row that is refused
__device__ __forceinline__ uint32_t reads_row(const KReads &K, uint32_t i, ReadRow &r, uint32_t &err) {
    if(i >= K.n) return 0;
    const int64_t at = K.r0 + i, o0 = K.name_off[at], o1 = K.name_off[at + 1];
    const uint32_t e = name_range_error(o0, o1, K.n_name_bytes);
    if(e) { err |= e; return 0; }
    const int32_t c = K.contig[at];
    if(c < 0 || c >= K.n_contigs) { err |= TEXT_E_CONTIG; return 0; }
    const uint32_t co = K.cname_off[c];
    r.o = o0; r.name_len = (uint32_t)(o1 - o0); r.cname = K.cnames + co; r.clen = K.cname_off[c + 1] - co;
    r.pos = K.pos[at]; r.m = (uint32_t)K.m[at]; r.u = (uint32_t)K.u[at];
    return txt_read_line_len(r.name_len, r.clen, r.pos, r.m, r.u);
}

__global__ __launch_bounds__(TEXT_WG) void k_rtext_len(const KReads K) {
    __shared__ uint32_t wtot[TEXT_WG / 64];
    ReadRow r; uint32_t err = 0, total;
    const uint32_t len = reads_row(K, blockIdx.x * TEXT_WG + threadIdx.x, r, err);
    if(err) atomicOr(&K.st->err, err);
    (void)block_excl_scan<TEXT_WG>(len, wtot, total);
    if(threadIdx.x == 0) K.btot[blockIdx.x] = total;
}

__global__ __launch_bounds__(TEXT_WG) void k_rtext_fill(const KReads K) {
    __shared__ uint32_t wtot[TEXT_WG / 64];
    __shared__ __attribute__((aligned(16))) uint8_t img[READS_IMG_BYTES + 16];
    __shared__ __attribute__((aligned(16))) uint8_t stage[READS_STAGE_BYTES + 32];       // (+ 16 of misalignment, + the word txt_copy_words reads ahead)
    ReadRow r; uint32_t err = 0, total;
    const uint32_t i0 = blockIdx.x * TEXT_WG;
    const uint32_t len = reads_row(K, i0 + threadIdx.x, r, err);
    const uint32_t ex = block_excl_scan<TEXT_WG>(len, wtot, total);
    const int64_t off = K.boff[blockIdx.x];
    // a row the length pass would have refused, or another total than it recorded: the columns are not the measured ones.  Nothing is read or written then
    if(__syncthreads_or(err != 0) || total != K.btot[blockIdx.x] || off < 0 || off + (int64_t)total > K.bytes) { if(threadIdx.x == 0) atomicOr(&K.st->err, (uint32_t)TEXT_E_CHANGED); return; }
    if(total == 0) return;
    uint8_t *const g = K.dst + off;
    // the workgroup's names: one span of name_bytes, from its first row's offset to the one behind its last row (every pair in between was checked)
    const uint32_t rows = K.n - i0 < TEXT_WG ? K.n - i0 : TEXT_WG;
    const int64_t s0 = K.name_off[K.r0 + i0];
    const uint32_t span = (uint32_t)(K.name_off[K.r0 + i0 + rows] - s0);
    if(total > READS_IMG_BYTES || span > READS_STAGE_BYTES) {          // longer than the image or the stage: every lane its own line, straight to global memory
        if(len) txt_put_read_line((char *)g + ex, K.name_bytes + r.o, r.name_len, r.cname, r.clen, r.pos, r.m, r.u);
        return;
    }
    const uint8_t *const src = K.name_bytes + s0;
    const txt_image_plan S = txt_plan_image((uint64_t)(uintptr_t)src, span);         // stage[S.sh + i] is src[i]: a stage quad is an aligned global quad
    {
        const uint8_t *const src0 = src - S.sh;
        const uint4 *const gq = (const uint4 *)src0; uint4 *const lq = (uint4 *)stage;
        for(uint32_t k = S.quad0 + threadIdx.x; k < S.quad1; k += TEXT_WG) lq[k] = gq[k];
        if(S.sh + threadIdx.x < S.head_end) stage[S.sh + threadIdx.x] = src0[S.sh + threadIdx.x];
        if(S.tail0 + threadIdx.x < S.end) stage[S.tail0 + threadIdx.x] = src0[S.tail0 + threadIdx.x];
    }
    const txt_image_plan P = txt_plan_image((uint64_t)(uintptr_t)g, total);
    __syncthreads();
    if(len) {
        uint8_t *const q = img + P.sh + ex;
        txt_copy_words(q, stage, S.sh + (uint32_t)(r.o - s0), r.name_len);
        txt_put_read_tail((char *)q + r.name_len, r.cname, r.clen, r.pos, r.m, r.u);
    }
    __syncthreads();
    text_stream_out(g, img, P);
}

__global__ __launch_bounds__(TEXT_WG) void k_rtext_gather(const KGather K) {
    __shared__ __attribute__((aligned(16))) uint8_t img[TEXT_LDS_BYTES + 16];
    const uint32_t i0 = blockIdx.x * TEXT_WG, i = i0 + threadIdx.x;
    uint32_t err = 0, len = 0; int64_t o = 0, d = 0;
    if(i < K.n) {
        const int64_t j = K.index[i];
        if(j < 0 || j >= K.n_src) err = TEXT_E_INDEX;
        else {
            const int64_t o1 = K.src_off[j + 1], d1 = K.dst_off[i + 1];
            o = K.src_off[j]; d = K.dst_off[i];
            err = name_range_error(o, o1, K.n_src_bytes);
            if(!err && (d < 0 || d1 > K.n_dst_bytes || d1 < d || d1 - d != o1 - o)) err = TEXT_E_DST;
            len = (uint32_t)(o1 - o);
        }
    }
    if(err) atomicOr(&K.st->err, err);
    if(__syncthreads_or(err != 0)) return;
    // every row's destination was checked against its source: the workgroup's bytes are [dst_off of its first row, dst_off behind its last)
    const uint32_t rows = K.n - i0 < TEXT_WG ? K.n - i0 : TEXT_WG;
    const int64_t d0 = K.dst_off[i0];
    const uint32_t total = (uint32_t)(K.dst_off[i0 + rows] - d0);
    if(total == 0) return;
    uint8_t *const g = K.dst + d0;
    const uint8_t *const name = K.src_bytes + o;
    if(total > TEXT_LDS_BYTES) { txt_put_name((char *)g + (d - d0), name, len); return; }
    const txt_image_plan P = txt_plan_image((uint64_t)(uintptr_t)g, total);
    txt_put_name((char *)img + P.sh + (uint32_t)(d - d0), name, len);
    __syncthreads();
    text_stream_out(g, img, P);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int md_text_open(int device, int32_t n_contigs, const char *const *names, md_text **out) {
    if(!out || device < 0 || n_contigs < 0 || (n_contigs && !names)) return fail(MDK_ERR_ARG, "md_text_open", hipSuccess);
    *out = nullptr;
    std::vector<uint32_t> off((size_t)n_contigs + 1, 0u); std::string bytes;
    for(int32_t i = 0; i < n_contigs; i++) {
        const size_t l = names[i] ? strlen(names[i]) : 0;
        if(!names[i] || l > MD_TEXT_NAME_MAX) { snprintf(mdk_err_buf(), MDK_ERR_BYTES, "md_text_open: contig %d has no name or one longer than %d bytes", (int)i, MD_TEXT_NAME_MAX); return MDK_ERR_ARG; }
        bytes.append(names[i], l); off[(size_t)i + 1] = (uint32_t)bytes.size();
    }
    HIPCHK(hipSetDevice(device));
    md_text *t = new md_text(); t->device = device; t->n_contigs = n_contigs;
    hipError_t e = hipStreamCreateWithFlags(&t->st, hipStreamNonBlocking);
    if(e == hipSuccess) e = hipMalloc((void **)&t->d_name_off, off.size() * 4);
    if(e == hipSuccess) e = hipMalloc((void **)&t->d_names, bytes.size() + 16);
    if(e == hipSuccess) e = hipMalloc((void **)&t->d_st, sizeof(TextStatus));
    if(e == hipSuccess) e = hipHostMalloc((void **)&t->h_st, sizeof(TextStatus), hipHostMallocDefault);
    if(e == hipSuccess) e = hipMemcpy(t->d_name_off, off.data(), off.size() * 4, hipMemcpyHostToDevice);
    if(e == hipSuccess && !bytes.empty()) e = hipMemcpy(t->d_names, bytes.data(), bytes.size(), hipMemcpyHostToDevice);
    if(e != hipSuccess) { md_text_close(t); return fail(MDK_ERR_HIP, "md_text_open", e); }
    *out = t;
    return 0;
}

extern "C" void md_text_close(md_text *t) {
    if(!t) return;
    (void)hipSetDevice(t->device);
    if(t->st) { (void)hipStreamSynchronize(t->st); (void)hipStreamDestroy(t->st); }
    text_parse_free(t); text_regions_free(t); text_unite_free(t); text_dmr_free(t); text_deflate_free(t);
    (void)hipFree(t->d_name_off); (void)hipFree(t->d_names); (void)hipFree(t->d_btot); (void)hipFree(t->d_boff); (void)hipFree(t->d_st);
    if(t->h_st) (void)hipHostFree(t->h_st);
    delete t;
}

// the status block back on the host; what the kernels flagged as this call's error
static int text_status(md_text *t, const char *what) {
    HIPCHK(hipMemcpyAsync(t->h_st, t->d_st, sizeof(TextStatus), hipMemcpyDeviceToHost, t->st));
    HIPCHK(hipStreamSynchronize(t->st));
    const uint32_t err = t->h_st->err;
    if(!err) return 0;
    snprintf(mdk_err_buf(), MDK_ERR_BYTES, "%s: %s", what,
             err & TEXT_E_CHANGED ? "the columns are not the ones that were measured" :
             err & TEXT_E_CONTIG ? "a row's contig is not an index into the renderer's names" :
             err & TEXT_E_INDEX ? "an index is not a row of the source" :
             err & TEXT_E_OFFSET ? "a name offset lies outside [0, the number of name bytes]" :
             err & TEXT_E_DECREASING ? "the name offsets decrease" :
             err & TEXT_E_NAME ? "a read name is longer than 255 bytes" :
             err & TEXT_E_DST ? "the destination offsets are not the scan of the selected names' lengths inside the destination" :
             err & TEXT_E_STRAND0 ? "a methylKit line needs the row's strand: --mergeContext rows (strand 0) have none" : "a row's context is not 0, 1 or 2");
    return MDK_ERR_ARG;
}

int text_blocks_reserve(md_text *t, uint32_t nb) {
    if(nb > t->cap_blocks) {
        (void)hipFree(t->d_btot); (void)hipFree(t->d_boff); t->d_btot = nullptr; t->d_boff = nullptr; t->cap_blocks = 0;
        const size_t want = (size_t)nb + nb / 4 + 64;
        hipError_t e = hipMalloc((void **)&t->d_btot, want * 4);
        if(e == hipSuccess) e = hipMalloc((void **)&t->d_boff, want * 8);
        if(e != hipSuccess) return fail(MDK_ERR_NOMEM, "hipMalloc(text block table)", e);
        t->cap_blocks = want;
    }
    return 0;
}

static int text_measure(md_text *t, const TextView &v, int64_t r0, int64_t r1, int fmt, int context, int64_t *bytes, const char *what) {
    if(!t || !bytes || r0 < 0 || r1 < r0 || r1 - r0 > TEXT_MAX_ROWS || context < -1 || context > 2) return fail(MDK_ERR_ARG, what, hipSuccess);
    *bytes = 0; t->measured = false; t->merge_measured = false; t->parse_measured = false;
    const uint32_t n = (uint32_t)(r1 - r0), nb = (n + TEXT_WG - 1) / TEXT_WG;
    if(n && (!v.contig || !v.a || !v.m || !v.u || !v.ctx || !v.strand || (fmt == MD_TEXT_CYTOSINE_REPORT ? !v.tri : !v.b))) return fail(MDK_ERR_ARG, what, hipSuccess);
    HIPCHK(hipSetDevice(t->device));
    { const int rc = text_blocks_reserve(t, nb); if(rc) return rc; }
    KText &K = t->K;
    K.v = v; K.r0 = r0; K.n = n; K.fmt = fmt; K.context = context; K.n_contigs = t->n_contigs; K.name_off = t->d_name_off; K.names = t->d_names;
    K.btot = t->d_btot; K.boff = t->d_boff; K.st = t->d_st; K.dst = nullptr; K.bytes = 0;
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    if(nb) {
        hipLaunchKernelGGL(k_text_len, dim3(nb), dim3(TEXT_WG), 0, t->st, K);
        hipLaunchKernelGGL(k_text_blocks, dim3(1), dim3(TEXT_SCAN_WG), 0, t->st, K);
        HIPCHK(hipGetLastError());
    }
    { const int rc = text_status(t, what); if(rc) return rc; }
    K.bytes = t->h_st->total; t->measured = true; t->reads = false;
    *bytes = K.bytes;
    return 0;
}

extern "C" int md_text_measure_reads(md_text *t, const md_reads_cols *c, int64_t n_name_bytes, int64_t r0, int64_t r1, int64_t *bytes) {
    const char *const what = "md_text_measure_reads";
    if(!t || !c || !bytes || n_name_bytes < 0 || r0 < 0 || r1 < r0 || r1 - r0 > TEXT_MAX_ROWS) return fail(MDK_ERR_ARG, what, hipSuccess);
    *bytes = 0; t->measured = false; t->merge_measured = false; t->parse_measured = false;
    const uint32_t n = (uint32_t)(r1 - r0), nb = (n + TEXT_WG - 1) / TEXT_WG;
    if(n && (!c->contig || !c->pos || !c->nmeth || !c->nunmeth || !c->name_off || (n_name_bytes && !c->name_bytes))) return fail(MDK_ERR_ARG, what, hipSuccess);
    HIPCHK(hipSetDevice(t->device));
    { const int rc = text_blocks_reserve(t, nb); if(rc) return rc; }
    KReads &R = t->R;
    R.contig = c->contig; R.pos = c->pos; R.m = c->nmeth; R.u = c->nunmeth; R.name_off = c->name_off; R.name_bytes = c->name_bytes; R.n_name_bytes = n_name_bytes;
    R.r0 = r0; R.n = n; R.n_contigs = t->n_contigs; R.cname_off = t->d_name_off; R.cnames = t->d_names;
    R.btot = t->d_btot; R.boff = t->d_boff; R.st = t->d_st; R.dst = nullptr; R.bytes = 0;
    KText &K = t->K;                          // (k_text_blocks reads the row count, the tables and the status block of a KText)
    K.n = n; K.btot = t->d_btot; K.boff = t->d_boff; K.st = t->d_st; K.dst = nullptr; K.bytes = 0;
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    if(nb) {
        hipLaunchKernelGGL(k_rtext_len, dim3(nb), dim3(TEXT_WG), 0, t->st, R);
        hipLaunchKernelGGL(k_text_blocks, dim3(1), dim3(TEXT_SCAN_WG), 0, t->st, K);
        HIPCHK(hipGetLastError());
    }
    { const int rc = text_status(t, what); if(rc) return rc; }
    R.bytes = K.bytes = t->h_st->total; t->measured = true; t->reads = true;
    *bytes = R.bytes;
    return 0;
}

extern "C" int md_text_gather_names(md_text *t, const int64_t *src_off, const uint8_t *src_bytes, int64_t n_src, int64_t n_src_bytes,
                                    const int64_t *index, int64_t n, const int64_t *dst_off, uint8_t *dst_bytes, int64_t n_dst_bytes) {
    const char *const what = "md_text_gather_names";
    if(!t || n_src < 0 || n_src_bytes < 0 || n < 0 || n > TEXT_MAX_ROWS || n_dst_bytes < 0) return fail(MDK_ERR_ARG, what, hipSuccess);
    if(!n) return 0;
    if(!src_off || !index || !dst_off || (n_src_bytes && !src_bytes) || (n_dst_bytes && !dst_bytes)) return fail(MDK_ERR_ARG, what, hipSuccess);
    HIPCHK(hipSetDevice(t->device));
    const KGather G = {src_off, src_bytes, n_src, n_src_bytes, index, (uint32_t)n, dst_off, dst_bytes, n_dst_bytes, t->d_st};
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    hipLaunchKernelGGL(k_rtext_gather, dim3(((uint32_t)n + TEXT_WG - 1) / TEXT_WG), dim3(TEXT_WG), 0, t->st, G);
    HIPCHK(hipGetLastError());
    return text_status(t, what);
}

extern "C" int md_text_measure_calls(md_text *t, const md_calls_cols *c, int64_t r0, int64_t r1, int fmt, int context, int64_t *bytes) {
    if(!c || fmt < MD_TEXT_BEDGRAPH || fmt > MD_TEXT_METHYLKIT) return fail(MDK_ERR_ARG, "md_text_measure_calls", hipSuccess);
    const TextView v = {c->contig, c->start, c->end, c->nmeth, c->nunmeth, c->context, c->strand, nullptr};
    return text_measure(t, v, r0, r1, fmt, context, bytes, "md_text_measure_calls");
}

extern "C" int md_text_measure_cytosines(md_text *t, const md_cytosines_cols *c, int64_t r0, int64_t r1, int context, int64_t *bytes) {
    if(!c) return fail(MDK_ERR_ARG, "md_text_measure_cytosines", hipSuccess);
    const TextView v = {c->contig, c->pos, nullptr, c->nmeth, c->nunmeth, c->context, c->strand, c->trinucleotide};
    return text_measure(t, v, r0, r1, MD_TEXT_CYTOSINE_REPORT, context, bytes, "md_text_measure_cytosines");
}

extern "C" int md_text_fill(md_text *t, void *dst, int64_t bytes) {
    if(!t || !t->measured || bytes != t->K.bytes || (bytes && !dst)) return fail(MDK_ERR_ARG, "md_text_fill: md_text_measure_* first, then a buffer of exactly the measured size", hipSuccess);
    if(!bytes) return 0;
    HIPCHK(hipSetDevice(t->device));
    KText &K = t->K; K.dst = (uint8_t *)dst;
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    if(t->reads) { KReads &R = t->R; R.dst = (uint8_t *)dst; hipLaunchKernelGGL(k_rtext_fill, dim3((R.n + TEXT_WG - 1) / TEXT_WG), dim3(TEXT_WG), 0, t->st, R); }
    else hipLaunchKernelGGL(k_text_fill, dim3((K.n + TEXT_WG - 1) / TEXT_WG), dim3(TEXT_WG), 0, t->st, K);
    HIPCHK(hipGetLastError());
    return text_status(t, "md_text_fill");
}
