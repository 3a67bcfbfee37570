// mdk_text_internal.hpp -- what the sources behind a md_text handle share (mdk_text.hip: the text; mdk_merge.hip: mergeContext's rows;
// mdk_parse.hip: text read back into columns; mdk_regions.hip: sums over intervals; mdk_unite.hip: samples joined into one site table; mdk_diff.hip: two groups of samples compared; mdk_dmr.hip: significant sites joined into regions): the
// handle itself -- its stream, the name table, the table of one entry per 256 rows, the status block --, the kernels' argument blocks and the
// scan of the block table.
#ifndef MDK_TEXT_INTERNAL_HPP
#define MDK_TEXT_INTERNAL_HPP
#include "mdk_hip_internal.hpp"

#define TEXT_WG 256
#define TEXT_SCAN_WG 1024
#define TEXT_MAX_ROWS (1ll << 30)         // rows of one measure / fill

struct TextStatus { int64_t total; uint32_t err, pad; unsigned long long first; };      // first: mdk_parse.hip, the refused line that starts earliest (offset << 8 | refusal); mdk_diff.hip, the first refused site; mdk_dmr.hip, the first refused row
// the columns of either layout: a = start (calls) or pos (cytosines), b = end (calls only), tri = trinucleotide (cytosines only)
struct TextView { const int32_t *contig, *a, *b, *m, *u; const uint8_t *ctx; const int8_t *strand; const uint8_t *tri; };
struct KText {
    TextView v; int64_t r0; uint32_t n; int32_t fmt, context, n_contigs;
    const uint32_t *name_off; const uint8_t *names;          // name c = names[name_off[c] .. name_off[c + 1])
    uint32_t *btot; int64_t *boff; TextStatus *st;
    uint8_t *dst; int64_t bytes;
};

// the Reads layout: name i = name_bytes[name_off[i] .. name_off[i + 1]), offsets into n_name_bytes bytes
struct KReads {
    const int32_t *contig, *pos, *m, *u; const int64_t *name_off; const uint8_t *name_bytes; int64_t n_name_bytes;
    int64_t r0; uint32_t n; int32_t n_contigs;
    const uint32_t *cname_off; const uint8_t *cnames;         // the renderer's contig names
    uint32_t *btot; int64_t *boff; TextStatus *st;
    uint8_t *dst; int64_t bytes;
};

// mergeContext over rows (mdk_merge.hip): the measured columns, and where the fill writes
struct KMerge {
    const int32_t *contig, *start, *end, *m, *u; const uint8_t *ctx; const int8_t *strand;
    uint32_t n; int32_t n_contigs, min_depth;
    uint32_t *btot; int64_t *boff; TextStatus *st;
    md_calls_cols dst; int64_t rows;
};

// text read back into columns (mdk_parse.hip): the measured text, what its lines are looked up in, and where the fill writes
struct KParse {
    const uint8_t *text; int64_t bytes; int32_t fmt, n_contigs;
    const uint32_t *name_off; const uint8_t *names; const uint32_t *sorted;      // sorted: the contig indices in ascending order of their names
    const uint8_t *const *ref; const int64_t *ref_len;                            // the resident bases per contig (ref_len < 0: none)
    uint32_t *btot; int64_t *boff; TextStatus *st;
    md_calls_cols calls; md_cytosines_cols cyto; int64_t rows;
};

// sums of rows over intervals (mdk_regions.hip): the rows, the intervals, the filter, the prefix table of one entry per 256 rows, the result
struct KRegion {
    const int32_t *contig, *start, *m, *u; const uint8_t *ctx; const int8_t *strand;
    uint32_t n; int32_t n_contigs;
    const int32_t *iv_contig, *iv_start, *iv_end; uint32_t k;
    uint32_t context_mask, strand_mask; int32_t min_depth;
    uint32_t *pre_sites; int64_t *pre_m, *pre_u; TextStatus *st;          // nb + 1 entries each: block totals, scanned in place
    int32_t *nsites; int64_t *nmeth, *nunmeth;
};

// samples joined into one site table (mdk_unite.hip): a sample's columns and rows; the samples, the tables of mdk_unite_core.h, the result
struct UniSample { const int32_t *contig, *start, *end, *m, *u; const uint8_t *ctx; const int8_t *strand; uint32_t n, pad; };
struct KUnite {
    const UniSample *S; int32_t n_samples, n_contigs, min_samples, min_depth;
    uint32_t *extent; int64_t *base;                                      // per contig: bits covered, first word
    uint32_t *bits, *rankw, *btot; int64_t n_words;                       // n_words: a multiple of UNI_BLOCK_WORDS; btot: an entry per UNI_BLOCK_WORDS words, scanned in place
    uint32_t *count, *owner, *map, *ktot; uint32_t n_union;               // per union site; ktot: an entry per UNI_ROWS sites, scanned in place
    TextStatus *st;
    int32_t *o_contig, *o_start, *o_end; uint8_t *o_ctx; int8_t *o_strand; int32_t *o_nsamples, *o_m, *o_u; int64_t n_out;
};
struct UniteState;                                                        // mdk_unite.hip: its buffers and what was measured

// two groups of samples compared site by site (mdk_diff.hip): the two count matrices [n_samples, n] of int32 or int64, the samples' marks
// (0: group A, 1: group B, -1: not used), the six results
struct KDiff {
    const void *m, *u; const int32_t *group; int32_t n_samples; int64_t n;
    int64_t *a, *b, *c, *d; double *diff, *p; TextStatus *st;
};

// significant neighbouring sites joined into regions (mdk_dmr.hip): the rows and the parameters; the tables per row, per block of 256 rows
// and per raw region (all mdk_dmr.hip's own); the result
struct KDmr {
    const int32_t *contig, *start, *end; const int64_t *a, *b, *c, *d; const uint8_t *sig;
    uint32_t n; int32_t n_contigs, max_gap, max_skip, min_sites; double min_diff;
    uint8_t *code; unsigned long long *hmask;                             // per row: DMR_CODE_*; per wavefront of rows: its heads as a mask
    int32_t *blast; uint32_t *bcand; int64_t *ba, *bb, *bc, *bd;          // nb + 1 entries each, scanned in place: the last candidate before the block (entry nb: of all), candidates and counts before it
    uint32_t *htot; int64_t *hoff;                                        // the blocks' heads, and the raw regions before each block
    uint32_t n_raw; int32_t *first, *last, *rnsig; uint32_t *rpos; int64_t *ra, *rb, *rc, *rd;      // per raw region; rpos: its place among the kept of its 256, or DMR_NO_PLACE
    uint32_t *ktot; int64_t *koff;                                        // per 256 raw regions: the kept, and the kept before them
    TextStatus *st;
    int32_t *o_contig, *o_start, *o_end, *o_nsites, *o_nsig; int8_t *o_dir; int64_t *o_a, *o_b, *o_c, *o_d; double *o_diff, *o_p; int64_t n_out;
};
struct DmrState;                                                          // mdk_dmr.hip: its buffers and what was measured
struct DeflateState;                                                      // mdk_deflate.hip: the members' slots, lengths and token strips, and what was measured

struct md_text {
    int device = 0; hipStream_t st = nullptr; int32_t n_contigs = 0;
    uint32_t *d_name_off = nullptr; uint8_t *d_names = nullptr;
    uint32_t *d_btot = nullptr; int64_t *d_boff = nullptr; size_t cap_blocks = 0;
    TextStatus *d_st = nullptr, *h_st = nullptr;
    KText K; KReads R; bool measured = false, reads = false;          // reads: the range measured last is one of md_text_measure_reads
    KMerge M; bool merge_measured = false;                            // the block table holds md_text_merge_measure's totals (one table: a measure of either kind voids the other's)
    KParse P; bool parse_measured = false;                            // ... or md_text_parse_measure's
    uint32_t *d_sorted = nullptr;                                     // mdk_parse.hip, made by the first parse: the name index
    std::vector<uint8_t *> ref; std::vector<int64_t> ref_len;         // md_text_reference: the contigs' bases on the device (host copies of the two tables below)
    uint8_t **d_ref = nullptr; int64_t *d_ref_len = nullptr;
    long long parse_error_offset = -1;
    uint32_t *d_rsites = nullptr; int64_t *d_rm = nullptr, *d_ru = nullptr; size_t cap_rblocks = 0;      // mdk_regions.hip: its prefix table, apart from d_btot / d_boff
    UniteState *unite = nullptr;                                      // mdk_unite.hip, made by the first md_text_unite_measure: tables of its own, too
    DmrState *dmr = nullptr;                                          // mdk_dmr.hip, made by the first md_text_dmr_measure: likewise
    DeflateState *deflate = nullptr;                                  // mdk_deflate.hip, made by the first md_text_deflate_measure: likewise
};

// the block table for nb workgroups
MDK_HIDDEN int text_blocks_reserve(md_text *t, uint32_t nb);
// md_text_close: what mdk_parse.hip hung on the handle
MDK_HIDDEN void text_parse_free(md_text *t);
// ... and mdk_regions.hip
MDK_HIDDEN void text_regions_free(md_text *t);
// ... and mdk_unite.hip
MDK_HIDDEN void text_unite_free(md_text *t);
// ... and mdk_dmr.hip
MDK_HIDDEN void text_dmr_free(md_text *t);
// ... and mdk_deflate.hip
MDK_HIDDEN void text_deflate_free(md_text *t);

// one workgroup of TEXT_SCAN_WG threads: the exclusive scan of the nb workgroup totals as int64 offsets, and their sum into the status block
__device__ __forceinline__ void text_scan_blocks(const uint32_t *btot, int64_t *boff, TextStatus *st, uint32_t nb, int64_t *wtot) {
    int64_t carry = 0;
    for(uint32_t b0 = 0; b0 < nb; b0 += TEXT_SCAN_WG) {          // (uniform trip count: every thread takes part in every scan)
        const uint32_t b = b0 + threadIdx.x;
        const int64_t v = b < nb ? (int64_t)btot[b] : 0;
        int64_t total;
        const int64_t ex = block_excl_scan<TEXT_SCAN_WG>(v, wtot, total);
        if(b < nb) boff[b] = carry + ex;
        carry += total;
    }
    if(threadIdx.x == 0) st->total = carry;
}
#endif
