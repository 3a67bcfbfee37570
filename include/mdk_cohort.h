/* mdk_cohort.h -- libmdk_cohort.so (csrc/mdk_cohort.hip): a united table (n sites, S samples, counts [S, n]) written as text and read
 * back on the device, and every sample's sums over intervals (csrc/mdk_cregion.hip).  The formats and the refusals are csrc/mdk_cohort_core.h's.  A library of its own: it links none of the others.
 * Every pointer but the names, `out` results and error text is DEVICE memory; every call is synchronous; a handle's calls come from one
 * thread at a time.  Return 0, or MD_COHORT_ERR_*; md_cohort_last_error() says more. */
#ifndef MDK_COHORT_H
#define MDK_COHORT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { MD_COHORT_ERR_HIP = -1, MD_COHORT_ERR_NOMEM = -2, MD_COHORT_ERR_ARG = -3 };
enum { MD_COHORT_FMT_COHORT = 0, MD_COHORT_FMT_METHYLBASE = 1 };

typedef struct md_cohort md_cohort;
/* the six site columns of a table: int32 contig, start, end; uint8 context; int8 strand; int32 nsamples */
typedef struct { const void *contig, *start, *end, *context, *strand, *nsamples; } md_cohort_sites;

const char *md_cohort_last_error(void);
int md_cohort_open(int device, md_cohort **out);
void md_cohort_close(md_cohort *h);
/* a test hook: the sites of a tile (a multiple of 64 up to 256), the samples of a block (1 to 64) and the most workgroups of a launch;
 * 0: the default of each.  No result depends on them. */
int md_cohort_limits(md_cohort *h, int32_t tile_sites, int32_t sample_block, int32_t max_workgroups);
/* the contig names (HOST memory): name c = names[name_off[c] .. name_off[c + 1]), 1 to 255 bytes each */
int md_cohort_names(md_cohort *h, const uint8_t *names, const uint32_t *name_off, int32_t n_contigs);

/* write: measure every line of the table (k_ctext_len, a scan), cut it into blocks of whole rows, fill a block's text (k_ctext_fill).
 * The table's tensors stay as they are until the last fill.  A refused table is MD_COHORT_ERR_ARG with the first site in the text. */
int md_cohort_measure(md_cohort *h, int fmt, const md_cohort_sites *sites, const int32_t *nmeth, const int32_t *nunmeth, int32_t n_samples, int64_t n, int64_t *total_bytes);
/* the longest run of whole rows from row0 whose text fits max_bytes, at least one row */
int md_cohort_cut(md_cohort *h, int64_t row0, int64_t max_bytes, int64_t *row1, int64_t *bytes);
int md_cohort_fill(md_cohort *h, int64_t row0, int64_t row1, void *out, int64_t bytes);

/* read: the lines of text[begin .. bytes) (text 16-byte aligned; the bytes before `begin` are the file's two header lines or nothing)
 * counted (k_cparse_len), then parsed into the columns of `rows` rows (k_cparse_fill): nmeth and nunmeth are [S, stride] with the rows at
 * [row_at, row_at + rows).  has_prev: the row before the first is (prev_contig, prev_start) and the first must ascend behind it.  A refused
 * line is MD_COHORT_ERR_ARG; md_cohort_parse_error_offset gives the offset of its first byte in `text`, or -1. */
int md_cohort_parse_measure(md_cohort *h, const void *text, int64_t bytes, int64_t begin, int32_t n_samples, int64_t *rows);
int md_cohort_parse_fill(md_cohort *h, const md_cohort_sites *sites, int32_t *nmeth, int32_t *nunmeth, int64_t stride, int64_t row_at, int64_t rows,
                         int has_prev, int32_t prev_contig, int32_t prev_start);
int64_t md_cohort_parse_error_offset(md_cohort *h);

/* sums over intervals (csrc/mdk_cregion.hip; the rule is csrc/mdk_region_core.h's, applied to every sample): the table's four site
 * columns the rule reads (int32 contig and start, uint8 context, int8 strand; rows strictly ascending in (contig, start)), nmeth and
 * nunmeth [n_samples, n] contiguous, k half-open intervals in any order, and the filter -- bit t of context_mask for context t; bit 0,
 * 1, 2 of strand_mask for strand +1, -1, 0; a cell counts with nmeth + nunmeth >= min_depth.  The results are [n_samples, k]
 * contiguous: cell (s, j) holds what md_text_regions gives for sample s and interval j.  The contig count is md_cohort_names'.  A row
 * that does not ascend, a row's contig outside the names or context above 2, an interval's contig outside the names, start < 0 or end <
 * start are MD_COHORT_ERR_ARG; the results are then undefined.  It leaves a measure that waits for its fill as it is. */
int md_cohort_regions(md_cohort *h, const void *contig, const void *start, const void *context, const void *strand,
                      const int32_t *nmeth, const int32_t *nunmeth, int32_t n_samples, int64_t n,
                      const int32_t *iv_contig, const int32_t *iv_start, const int32_t *iv_end, int64_t k,
                      uint32_t context_mask, uint32_t strand_mask, int32_t min_depth,
                      int32_t *nsites, int64_t *out_nmeth, int64_t *out_nunmeth);
#ifdef __cplusplus
}
#endif
#endif
