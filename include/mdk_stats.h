/* mdk_stats.h -- the C ABI of libmdk_stats.so: two groups of REPLICATE samples compared site by site on the device, the quasi-binomial F
 * test of csrc/mdk_qdiff_core.h (csrc/mdk_qdiff.hip; entries, limits and refusals are csrc/mdk_diff_core.h's) -- and how alike the samples
 * of a table are, the pairwise sample moments of csrc/mdk_moments_core.h (csrc/mdk_moments.hip, the same source).  A library of its own, as
 * libmdk_index.so is: one code object, its own stream, its own pinned status block and its own error text, and no link dependency on
 * libmdk_hip.so or libmdk_extract.so.
 *
 * All calls of one handle come from one thread at a time; a call returns when its work on the device is done. */
#ifndef MDK_STATS_H
#define MDK_STATS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct md_stats md_stats;

enum { MD_STATS_OK = 0, MD_STATS_ERR_ARG = -3, MD_STATS_ERR_HIP = -2, MD_STATS_ERR_NOMEM = -4 };          /* mdk_index.h's codes */

int md_stats_open(int device, md_stats **out);
/* nmeth, nunmeth: two [n_samples, n] device matrices of int32 (elem_bytes 4) or int64 (8), sample-major, as md_text_diff takes them.
 * order: a HOST array of n_a + n_b sample indices in the rule's visiting order -- group A's members ascending, then group B's --, at most
 * 1024, each within the matrices and named once; the call copies it to a buffer on the handle.  Samples it does not name are not read.
 * min_dispersion: the floor of the dispersion, within [2^-55, 2^800] (what the header's analysis covers).
 * The outputs are device arrays of n entries: the groups' pooled counts, meth_diff (mdk_diff_core.h's diff_meth), and the test's pvalue,
 * df, dispersion and statistic; steps (may be NULL) the terms added to the tail's series, for measurements and tests.
 * MD_STATS_ERR_ARG: n_samples outside 1..1024, n outside 0..2^30, elem_bytes not 4 or 8, a group without a sample, an index outside the
 * matrices or named twice, a min_dispersion outside its range -- and, after the launch, a negative entry, an entry of 2^26 or more or a
 * pooled margin of 2^26 or more, md_text_diff's refusals in its words with the first (smallest) refused site in the error text.  A refused
 * site is not tested: the rule has no result for it, so its outputs are those of a site without anything to test -- counts 0, meth_diff
 * 0.0, pvalue 1.0, df 0, dispersion 1.0, statistic 0.0, steps 0 -- and the call fails.  n == 0 succeeds without a launch. */
int md_stats_qdiff(md_stats *h, const void *nmeth, const void *nunmeth, int elem_bytes, int32_t n_samples, int64_t n,
                   const int32_t *order, int32_t n_a, int32_t n_b, double min_dispersion,
                   int64_t *nmeth_a, int64_t *nunmeth_a, int64_t *nmeth_b, int64_t *nunmeth_b, double *meth_diff,
                   double *pvalue, int32_t *df, double *dispersion, double *statistic, uint32_t *steps);

/* The pairwise sample moments, on the same handle: three more calls, declared and documented in a header of their own */
#include "mdk_moments.h"
/* The count profile -- depth and level histograms per sample and group --, on the same handle: two more calls, likewise */
#include "mdk_profile.h"
/* Three or more groups of replicate samples -- the F test with groups - 1 numerator degrees of freedom --, on the same handle: one more call, likewise */
#include "mdk_gdiff.h"
/* A design matrix -- the F test of some columns of a logistic regression given the others: covariates, pairs, slopes --, on the same handle: one more call, likewise */
#include "mdk_mdiff.h"
void md_stats_close(md_stats *h);
const char *md_stats_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
