/* mdk_mdiff.h -- more of the C ABI of libmdk_stats.so, included by mdk_stats.h (include that): a site's counts regressed on a DESIGN MATRIX
 * on the device, the quasi-binomial F test of the design's tested columns given the others of csrc/mdk_mdiff_core.h (csrc/mdk_mdiff.hip) --
 * covariates, paired designs, the slope of a continuous variable.  The call lives on the md_stats handle -- its stream, its status block,
 * its error text (md_stats_last_error) -- and follows its rule: all calls of one handle come from one thread at a time; a call returns
 * when its work on the device is done. */
#ifndef MDK_MDIFF_H
#define MDK_MDIFF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct md_stats md_stats;

enum { MD_STATS_MDIFF_RANK = 1, MD_STATS_MDIFF_NUMERIC = 2, MD_STATS_MDIFF_REDUCED = 4, MD_STATS_MDIFF_FULL = 8 };          /* the bits of `flags` */

/* nmeth, nunmeth: two [n_samples, n] device matrices of int32 (elem_bytes 4) or int64 (8), sample-major, as md_stats_qdiff takes them; they
 * are read only.  order, design: HOST arrays the call copies to buffers on the handle -- order the n_used sample indices in the rule's
 * visiting order, ascending, each within the matrices and named once; design [n_used, p], row-major, row j the design row of sample
 * order[j]: the p - q REDUCED columns first, then the q TESTED ones, 1 <= q < p <= 8, every entry finite and at most 2^20 in magnitude,
 * the columns independent over the n_used rows.  Samples that order does not name are not read.
 * min_dispersion: the floor of the dispersion, within [2^-55, 2^800].
 * The outputs are device arrays: coef [p, n], column-major by design column, the fitted coefficients of the full model on the logit
 * scale; of n entries each nmeth_all and nunmeth_all (the used samples' counts added), pvalue, df (the covered samples less p),
 * dispersion, statistic, flags (uint8: the bits above -- the site's covered samples leave the design without its full rank: nothing to
 * test, df 0; a pivot of a fit was lost: nothing reported; the reduced or the full fit did not converge within 40 passes: reported all
 * the same) and iterations (the passes of both fits); steps (may be NULL) the terms added to the tail's series, for measurements and tests.
 * MD_STATS_ERR_ARG: n_samples outside 1..1024, n outside 0..2^30, elem_bytes not 4 or 8, p outside 2..8, q outside 1..p - 1, n_used
 * outside 1..n_samples, an index outside the matrices or named twice, a design entry that is not finite or above 2^20 in magnitude,
 * columns that are dependent over the used samples, a min_dispersion outside its range -- and, after the launch, a negative entry, an
 * entry of 2^26 or more or a pooled margin (the methylated or the unmethylated of all used samples) of 2^26 or more, md_stats_qdiff's
 * refusals in its words with the first (smallest) refused site in the error text.  A refused site is not tested: its outputs are those of
 * a site without anything to test -- counts 0, coefficients 0.0, pvalue 1.0, df 0, dispersion 1.0, statistic 0.0, flags, iterations and
 * steps 0 -- and the call fails.  n == 0 succeeds without a launch. */
int md_stats_mdiff(md_stats *h, const void *nmeth, const void *nunmeth, int elem_bytes, int32_t n_samples, int64_t n,
                   const int32_t *order, int32_t n_used, const double *design, int32_t p, int32_t q, double min_dispersion,
                   double *coef, int64_t *nmeth_all, int64_t *nunmeth_all, double *pvalue, int32_t *df, double *dispersion, double *statistic,
                   uint8_t *flags, int32_t *iterations, uint32_t *steps);

#ifdef __cplusplus
}
#endif
#endif
