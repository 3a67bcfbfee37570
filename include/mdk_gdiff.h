/* mdk_gdiff.h -- more of the C ABI of libmdk_stats.so, included by mdk_stats.h (include that): three or more groups of REPLICATE samples
 * compared site by site on the device, the quasi-binomial F test of csrc/mdk_gdiff_core.h (csrc/mdk_gdiff.hip).  The call lives on the
 * md_stats handle -- its stream, its status block, its error text (md_stats_last_error) -- and follows its rule: all calls of one handle
 * come from one thread at a time; a call returns when its work on the device is done. */
#ifndef MDK_GDIFF_H
#define MDK_GDIFF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct md_stats md_stats;

/* nmeth, nunmeth: two [n_samples, n] device matrices of int32 (elem_bytes 4) or int64 (8), sample-major, as md_stats_qdiff takes them; they
 * are read only.  order, group_end: HOST arrays the call copies to buffers on the handle -- order the sample indices in the rule's
 * visiting order, group 0's members ascending, then group 1's, ..., each within the matrices and named once; group_end the n_groups
 * cumulative ends of the groups in it, ascending, no group empty.  Samples that order does not name are not read.
 * min_dispersion: the floor of the dispersion, within [2^-55, 2^800].
 * The outputs are device arrays: nmeth_g, nunmeth_g [n_groups, n], group-major, the groups' pooled counts; of n entries each meth_diff
 * (the most methylated covered group's fraction less the least methylated one's, in percent: never negative), group_lo, group_hi (these
 * two groups; -1 where no group is covered), and the test's pvalue, df (the covered samples less the covered groups), df_groups (the
 * covered groups less one), dispersion and statistic; steps (may be NULL) the terms added to the tail's series, for measurements and
 * tests.  A site whose covered groups are two has md_stats_qdiff's pvalue, df, dispersion and statistic of them, bit for bit.
 * MD_STATS_ERR_ARG: n_samples outside 1..1024, n outside 0..2^30, elem_bytes not 4 or 8, n_groups outside 2..n_samples, a group without
 * a sample, group_end not ascending, an index outside the matrices or named twice, a min_dispersion outside its range -- and, after the
 * launch, a negative entry, an entry of 2^26 or more or a pooled margin (a group's depth, the methylated or the unmethylated of all
 * groups) of 2^26 or more, md_stats_qdiff's refusals in its words with the first (smallest) refused site in the error text.  A refused
 * site is not tested: its outputs are those of a site without anything to test -- counts 0, meth_diff 0.0, group_lo and group_hi -1,
 * pvalue 1.0, df and df_groups 0, dispersion 1.0, statistic 0.0, steps 0 -- and the call fails.  n == 0 succeeds without a launch. */
int md_stats_gdiff(md_stats *h, const void *nmeth, const void *nunmeth, int elem_bytes, int32_t n_samples, int64_t n,
                   const int32_t *order, const int32_t *group_end, int32_t n_groups, double min_dispersion,
                   int64_t *nmeth_g, int64_t *nunmeth_g, double *meth_diff, int32_t *group_lo, int32_t *group_hi,
                   double *pvalue, int32_t *df, int32_t *df_groups, double *dispersion, double *statistic, uint32_t *steps);

#ifdef __cplusplus
}
#endif
#endif
