/* mdk_profile.h -- more of the C ABI of libmdk_stats.so, included by mdk_stats.h (include that): the count profile of a table, the depth
 * and level histograms per sample and group of csrc/mdk_profile_core.h (csrc/mdk_profile.hip).  The calls live on the md_stats handle --
 * its stream, its status block, its error text (md_stats_last_error) -- and follow its rule: all calls of one handle come from one
 * thread at a time; a call returns when its work on the device is done. */
#ifndef MDK_PROFILE_H
#define MDK_PROFILE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct md_stats md_stats;

/* The count profile of a table (csrc/mdk_profile.hip; the rule, in full, is csrc/mdk_profile_core.h's).
 * nmeth, nunmeth: two [n_samples, n] device matrices of int32 (elem_bytes 4) or int64 (8), sample-major, as md_stats_qdiff takes them; they
 * are read only.  group: n device bytes, the group of each site, every one below n_groups (1 to 4) -- or NULL: every site is in group 0.
 * With d = nmeth + nunmeth of a cell and g its site's group, the outputs, device int64 arrays that are zeroed and filled:
 *   depth_hist   [n_samples, n_groups, depth_bins + 1]: the cells of depth exactly b in bin b < depth_bins, of depth_bins or more in the
 *                last; every cell counts, d = 0 included (depth_bins 1 to 4096)
 *   level_hist   [n_samples, n_groups, level_bins]: the covered cells, d >= min_depth (1 to 2^26 - 1), by
 *                min(level_bins - 1, floor(nmeth * level_bins / d)) (level_bins 1 to 256)
 *   nmeth_sum, nunmeth_sum   [n_samples, n_groups]: the sums of the covered cells
 *   max_depth    [n_samples, n_groups]: the largest d of any cell, 0 where there is none
 * Exact integers: the same on every run, device and blocking.
 * MD_STATS_ERR_ARG: n_samples outside 1..1024, n outside 0..2^30, elem_bytes not 4 or 8, n_groups, depth_bins, level_bins or min_depth
 * outside their ranges -- and, after the launch, a negative entry, an entry of 2^26 or more (md_stats_qdiff's refusals in its words) or a
 * group of n_groups or more, with the first (smallest) refused site in the error text; a refused cell is counted nowhere and the call
 * fails.  n == 0 gives zeros without a launch. */
int md_stats_profile(md_stats *h, const void *nmeth, const void *nunmeth, int elem_bytes, int32_t n_samples, int64_t n,
                     const uint8_t *group, int32_t n_groups, int64_t min_depth, int32_t depth_bins, int32_t level_bins,
                     int64_t *depth_hist, int64_t *level_hist, int64_t *nmeth_sum, int64_t *nunmeth_sum, int64_t *max_depth);
/* A test hook: how the profile cuts its work on this handle from now on; 0 is the default of each.  range_sites: the sites of a
 * workgroup's range (a multiple of 64; by default the table's sites dealt over the launch, 8192 at least).  band_samples: the samples
 * whose histograms a workgroup keeps in LDS at a time, 1 (the default), 2 or 4; a band that holds no sample more for being wider, or
 * that the LDS cannot hold at a call's bins, is halved.  max_workgroups: the most workgroups of the launch.  The results never depend on
 * it.  MD_STATS_ERR_ARG: a value outside these. */
int md_stats_profile_limits(md_stats *h, int32_t range_sites, int32_t band_samples, int32_t max_workgroups);

#ifdef __cplusplus
}
#endif
#endif
