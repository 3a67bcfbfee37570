/* mdk_moments.h -- the rest of the C ABI of libmdk_stats.so, included by mdk_stats.h (include that): how alike the samples of a table are,
 * the pairwise sample moments of csrc/mdk_moments_core.h (csrc/mdk_moments.hip) and their centring.  The calls live on the md_stats handle
 * -- its stream, its status block, its error text (md_stats_last_error) -- and follow its rule: all calls of one handle come from one
 * thread at a time; a call returns when its work on the device is done. */
#ifndef MDK_MOMENTS_H
#define MDK_MOMENTS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct md_stats md_stats;

/* The pairwise sample moments of a table (csrc/mdk_moments.hip; the rule, in full, is csrc/mdk_moments_core.h's).
 * nmeth, nunmeth: two [n_samples, n] device matrices of int32 (elem_bytes 4) or int64 (8), sample-major, as md_stats_qdiff takes them; they
 * are read only.  A cell is covered if nmeth + nunmeth >= min_depth (1 to 2^26 - 1); its level is the methylated fraction in units of
 * 2^-16, rounded half up.  n_out, sx_out, sxx_out, sxy_out: four device [n_samples, n_samples] int64 matrices, zeroed and filled: over
 * the sites where samples i and j are both covered, their number, the sum of i's levels, of their squares, and of the products of i's
 * and j's.  Exact integers: the same on every run, device and blocking.
 * MD_STATS_ERR_ARG: n_samples outside 1..1024, n outside 0..2^30, elem_bytes not 4 or 8, a min_depth outside its range -- and, after the
 * launch, a negative entry or an entry of 2^26 or more, md_stats_qdiff's refusals in its words with the first (smallest) refused site in
 * the error text; a refused cell counts as uncovered and the call fails.  n == 0 gives zeros without a launch. */
int md_stats_moments(md_stats *h, const void *nmeth, const void *nunmeth, int elem_bytes, int32_t n_samples, int64_t n, int64_t min_depth,
                     int64_t *n_out, int64_t *sx_out, int64_t *sxx_out, int64_t *sxy_out);
/* The four sums centred: cxy[i][j] = n sxy - sx[i][j] sx[j][i] and vxx[i][j] = n sxx[i][j] - sx[i][j]^2, exact in 128-bit integers and
 * rounded once to a double, to nearest and ties to even.  The inputs are device [n_samples, n_samples] int64 matrices -- md_stats_moments'
 * outputs, or cell-by-cell sums of several calls' over disjoint sites --, the outputs device matrices of doubles of the same shape.
 * MD_STATS_ERR_ARG: n_samples outside 1..1024 -- and, after the launch, naming the first such cell (row-major): a negative sum, n above
 * 2^30, sx above n * 65536, sxx or sxy above n * 2^32, what the 128-bit bounds rest on.  A refused cell's outputs are 0.0. */
int md_stats_center(md_stats *h, const int64_t *n_in, const int64_t *sx_in, const int64_t *sxx_in, const int64_t *sxy_in, int32_t n_samples,
                    double *cxy_out, double *vxx_out);
/* A test hook: how md_stats_moments cuts its work on this handle from now on; 0 is the default of each.  shape 1: a lane per site, the
 * pairs in registers (the default up to 8 samples); 2: sites and sample bands staged in LDS, a lane per tile of pairs.  chunk_sites: the
 * sites staged at a time, and the least sites of a workgroup's range (a multiple of 64 up to 256; up to 64 at pair_tile 4 or 0, 192 at
 * 2: what the LDS holds).  pair_tile: 1, 2 or 4, a lane's pairs a side.  max_workgroups: the most workgroups of the launch.  The
 * results never depend on it.  MD_STATS_ERR_ARG: a value outside these. */
int md_stats_moments_limits(md_stats *h, int32_t shape, int32_t chunk_sites, int32_t pair_tile, int32_t max_workgroups);

#ifdef __cplusplus
}
#endif
#endif
