/* mdk_smooth.h -- the C ABI of libmdk_smooth.so: kernel-weighted methylation levels of every site of a table, per sample, made on the
 * device by the rule of csrc/mdk_smooth_core.h (csrc/mdk_smooth.hip).  A library of its own, as libmdk_stats.so is: one code object, its
 * own stream, its own pinned status block and its own error text, and no link dependency on the other libraries.
 *
 * All calls of one handle come from one thread at a time; a call returns when its work on the device is done. */
#ifndef MDK_SMOOTH_H
#define MDK_SMOOTH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct md_smooth md_smooth;

enum { MD_SMOOTH_OK = 0, MD_SMOOTH_ERR_ARG = -3, MD_SMOOTH_ERR_HIP = -2, MD_SMOOTH_ERR_NOMEM = -4 };      /* mdk_stats.h's codes */

int md_smooth_open(int device, md_smooth **out);
/* contig, start: device arrays of n int32, strictly ascending in (contig, start).  nmeth, nunmeth: two [n_samples, n] device matrices of
 * int32 (elem_bytes 4) or int64 (8), sample-major, as md_stats_qdiff takes them.  half_bases within [0, 2^20], min_sites within
 * [1, 2^16], kernel 0 (tricube) or 1 (flat): a site's window reaches at least half_bases to either side and holds at least min_sites
 * sites of its contig (all of a shorter contig).
 * The outputs are device arrays: level and depth, [n_samples, n] doubles -- the weighted methylated sum over the weighted depth (the
 * quiet NaN 0x7ff8000000000000 where that depth is not above 0) and the weighted depth --, nsites and half, n int32 -- the window's rows
 * and its half-width in bases, the same for every sample.  Nothing else is written, and the inputs are only read; the handle keeps n
 * int32 of scratch from the largest call on.
 * MD_SMOOTH_ERR_ARG: n_samples outside 1..1024, n outside 0..2^30, elem_bytes not 4 or 8, a parameter outside its range -- and, after
 * the launches, a row not strictly ascending behind its predecessor, a negative contig or start, a negative entry, an entry of 2^26 or
 * more, with the first (smallest) refused site in the error text.  A refused call's outputs are unspecified.  n == 0 succeeds without a
 * launch. */
int md_smooth_run(md_smooth *h, const int32_t *contig, const int32_t *start, const void *nmeth, const void *nunmeth, int elem_bytes,
                  int32_t n_samples, int64_t n, int32_t half_bases, int32_t min_sites, int32_t kernel,
                  double *level, double *depth, int32_t *nsites, int32_t *half);
/* A test hook: the sites of a workgroup's tile (a multiple of 64, at most 256), the rows of a chunk staged in LDS (at least 64), the
 * samples of a batch (at most 8) and the most workgroups of a launch, from the next call on; 0 is the default of each.  A chunk and
 * a batch that do not fit 64 KiB of LDS together are MD_SMOOTH_ERR_ARG.  The results never depend on any of them. */
int md_smooth_limits(md_smooth *h, int32_t tile_sites, int32_t chunk_sites, int32_t sample_batch, int32_t max_workgroups);
void md_smooth_close(md_smooth *h);
const char *md_smooth_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
