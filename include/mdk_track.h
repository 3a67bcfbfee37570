/* mdk_track.h -- the C ABI of libmdk_track.so: a table of calls as a bigWig track, made on the device by the rule of
 * csrc/mdk_bigwig_core.h (csrc/mdk_bigwig.hip; the sections' compression is the rule of csrc/mdk_deflate_core.h).  A library of its own,
 * as libmdk_index.so and libmdk_stats.so are: one code object, its own stream, its own pinned status block and its own error text, and no
 * link dependency on libmdk_hip.so or libmdk_extract.so.
 *
 * All calls of one handle come from one thread at a time; a call returns when its work on the device is done. */
#ifndef MDK_TRACK_H
#define MDK_TRACK_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct md_track md_track;

enum { MD_TRACK_OK = 0, MD_TRACK_ERR_ARG = -3, MD_TRACK_ERR_HIP = -2, MD_TRACK_ERR_NOMEM = -4 };          /* mdk_index.h's codes */
enum { MD_TRACK_PERCENT = 0, MD_TRACK_COVERAGE = 1 };                                                     /* BW_VALUE_* of the rule */

int md_track_open(int device, md_track **out);
void md_track_close(md_track *h);
const char *md_track_last_error(void);
/* A test hook: at most max_workgroups workgroups per launch (every kernel walks its work with a grid-stride loop) and batch_sections
 * sections compressed per batch; 0 is the default of either (what the device's compute units suggest; 4096). */
int md_track_limits(md_track *h, int max_workgroups, int batch_sections);
/* The whole of the device work.  contig, start, end, nmeth, nunmeth: five DEVICE int32 arrays of n rows (0 <= n <= 2^30).  names and
 * lengths: HOST arrays of n_contigs entries, the list the contig column indexes (a length is 0 .. 2^31 - 1; level 0 of all contigs
 * together may have at most 2^30 bins).  value: MD_TRACK_PERCENT or MD_TRACK_COVERAGE.  *bytes: the size of the file.
 * The rows are checked first (k_bw_check); a table the rule refuses is MD_TRACK_ERR_ARG with the text "row R: why" -- the row with the
 * smallest number, mdk_bigwig_core.h's bw_error_text -- and nothing else is launched.  n == 0 is the file without sections and makes
 * no launch.  After a successful call the file stays measured on the handle until the next measure. */
int md_track_bigwig_measure(md_track *h, const int32_t *contig, const int32_t *start, const int32_t *end, const int32_t *nmeth, const int32_t *nunmeth,
                            int64_t n, int32_t n_contigs, const char *const *names, const int64_t *lengths, int value, int64_t *bytes);
/* Bytes [offset, offset + bytes) of the measured file into the device buffer d_out (bytes long).  The range may begin and end anywhere:
 * inside the header, a tree or a section; it must lie inside the file.  Any number of calls, in any order, after one measure. */
int md_track_bigwig_fill_range(md_track *h, void *d_out, int64_t offset, int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif
