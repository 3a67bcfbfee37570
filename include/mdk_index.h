/* mdk_index.h -- the C ABI of libmdk_index.so: tabix indexes (.tbi) of BGZF tables, the per-line work done on the device
 * (csrc/mdk_tabix.hip; the rule is csrc/mdk_tabix_core.h).  A library of its own: one code object, its own stream and its own error text,
 * and no link dependency on libmdk_hip.so or libmdk_extract.so.
 *
 * The decompressed text is fed piece by piece, in file order: every piece is device memory of whole lines (only the file's last piece may
 * end without a newline), 16-byte aligned, at most 2^31 - 1 bytes.  The library keeps the running offset and line number.  All calls of
 * one handle come from one thread at a time; a call returns when its work on the device is done. */
#ifndef MDK_INDEX_H
#define MDK_INDEX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct md_index md_index;
typedef struct { int32_t format, col_seq, col_beg, col_end, meta, skip; } md_index_conf;      /* the six fields of a .tbi header */
typedef struct { uint64_t c_off, u_off; uint32_t isize, pad; } md_index_member;               /* a member that holds bytes: file offset, decompressed start, size */

enum { MD_INDEX_OK = 0, MD_INDEX_REFUSED = 1, MD_INDEX_ERR_ARG = -3, MD_INDEX_ERR_HIP = -2, MD_INDEX_ERR_NOMEM = -4 };

int md_index_open(int device, const md_index_conf *conf, md_index **out);
/* one piece of the text.  MD_INDEX_REFUSED: the rule refuses a line (md_index_refusal, md_index_last_error); the handle takes no more */
int md_index_feed(md_index *h, const void *d_text, int64_t bytes);
/* the 1-based line and the TBX_E_* code of the refusal, after MD_INDEX_REFUSED */
int md_index_refusal(const md_index *h, int64_t *line, int *code);
/* the end of the text: the members of the data file that hold bytes, in file order, and the file offset behind the last of them.
 * Gives the payload's size; the payload (not yet BGZF) is then copied to host memory by md_index_payload */
int md_index_finish(md_index *h, const md_index_member *members, int64_t n_members, uint64_t c_end, int64_t *payload_bytes);
int md_index_payload(md_index *h, void *dst, int64_t bytes);
/* counters for measurements: 0 lines, 1 entries, 2 records, 3 names, 4 pieces */
int64_t md_index_count(const md_index *h, int which);
void md_index_close(md_index *h);
const char *md_index_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
