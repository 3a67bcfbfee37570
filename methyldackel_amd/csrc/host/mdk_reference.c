/* mdk_reference.c -- the FASTA reader of the commands (mdk_fasta.c) behind a handle, for callers outside this library: Python's Reference
 * uploads the bases to a renderer (include/mdk_hip.h md_text_reference) so that bedGraph files can be read back on the device. */
#include <stdlib.h>
#include "mdk_extract.h"
#include "mdk_io.h"

struct mdk_reference { mdk_fasta fa; };

int mdk_reference_load(const char *fasta, mdk_reference **out) {
    mdk_reference *r;
    if(!out) return -1;
    *out = NULL;
    if(!fasta || (r = calloc(1, sizeof(*r))) == NULL) return -1;
    if(mdk_fasta_load(fasta, &r->fa) != 0) { free(r); return -1; }
    *out = r;
    return 0;
}
int mdk_reference_n_contigs(const mdk_reference *r) { return r ? r->fa.n : -1; }
const char *mdk_reference_name(const mdk_reference *r, int i) { return r && i >= 0 && i < r->fa.n ? r->fa.name[i] : NULL; }
int64_t mdk_reference_length(const mdk_reference *r, int i) { return r && i >= 0 && i < r->fa.n ? r->fa.len[i] : -1; }
const char *mdk_reference_bases(const mdk_reference *r, int i) { return r && i >= 0 && i < r->fa.n ? r->fa.seq[i] : NULL; }
void mdk_reference_free(mdk_reference *r) { if(r) { mdk_fasta_free(&r->fa); free(r); } }
