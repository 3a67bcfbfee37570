/*
 * mdk_session.c -- the resident session of include/mdk_extract.h, as far as it is not one command's: the device handle that every run
 * of a session works on, and the object a run hands back (the rows' device set with the contig names of the BAM header).  The runs
 * themselves are extract_run (mdk_extract.c) and perread_run (mdk_cmd_perread.c).
 */
#include "mdk_plan.h"

int mdk_session_open(int device, mdk_session **out) {
    mdk_session *s;
    if(!out || device < 0) return MDK_ERR_ARG;
    *out = NULL;
    if(!(s = calloc(1, sizeof(*s)))) return -5;
    s->device = device;
    *out = s;
    return 0;
}
void mdk_session_close(mdk_session *s) { if(!s) return; if(s->dev) md_dev_close(s->dev); free(s); }

MDK_LOCAL void session_device(mdk_session *S, devopen_t *d) {
    d->device = S->device;
    if(S->dev && (S->cfg.n_slots != d->cfg.n_slots || S->cfg.n_streams != d->cfg.n_streams)) { md_dev_close(S->dev); S->dev = NULL; }
    if(S->dev) { d->rc = md_dev_reset(S->dev, &d->cfg); d->dev = S->dev; if(d->rc) { snprintf(d->err, sizeof(d->err), "%s", md_dev_last_error()); md_dev_close(S->dev); S->dev = d->dev = NULL; } }
    else devopen_main(d);
    S->dev = d->dev; S->cfg = d->cfg;
}

MDK_LOCAL int session_run(mdk_session *s, int argc, char *argv[], void **out, size_t size, session_run_fn run) {
    int rc;
    if(!s || !out || argc < 1 || !argv) return MDK_ERR_ARG;
    *out = NULL;
    rc = run(argc, argv, s, out);
    if(rc == 0 && !*out) { *out = calloc(1, size); if(!*out) return -5; }      /* (help / version: no run, no rows) */
    return rc;
}

MDK_LOCAL int session_result(int ret, int frc, const mdk_plan *p, size_t size, void *set, int64_t n, void **out) {
    mdk_result *r; const int nt = p->bam->n_targets; int i;
    if(!ret && frc) { fprintf(stderr, "[mdk] device error: %s\n", md_dev_last_error()); ret = MDK_RC_DEVICE; }
    if(ret) return ret;
    r = calloc(1, size);
    if(r) r->names = calloc((size_t)nt + 1, sizeof(char *));
    if(!r || !r->names) { free(r); return -5; }
    r->set = set; r->n = n; r->n_contigs = nt;
    r->merged = p->o.merge ? 1 : 0; r->contexts = (p->o.ctx_on[0] ? 1 : 0) | (p->o.ctx_on[1] ? 2 : 0) | (p->o.ctx_on[2] ? 4 : 0);
    for(i = 0; i < nt; i++) r->names[i] = strdup(p->bam->target_name[i]);
    *out = r;
    return 0;
}
MDK_LOCAL void session_result_free(mdk_result *r) {
    int i;
    for(i = 0; i < r->n_contigs; i++) free(r->names[i]);
    free(r->names); free(r);
}
MDK_LOCAL int result_n_contigs(const mdk_result *r) { return r ? r->n_contigs : -1; }
MDK_LOCAL const char *result_contig_name(const mdk_result *r, int i) { return (r && i >= 0 && i < r->n_contigs) ? r->names[i] : NULL; }
