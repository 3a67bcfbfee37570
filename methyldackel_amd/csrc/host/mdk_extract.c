/*
 * mdk_extract.c -- extract_main, the drop-in entry point of the MI355X `MethylDackel extract` path (extract.c:706 in the reference).
 *
 * Division of labour:
 *   host  : options and inputs (mdk_plan.c), reading the file and part of the BGZF inflate (mdk_io.c), the reference's chunk
 *           schedule (extract.c:325-350, common.c:466-493) applied to member digests and record tables (mdk_pipeline.c), and the
 *           text post-pass (extract.c:443-510, 39-99; mdk_emit.c).  Per record or per base the host does nothing, except for a
 *           chunk the device hands back (MDK_ERR_PREP_HOST) and under MDK_HOST_PREP=1.
 *   device: the rest of the BGZF inflate and the record framing (k_inflate, k_walk), read admission (filter_func, common.c:416-444),
 *           strand (getStrand, common.c:84-116), read-name pairing (overlaps.c:121-147), CIGAR expansion, trimming, overlap
 *           resolution, context classification, counting.
 * Three threads move the chunks here: this one uploads and launches them in groups, a second collects the results and hands them
 * to the emitter, a third uploads the contigs' references ahead of the chunks that need them.
 * There is no CPU implementation of the per-base work in this library.
 */
#include <fcntl.h>
#include <sys/prctl.h>
#include "mdk_plan.h"

/* ------------------------------------------------------------------------------------------------ */
/* the drop-in entry point                                                                           */
/* ------------------------------------------------------------------------------------------------ */
/* The `MethylDackel` command asks (MDK_FAST_EXIT) to leave with _exit once the outputs are closed, skipping the unpinning
 * of buffers and the HIP shutdown.  Not under a profiler or another injected tool: those finalise at normal exit. */
static double rss_mb(int shared) {      /* resident set (or its file-backed/shared part) in MB: host profile only */
    long vm = 0, rss = 0, shr = 0; FILE *sf = fopen("/proc/self/statm", "r");
    if(sf) { if(fscanf(sf, "%ld %ld %ld", &vm, &rss, &shr) != 3) rss = shr = 0; fclose(sf); }
    return (shared ? shr : rss) * 4096e-6;
}
/* formatting threads: 8 are ahead of a CpG-only run; the dense contexts print ~20x the lines */
static int emit_threads(const mdk_plan *p) { const int cap = (p->o.ctx_on[1] || p->o.ctx_on[2]) ? 24 : 8; return p->o.n_threads >= cap ? cap : p->o.n_threads; }
MDK_LOCAL int fast_exit_wanted(void) {
    const char *pre = getenv("LD_PRELOAD");
    if(!getenv("MDK_FAST_EXIT")) return 0;
    if(getenv("HSA_TOOLS_LIB") || getenv("ROCP_TOOL_LIBRARIES") || getenv("ROCPROFILER_REGISTER_FORCE_LOAD") || getenv("ROCPROF_OUTPUT_PATH")) return 0;
    if(pre && (strstr(pre, "rocprof") || strstr(pre, "roctx") || strstr(pre, "rocm"))) return 0;
    return 1;
}
/* leave now: outputs are flushed and closed; nobody needs to wait for staging buffers to be unpinned one by one and for the
 * runtime's exit handlers (the `MethylDackel` command only: main.c sets MDK_FAST_EXIT) */
MDK_LOCAL void leave_fast(int ret) {
    const char *fdv = getenv("MDK_DONE_FD");
    fflush(stdout); fflush(stderr);
    if(fdv) {     /* the command runs as the child of a process that only waits for this word (main.c detach_teardown): outputs are closed, it may return */
        const int fd = atoi(fdv), nul = open("/dev/null", O_RDWR);
        unsigned char code = (unsigned char)(ret & 0xff);
        if(nul >= 0) { dup2(nul, 0); dup2(nul, 1); dup2(nul, 2); if(nul > 2) close(nul); }
        (void)prctl(PR_SET_PDEATHSIG, 0);
        if(write(fd, &code, 1) != 1) { /* nobody is listening any more */ }
        close(fd);
    }
    mdk_cli_quiesce();
    _exit(ret & 0xff);
}
/* the HIP runtime takes 0.1-0.4 s to come up: start that before anything else (options, BAM header, FASTA), on its own thread */
static void *hipwarm_main(void *arg) { (void)arg; (void)md_dev_warm(getenv("MDK_DEVICE") ? atoi(getenv("MDK_DEVICE")) : 0); return NULL; }
/* only in the `MethylDackel` command, which always ends with _exit (leave_fast): a library caller whose bad command line makes
 * us return at once must not find a half-initialised runtime racing its exit handlers.  The thread is joined -- and with it the side
 * threads md_dev_warm starts (md_dev_quiesce) -- before the command leaves: mdk_cli_quiesce, called by leave_fast and by main.c after
 * the caller has been told that the outputs are closed. */
static pthread_t g_warm_th; static int g_warm_started = 0;
static mdk_plan *g_leaving = NULL;          /* the plan of a command on its way out: its reaper is waited for (mdk_io.h) */
MDK_LOCAL void hip_warm_up(void) {
    if(!fast_exit_wanted() || g_warm_started) return;
    if(pthread_create(&g_warm_th, NULL, hipwarm_main, NULL) == 0) g_warm_started = 1;
}
MDK_LOCAL void leave_fast_plan(mdk_plan *p, int ret) { g_leaving = p; leave_fast(ret); }      /* every command's way out: the plan's reaper and device teams are waited for */
void mdk_cli_quiesce(void) {
    if(g_leaving && g_leaving->bam) { mdk_bam_teams_leave(g_leaving->bam); mdk_bam_reap_wait(g_leaving->bam); }
    if(g_warm_started) { pthread_join(g_warm_th, NULL); g_warm_started = 0; }
    md_dev_quiesce();
}
/* md_dev_last_error is per thread: keep the text of a failed open for the thread that reports it */
MDK_LOCAL void *devopen_main(void *arg) { devopen_t *d = arg; d->rc = md_dev_open(d->device, &d->cfg, &d->dev); if(d->rc) snprintf(d->err, sizeof(d->err), "%s", md_dev_last_error()); return NULL; }

/* Chunks travel to the device in GROUPS of up to MDK_GROUP: a 1 Mb chunk alone is fewer than two workgroups per CU and pays every
 * launch boundary itself, so whatever the reader has ready when a group is opened (at least one chunk, at most eight) is uploaded
 * into the group's slots and prepared and piled up with one launch per kernel (md_dev_launch_group).  MDK_NGROUPS groups are in
 * flight, each on its own stream: while one computes, the next is uploaded by this thread and the one before is collected by the
 * collector thread (one wait and one round of copies per group, md_dev_download_group) and handed to the emitter in schedule
 * order.  The reference's unit of work is the chunk (extract.c:325-350); here it is the unit of scheduling and of output only. */
#define MDK_GROUP 8
#define MDK_NGROUPS_MAX 6
static int g_ngroups = 3;            /* groups in flight (MDK_GROUPS_IN_FLIGHT=n, 2..6) */
#define MDK_NGROUPS g_ngroups
enum { G_FREE = 0, G_FILL, G_LAUNCHED };
enum { SINK_TEXT = 0, SINK_CALLS, SINK_BIAS, SINK_CYTO };      /* where collected groups go: the text emitter (extract_main); the device calls of a session (md_dev_calls_group); the mbias
                                                     * histogram of a session -- nothing comes back per chunk, the collector reads the group's status blocks (md_dev_mbias_collect); the
                                                     * cytosine report of a session (md_dev_cytosines_group): every chunk that is not skipped has rows, with or without reads */
typedef struct { mdk_chunk ch[MDK_GROUP]; int slot[MDK_GROUP]; int n, launched[MDK_GROUP], inplace[MDK_GROUP], single[MDK_GROUP], state, held, n_held, rel_slot[MDK_GROUP]; mdk_chunk rel_ch[MDK_GROUP]; } cgroup;      /* held: the host memory behind its records has not been given back yet; inplace: the device reads the chunk's records where the piece they were inflated in holds them (md_dev_upload_raw_inplace): that piece goes back when the chunk's results are in */
typedef struct {
    mdk_plan *p; md_dev *dev; emitter *em; cgroup G[MDK_NGROUPS_MAX];
    int sink;                            /* SINK_* */
    pthread_mutex_t mu; pthread_cond_t cv;
    int ret, up_done;                    /* (mu) first error; the uploader has launched its last group */
    uint64_t n_up, n_col;                /* (mu) groups launched / collected: group k lives in G[k % MDK_NGROUPS] */
    int *ref_state; int ref_quit, ref_done; int32_t ref_t0, ref_t1;        /* (mu) per contig: 0 not uploaded yet, 1 resident, < 0 the error its upload met; ref_done: the thread has left */
    double w_down, w_emit; int n_host_prep;
} xpipe;
/* Once a group's records have crossed the link (a few ms: they were queued before its kernels), the staging memory they came from goes back to
 * the inflate teams -- not when the results are in.  block = 0: only if the copies are done already; 1: wait for them (the reader is out of
 * chunks, perhaps for want of that very memory).  Called by the uploader thread only. */
static void release_uploaded(xpipe *X, int block) {
    int k, i;
    if(getenv("MDK_NO_EARLY_RELEASE")) return;
    for(k = 0; k < MDK_NGROUPS; k++) {
        cgroup *g = &X->G[(X->n_up + (uint64_t)k) % MDK_NGROUPS]; int last = -1;      /* oldest first: the group about to be refilled, ..., the one launched last */
        if(!g->held) continue;
        for(i = 0; i < g->n_held; i++) if(g->rel_slot[i] >= 0) last = g->rel_slot[i];
        if(last >= 0) { const int done = block ? (md_dev_upload_wait(X->dev, last) == 0) : md_dev_upload_done(X->dev, last) == 1; if(!done) return; }      /* (in order: a later group's copies are queued behind) */
        for(i = 0; i < g->n_held; i++) if(g->rel_slot[i] >= 0) (void)mdk_plan_release_records(X->p, &g->rel_ch[i]);
        g->held = 0; block = 0;
    }
}
static md_cyto_chunk cyto_chunk(const mdk_chunk *c) { md_cyto_chunk q; q.key = c->index; q.tid = c->tid; q.beg = c->beg; q.end = c->end; return q; }
static void xp_fail(xpipe *X, int ret) { pthread_mutex_lock(&X->mu); if(!X->ret) X->ret = ret; pthread_cond_broadcast(&X->cv); pthread_mutex_unlock(&X->mu); }

/* the contigs' bases (and BED runs, mappability tracks) go to the device ahead of the chunks, in schedule order */
static void *refs_main(void *arg) {
    xpipe *X = arg; mdk_plan *p = X->p; int32_t t;
    for(t = X->ref_t0; t < X->ref_t1 && t < p->bam->n_targets; t++) {
        int rc = 1, q;
        pthread_mutex_lock(&X->mu); q = X->ref_quit || X->ret; pthread_mutex_unlock(&X->mu);
        if(q) break;
        if(p->fa_of_tid[t] >= 0) { rc = mdk_plan_ensure_reference(p, X->dev, t); rc = rc ? (rc < 0 ? rc : -1) : 1; }
        pthread_mutex_lock(&X->mu); X->ref_state[t] = rc; pthread_cond_broadcast(&X->cv); pthread_mutex_unlock(&X->mu);
    }
    pthread_mutex_lock(&X->mu); X->ref_done = 1; pthread_cond_broadcast(&X->cv); pthread_mutex_unlock(&X->mu);
    return NULL;
}
static int ref_wait(xpipe *X, int32_t tid) {
    int rc;
    pthread_mutex_lock(&X->mu);
    while(!X->ref_state[tid] && !X->ret && !X->ref_done) pthread_cond_wait(&X->cv, &X->mu);
    rc = X->ref_state[tid];
    pthread_mutex_unlock(&X->mu);
    if(!rc && !X->ret) { rc = mdk_plan_ensure_reference(X->p, X->dev, tid); return rc; }       /* a contig the thread did not have on its list (it has left: nobody else uploads) */
    return rc == 1 ? 0 : rc ? rc : -1;
}

/* MDK_WATCHDOG=1 (diagnostics): once a second, where every stage of the pipeline stands -- for a run that stalls.  MDK_WATCHDOG=<ms> with
 * ms >= 2: the same every <ms> milliseconds in short form, a time series of the queues between the stages (which one runs empty, which one full) */
static volatile int g_up_phase, g_col_phase;
static void *watchdog_main(void *arg) {
    xpipe *X = arg; mdk_plan *p = X->p; mdk_bam *b = p->bam; int k; const double t0 = now_s();
    const int ms = atoi(getenv("MDK_WATCHDOG")) >= 2 ? atoi(getenv("MDK_WATCHDOG")) : 1000;
    for(;;) {
        int q, st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if(ms >= 1000) { for(k = 0; k < 10; k++) { usleep(100000); pthread_mutex_lock(&X->mu); q = X->up_done && X->n_col == X->n_up; pthread_mutex_unlock(&X->mu); if(q) return NULL; } }
        else { usleep((useconds_t)ms * 1000); pthread_mutex_lock(&X->mu); q = X->up_done && X->n_col == X->n_up; pthread_mutex_unlock(&X->mu); if(q) return NULL; }
        for(k = 0; k < p->n_slot; k++) st[p->slot_state ? p->slot_state(p, k) & 7 : 0]++;
        if(ms < 1000) fprintf(stderr, "[wd] t=%.3f up=%d L=%" PRIu64 " C=%" PRIu64 " col=%d out=%u slots=%d/%d/%d/%d/%d/%d pieces=%" PRIu64 "/%" PRIu64 "/%d slabs=%d+%d/%d+%d\n",
                now_s() - t0, g_up_phase, X->n_up, X->n_col, g_col_phase, p->next_out, st[0], st[1], st[2], st[3], st[4], st[5], b->next_seq, b->pop_seq, b->n_ready, b->n_alloc, b->n_pool, b->n_dalloc, b->n_dpool);
        else
        fprintf(stderr, "[mdk watchdog] %.1fs: uploader phase %d groups launched %" PRIu64 " collected %" PRIu64 " collector phase %d | chunks handed out %u, slots free/fill/raw/work/done/held %d/%d/%d/%d/%d/%d | pieces handed %" PRIu64 " popped %" PRIu64 " ready %d, slabs host %d(+%d free) device %d(+%d free), io %d inf_done %d\n",
                now_s() - t0, g_up_phase, X->n_up, X->n_col, g_col_phase, p->next_out, st[0], st[1], st[2], st[3], st[4], st[5], b->next_seq, b->pop_seq, b->n_ready, b->n_alloc, b->n_pool, b->n_dalloc, b->n_dpool, b->io_status, b->inf_done);
    }
}

/* collects the launched groups in order: results to the emitter, the group back to the uploader */
static void *collector_main(void *arg) {
    xpipe *X = arg; mdk_plan *p = X->p; md_dev *dev = X->dev; int i;
    for(;;) {
        cgroup *g; int ls[MDK_GROUP], li[MDK_GROUP], nl = 0, rcs[MDK_GROUP], rc = 0, bad = 0; md_sites st[MDK_GROUP], sites[MDK_GROUP]; double ta;
        memset(st, 0, sizeof(st));
        pthread_mutex_lock(&X->mu);
        while(X->n_col == X->n_up && !X->up_done && !X->ret) pthread_cond_wait(&X->cv, &X->mu);
        if(X->ret || X->n_col == X->n_up) { pthread_mutex_unlock(&X->mu); break; }
        g = &X->G[X->n_col % MDK_NGROUPS];
        pthread_mutex_unlock(&X->mu);
        memset(sites, 0, sizeof(sites));
        for(i = 0; i < g->n; i++) if(g->launched[i] && !g->single[i]) { ls[nl] = g->slot[i]; li[nl] = i; nl++; }
        ta = now_s(); g_col_phase = 1;
        switch(X->sink) {
        case SINK_BIAS:      /* (a chunk the host prepared was counted by a launch of its own: its slot's stream is waited for) */
            for(i = 0; i < g->n && !rc; i++) if(g->launched[i] && g->single[i]) rc = md_dev_slot_sync(dev, g->slot[i]);
            if(nl && !rc) rc = md_dev_mbias_collect(dev, ls, nl, rcs);
            break;
        case SINK_CALLS:
            if(nl) { uint32_t keys[MDK_GROUP]; for(i = 0; i < nl; i++) keys[i] = g->ch[li[i]].index; rc = md_dev_calls_group(dev, ls, keys, nl, rcs); }
            break;
        case SINK_CYTO: {    /* the launched chunks first (rcs[i] belongs to li[i]), then any chunk of the schedule that was not skipped and not launched: its rows are all 0 0 */
            int cs[MDK_GROUP], crc[MDK_GROUP], nc = nl; md_cyto_chunk cq[MDK_GROUP];
            memset(crc, 0, sizeof(crc));
            for(i = 0; i < nl; i++) { cs[i] = ls[i]; cq[i] = cyto_chunk(&g->ch[li[i]]); }
            for(i = 0; i < g->n && !rc; i++) if(!g->launched[i] && !g->ch[i].skipped) { rc = ref_wait(X, g->ch[i].tid); cs[nc] = -1; cq[nc] = cyto_chunk(&g->ch[i]); nc++; }
            if(nc && !rc) rc = md_dev_cytosines_group(dev, cs, cq, nc, crc);
            for(i = 0; i < nl; i++) rcs[i] = crc[i];
            break; }
        default:
            if(nl) rc = md_dev_download_group(dev, ls, nl, st, rcs);
        }
        g_col_phase = 2;
        if(rc) { fprintf(stderr, "[mdk] device error: %s\n", md_dev_last_error()); xp_fail(X, MDK_RC_DEVICE); break; }
        for(i = 0; i < nl && !bad; i++) {
            const int k = li[i];
            rc = rcs[i];
            if(rc == MDK_ERR_PREP_HOST) {          /* a read name the device preparation does not handle: this chunk the slow way */
                static int told = 0;
                if(!told) { told = 1; fprintf(stderr, "[mdk] note: a chunk holds a read name with more records than the device preparation handles (secondary/supplementary-rich or amplicon-like data); such chunks are prepared on the host, which is slower\n"); }
                rc = mdk_plan_host_prepare_from(p, &g->ch[k], dev, g->slot[k]);
                if(!rc) rc = X->sink == SINK_BIAS ? md_dev_mbias_submit(dev, g->slot[k], &g->ch[k].batch) : md_dev_submit(dev, g->slot[k], &g->ch[k].batch);
                if(!rc && X->sink == SINK_BIAS) rc = md_dev_slot_sync(dev, g->slot[k]);
                else if(!rc && X->sink == SINK_CALLS) { int rc1 = 0; rc = md_dev_calls_group(dev, &g->slot[k], &g->ch[k].index, 1, &rc1); if(!rc) rc = rc1; }
                else if(!rc && X->sink == SINK_CYTO) { int rc1 = 0; const md_cyto_chunk q = cyto_chunk(&g->ch[k]); rc = md_dev_cytosines_group(dev, &g->slot[k], &q, 1, &rc1); if(!rc) rc = rc1; }
                else if(!rc) rc = md_dev_download(dev, g->slot[k], &st[i]);
                X->n_host_prep++;
            }
            if(rc == MDK_ERR_STRAND0) { fprintf(stderr, "Can't determine the strand of a read!\n"); abort(); }
            if(rc) { fprintf(stderr, "[mdk] device error: %s\n", md_dev_last_error()); xp_fail(X, MDK_RC_DEVICE); bad = 1; break; }
            sites[k] = st[i];
            if(g->inplace[k] && !getenv("MDK_NO_EARLY_RELEASE")) (void)mdk_plan_release_records(p, &g->ch[k]);      /* the kernels that read the piece are done: it goes back to the inflate teams */
        }
        X->w_down += now_s() - ta;
        if(bad) break;
        if(X->sink != SINK_TEXT) { g_col_phase = 0; pthread_mutex_lock(&X->mu); g->n = 0; g->state = G_FREE; X->n_col++; pthread_cond_broadcast(&X->cv); pthread_mutex_unlock(&X->mu); continue; }      /* the rows stay on the device */
        ta = now_s();
        g_col_phase = 3;
        for(i = 0; i < g->n; i++) if(emitter_push_lazy(X->em, &g->ch[i], &sites[i])) { xp_fail(X, X->em->failed ? MDK_RC_OUTPUT : MDK_RC_DEVICE); bad = 1; break; }
        emitter_wait_copied(X->em);                  /* (the emitter threads copy the group's site arrays side by side; the slots' buffers are the device's again from here) */
        X->w_emit += now_s() - ta;
        if(bad) break;
        g_col_phase = 0;
        pthread_mutex_lock(&X->mu); g->n = 0; g->state = G_FREE; X->n_col++; pthread_cond_broadcast(&X->cv); pthread_mutex_unlock(&X->mu);
    }
    return NULL;
}

/* the slabs the host teams filled while the runtime was still starting: registered with it now, next to the uploader instead of by it */
static void *prereg_main(void *arg) { md_dev *dev = arg; (void)md_host_register_all(dev, 1); return NULL; }

/* opening the device on its own thread, from the moment the options are known: the inputs (BAM header, index, FASTA) are opened meanwhile */
typedef struct { devopen_t d; pthread_t th; int started; } xopen;
static void xopen_start(mdk_plan *p, void *arg) {
    xopen *o = arg;
    if(getenv("MDK_GROUPS_IN_FLIGHT")) { g_ngroups = atoi(getenv("MDK_GROUPS_IN_FLIGHT")); if(g_ngroups < 2) g_ngroups = 2; if(g_ngroups > MDK_NGROUPS_MAX) g_ngroups = MDK_NGROUPS_MAX; }
    mdk_plan_dev_cfg(p, &o->d.cfg);
    o->d.cfg.n_slots = MDK_NGROUPS * MDK_GROUP; o->d.cfg.n_streams = MDK_NGROUPS;
    if(getenv("MDK_DEVICE")) o->d.device = atoi(getenv("MDK_DEVICE"));
    o->started = pthread_create(&o->th, NULL, devopen_main, &o->d) == 0;
}

/* ---- a resident session (include/mdk_extract.h, mdk_session.c): the same pipeline, one device handle across runs, calls kept on the device ---- */
/* the session's after_options: options that only shape text or files are refused; the device configuration is worked out as for the command */
static void session_options(mdk_plan *p, void *arg) {
    xopen *o = arg; const opts_t *q = &p->o;
    p->no_text = 1;
    if(q->fraction || q->counts || q->logit || q->methylkit || q->cytosine_report) {
        fprintf(stderr, "[mdk] --fraction, --counts, --logit, --methylKit and --cytosine_report only shape text output: a session returns the calls themselves\n");
        p->open_rc = MDK_RC_UNSUPPORTED; return;
    }
    mdk_plan_dev_cfg(p, &o->d.cfg);
    session_geometry(&o->d.cfg);
}
/* the same for mdk_session_cytosines: --cytosine_report is what the run is (implied, accepted if given), the formats that are arithmetic on
 * columns are refused as above, and --mergeContext ends as it ends the command.  The device is configured as the command configures it */
static void session_options_cyto(mdk_plan *p, void *arg) {
    xopen *o = arg; opts_t *q = &p->o;
    p->no_text = 1;
    if(q->fraction || q->counts || q->logit || q->methylkit) {
        fprintf(stderr, "[mdk] --fraction, --counts, --logit and --methylKit only shape text output: a session returns the report's rows themselves\n");
        p->open_rc = MDK_RC_UNSUPPORTED; return;
    }
    if(q->merge) { fprintf(stderr, "--mergeContext and --cytosine_report are mutually exclusive.\n"); plan_usage(); p->open_rc = 1; return; }
    q->cytosine_report = 1;
    mdk_plan_dev_cfg(p, &o->d.cfg);
    session_geometry(&o->d.cfg);
}
MDK_LOCAL void session_geometry(md_dev_cfg *cfg) {
    if(getenv("MDK_GROUPS_IN_FLIGHT")) { g_ngroups = atoi(getenv("MDK_GROUPS_IN_FLIGHT")); if(g_ngroups < 2) g_ngroups = 2; if(g_ngroups > MDK_NGROUPS_MAX) g_ngroups = MDK_NGROUPS_MAX; }
    else g_ngroups = 3;
    cfg->n_slots = MDK_NGROUPS * MDK_GROUP; cfg->n_streams = MDK_NGROUPS;
}

/* extract_main's pipeline; S != NULL: a session's run -- no output files, no emitter, every collected group compacted into calls on S's device
 * handle (opened at the first run, reset before every later one), handed over in *out.  mbias (a session's only): the command line is mbias_main's, the
 * groups are launched with md_dev_mbias_group and leave nothing but their status blocks, and the run ends with the histogram's table (md_dev_bias_finish).
 * RUN_CYTO (a session's only): the extract command line with --cytosine_report implied; the collected groups become the report's rows (md_dev_cytosines_group) */
enum { RUN_EXTRACT = 0, RUN_MBIAS, RUN_CYTO };
static int pipeline_run(int argc, char *argv[], mdk_session *S, void **out, int mode) {
    const int mbias = mode == RUN_MBIAS, cyto = mode == RUN_CYTO;
    mdk_plan *p = NULL; md_dev *dev = NULL; xpipe *X = NULL; int rc, ret = 0, more = 1, i, g_i; xopen dop; pthread_t cth, rth, preg; int cth_ok = 0, rth_ok = 0, preg_ok = 0; emitter em;
    double T0 = now_s(), t_open, t_dev, w_next = 0, w_sub = 0, w_group = 0, w_ref = 0, w_rel = 0, ta; uint64_t n_chunks = 0; int32_t ref_t0, ref_t1;
    if(getenv("MDK_HOST_PROFILE")) { struct timespec ts; clock_gettime(CLOCK_REALTIME, &ts); fprintf(stderr, "[mdk main] entered at epoch %.3f\n", ts.tv_sec + 1e-9 * ts.tv_nsec); }
    if(argc > 2 && !S) hip_warm_up();
    memset(&dop, 0, sizeof(dop)); memset(&em, 0, sizeof(em));
    if(mbias) { rc = mdk_plan_open_mbias(argc, argv, &p); if(!rc && p) { mdk_plan_dev_cfg(p, &dop.d.cfg); session_geometry(&dop.d.cfg); } }
    else rc = plan_open_ex(argc, argv, &p, S ? (cyto ? session_options_cyto : session_options) : xopen_start, &dop);
    t_open = now_s() - T0;
    if(rc != 0 || !p) { if(dop.started) { pthread_join(dop.th, NULL); if(dop.d.dev) md_dev_close(dop.d.dev); } return rc; }
    if(getenv("MDK_HOST_PROFILE")) fprintf(stderr, "[mdk main] resident after plan open %.0f MB\n", rss_mb(0));
    ref_t0 = p->o.region ? (int32_t)p->g_tid : 0; ref_t1 = (p->o.region && p->g_end) ? ref_t0 + 1 : p->bam->n_targets;       /* (before the reader moves the schedule) */
    /* the per-record work of a chunk (admission, strand, name pairing, CIGAR expansion) runs on the device; MDK_HOST_PREP=1 keeps
     * it on the host's chunk workers (the round-1 arrangement, and what a chunk the device gives up on falls back to) */
    if(!getenv("MDK_HOST_PREP")) mdk_plan_set_prep(p, 1);
    mdk_plan_set_hold(p, MDK_NGROUPS * MDK_GROUP + 2);
    if(!p->started && pipeline_start(p)) { if(dop.started) pthread_join(dop.th, NULL); if(dop.d.dev) md_dev_close(dop.d.dev); mdk_plan_close(p); return -5; }
    if(S) session_device(S, &dop.d);          /* the session's handle: opened once, then reset to this run's configuration */
    else if(dop.started) pthread_join(dop.th, NULL); else { xopen_start(p, &dop); if(dop.started) pthread_join(dop.th, NULL); else devopen_main(&dop.d); }
    t_dev = now_s() - T0;
    if(getenv("MDK_HOST_PROFILE")) fprintf(stderr, "[mdk main] resident at device ready %.0f MB\n", rss_mb(0));
    dev = dop.d.dev;
    if(dop.d.rc) { fprintf(stderr, "[mdk] cannot open MI355X device %d: %s\n[mdk] this build has no CPU path for `extract`.\n", user_device(dop.d.device), dop.d.err); mdk_plan_close(p); return MDK_RC_NODEVICE; }
    (void)md_dev_reserve_contigs(dev, p->bam->n_targets);
    if(p->dev_prep) { md_prep_cfg pc; mdk_plan_prep_cfg(p, &pc); md_dev_set_prep(dev, &pc); }
    if(p->dev_prep) mdk_plan_attach_device(p, dev);      /* from here on the device inflates pieces of the file too */
    X = calloc(1, sizeof(*X));
    if(X) X->ref_state = calloc((size_t)p->bam->n_targets + 1, sizeof(int));
    if(X && mbias) X->sink = SINK_BIAS;
    else if(X && cyto) {       /* the report's sink: the variant filter and the contexts of the text post-pass, no depth test */
        md_cyto_cfg yc; memset(&yc, 0, sizeof(yc));
        yc.min_opposite_depth = p->o.min_opp_depth > 0 ? p->o.min_opp_depth : 0; yc.max_variant_frac = p->o.max_variant_frac;
        for(i = 0; i < 3; i++) yc.ctx_on[i] = p->o.ctx_on[i];
        X->sink = SINK_CYTO;
        if(md_dev_cytosines_begin(dev, &yc)) { fprintf(stderr, "[mdk] device error: %s\n", md_dev_last_error()); free(X->ref_state); free(X); mdk_plan_detach_device(p); mdk_plan_close(p); return MDK_RC_DEVICE; }
    }
    else if(X && S) {     /* the session's sink: the calls configuration is the text post-pass's */
        md_calls_cfg cc; memset(&cc, 0, sizeof(cc));
        cc.min_depth = p->o.min_depth; cc.merge = p->o.merge; cc.min_opposite_depth = p->o.min_opp_depth > 0 ? p->o.min_opp_depth : 0; cc.max_variant_frac = p->o.max_variant_frac;
        for(i = 0; i < 3; i++) cc.ctx_on[i] = p->o.ctx_on[i];
        X->sink = SINK_CALLS;
        if(md_dev_calls_begin(dev, &cc)) { fprintf(stderr, "[mdk] device error: %s\n", md_dev_last_error()); free(X->ref_state); free(X); mdk_plan_detach_device(p); mdk_plan_close(p); return MDK_RC_DEVICE; }
    }
    if(!X || !X->ref_state || (!S && emitter_start(&em, p, emit_threads(p)))) { if(X) free(X->ref_state); free(X); mdk_plan_detach_device(p); if(!S) md_dev_close(dev); mdk_plan_close(p); return -5; }
    X->p = p; X->dev = dev; X->em = S ? NULL : &em; X->ref_t0 = ref_t0; X->ref_t1 = ref_t1; pthread_mutex_init(&X->mu, NULL); pthread_cond_init(&X->cv, NULL);
    for(g_i = 0; g_i < MDK_NGROUPS; g_i++) for(i = 0; i < MDK_GROUP; i++) X->G[g_i].slot[i] = g_i * MDK_GROUP + i;
    preg_ok = !getenv("MDK_NO_PREREG") && pthread_create(&preg, NULL, prereg_main, dev) == 0;
    rth_ok = pthread_create(&rth, NULL, refs_main, X) == 0;
    cth_ok = pthread_create(&cth, NULL, collector_main, X) == 0;
    if(getenv("MDK_WATCHDOG")) { pthread_t wd; if(pthread_create(&wd, NULL, watchdog_main, X) == 0) pthread_detach(wd); }
    if(!rth_ok || !cth_ok) { fprintf(stderr, "[mdk] cannot create a thread\n"); ret = -5; more = 0; }
    while(more && !ret) {
        cgroup *g;
        /* the next group, once the collector has given it back */
        ta = now_s(); g_up_phase = 1;
        pthread_mutex_lock(&X->mu);
        g = &X->G[X->n_up % MDK_NGROUPS];
        while(g->state != G_FREE && !X->ret) pthread_cond_wait(&X->cv, &X->mu);
        ret = X->ret; g->state = G_FILL;
        pthread_mutex_unlock(&X->mu);
        w_group += now_s() - ta;
        if(ret) break;
        g_up_phase = 2; ta = now_s(); while(g->held) release_uploaded(X, 1); release_uploaded(X, 0); w_rel += now_s() - ta; g_up_phase = 3;
        /* the first chunk is waited for, the others are taken only if they are ready now */
        g->n = 0;
        while(more && g->n < MDK_GROUP) {
            mdk_chunk *c = &g->ch[g->n];
            ta = now_s();
            rc = mdk_plan_try_next_chunk(p, c);
            if(rc == 2 && g->n == 0) {      /* nothing ready: before waiting, give back what can be given back -- the reader may be short of that very memory */
                const double tb = now_s(); g_up_phase = 4; release_uploaded(X, 1); w_rel += now_s() - tb; ta += now_s() - tb;
                g_up_phase = 5; rc = mdk_plan_next_chunk(p, c); g_up_phase = 3;
            }
            w_next += now_s() - ta;
            if(rc == 2) break;
            if(rc < 0) { ret = rc == -5 ? -5 : -4; break; }
            if(rc == 0) { more = 0; break; }
            g->launched[g->n] = 0; g->inplace[g->n] = 0; g->single[g->n] = 0;
            if(mbias && (c->skipped & MDK_CHUNK_NOREF)) { ret = -4; break; }      /* as mbias_main: the reference's worker gives up here (MBias.c:150-155,543) */
            if(!c->skipped) {
                ta = now_s(); rc = c->prep ? 0 : ref_wait(X, c->tid); w_ref += now_s() - ta;       /* (raw records can cross the link before the contig's bases have) */
                ta = now_s(); g_up_phase = 6;
                g->inplace[g->n] = 0;
                if(!rc) { if(c->prep) { rc = md_dev_upload_raw_inplace(dev, g->slot[g->n], &c->raw); if(rc > 0) { g->inplace[g->n] = 1; rc = 0; } } else if(mbias) { rc = md_dev_mbias_submit(dev, g->slot[g->n], &c->batch); g->single[g->n] = 1; } else rc = md_dev_upload(dev, g->slot[g->n], &c->batch); }
                w_sub += now_s() - ta; g_up_phase = 3;
                if(rc) { fprintf(stderr, "[mdk] device error: %s\n", md_dev_last_error()); ret = MDK_RC_DEVICE; break; }
                g->launched[g->n] = 1;
            }
            g->n++; n_chunks++;
        }
        if(ret) break;
        {   /* one launch per kernel for the group's chunks */
            int ls[MDK_GROUP], nl = 0;
            for(i = 0; i < g->n; i++) if(g->launched[i] && !g->single[i]) ls[nl++] = g->slot[i];
            ta = now_s(); g_up_phase = 7;
            for(i = 0, rc = 0; i < g->n && !rc; i++) if(g->launched[i] && g->ch[i].prep) rc = ref_wait(X, g->ch[i].tid);
            w_ref += now_s() - ta;
            if(rc) { fprintf(stderr, "[mdk] device error: %s\n", md_dev_last_error()); ret = MDK_RC_DEVICE; break; }
            g_up_phase = 8;
            if(nl) { ta = now_s(); rc = mbias ? md_dev_mbias_group(dev, ls, nl) : md_dev_launch_group(dev, ls, nl); w_sub += now_s() - ta; if(rc) { fprintf(stderr, "[mdk] device error: %s\n", md_dev_last_error()); ret = MDK_RC_DEVICE; break; } }
        }
        g->n_held = g->n; g->held = 0;
        for(i = 0; i < g->n; i++) { g->rel_slot[i] = (g->launched[i] && g->ch[i].prep && !g->inplace[i]) ? g->slot[i] : -1; g->rel_ch[i] = g->ch[i]; if(g->rel_slot[i] >= 0 && !getenv("MDK_NO_EARLY_RELEASE")) g->held = 1; }
        pthread_mutex_lock(&X->mu);
        if(g->n) { g->state = G_LAUNCHED; X->n_up++; } else g->state = G_FREE;
        pthread_cond_broadcast(&X->cv);
        pthread_mutex_unlock(&X->mu);
        ta = now_s(); release_uploaded(X, 0); w_rel += now_s() - ta;
    }
    /* the last groups' records have crossed the link or are about to: their slabs go back too (to the reaper: the file has been read to its end),
     * instead of staying registered until the process ends */
    if(!ret) { int guard = 0; for(;;) { int any = 0; for(i = 0; i < MDK_NGROUPS; i++) any |= X->G[i].held; if(!any || ++guard > 2 * MDK_NGROUPS_MAX) break; release_uploaded(X, 1); } }
    if(ret) xp_fail(X, ret);
    pthread_mutex_lock(&X->mu); X->up_done = 1; X->ref_quit = 1; pthread_cond_broadcast(&X->cv); pthread_mutex_unlock(&X->mu);
    if(cth_ok) pthread_join(cth, NULL);
    if(rth_ok) pthread_join(rth, NULL);
    if(preg_ok) pthread_join(preg, NULL);
    if(!ret) ret = X->ret;
    if(ret && S) (void)md_dev_sync(dev);      /* a session's run that ends early: what its groups queued (copies from the slabs, kernels over the pieces) has run before the plan gives that memory back */
    if(!S) { double tw = now_s(); emitter_stop(&em); X->w_emit += now_s() - tw; }
    if(em.failed && !ret) ret = MDK_RC_OUTPUT;
    if(getenv("MDK_HOST_PROFILE")) { double rs = 0; uint64_t rc2 = 0, rb = 0; md_host_profile(&rs, &rc2, &rb); fprintf(stderr, "[mdk main] staging blocks registered: %" PRIu64 " (%.0f MB) in %.3fs; %" PRIu64 " chunks in %" PRIu64 " group launches\n", rc2, rb / 1048576.0, rs, n_chunks, X->n_up); }
    if(getenv("MDK_HOST_PROFILE")) { char pt[1024]; if(md_dev_profile_text(pt, sizeof(pt)) == 0) fprintf(stderr, "[mdk hip] host threads inside the device library: %s\n", pt); }
    if(getenv("MDK_HOST_PROFILE")) fprintf(stderr, "[mdk main] plan open %.3fs, device ready at %.3fs, uploader: wait-for-chunk %.3fs wait-for-reference %.3fs wait-for-group %.3fs submit %.3fs wait-for-uploads %.3fs; collector: download %.3fs emit %.3fs, total %.3fs; chunks prepared on the host after all: %d\n", t_open, t_dev, w_next, w_ref, w_group, w_sub, w_rel, X->w_down, X->w_emit, now_s() - T0, X->n_host_prep);
    if(mbias) {      /* the table, the dense histogram and -- from the histogram read back with the row count -- the bounds the command suggests */
        md_bias_set *set = NULL; const int frc = ret ? 0 : md_dev_bias_finish(dev, &set);
        if(frc == MDK_ERR_STRAND0) { fprintf(stderr, "Can't determine the strand of a read!\n"); abort(); }
        if(getenv("MDK_HOST_PROFILE") && set) fprintf(stderr, "[mdk main] mbias: %d chunks counted through the single-chunk path after their group launch\n", md_bias_set_redone(set));
        ret = session_result(ret, frc, p, sizeof(mdk_bias), set, set ? md_bias_set_count(set) : 0, out);
        if(ret) md_bias_set_free(set);
        else { mdk_bias *b = *out; md_mbias hist; b->len = md_bias_set_len(set); b->redone = md_bias_set_redone(set); if(md_bias_set_hist(set, &hist) || mdk_mbias_suggest(&hist, b->bounds, b->has)) { mdk_bias_free(b); *out = NULL; ret = MDK_RC_DEVICE; } }
    } else if(cyto) {       /* the report's rows, in schedule order; the handle's state is finished either way */
        md_cytosines_set *set = NULL; const int frc = md_dev_cytosines_finish(dev, &set);
        ret = session_result(ret, frc, p, sizeof(mdk_cytosines), set, md_cytosines_set_count(set), out);
        if(ret) md_cytosines_set_free(set);
    } else if(S) {          /* the rows, in schedule order, handed over with the contig names; the handle's calls state is finished either way */
        md_calls_set *set = NULL; const int frc = md_dev_calls_finish(dev, &set);
        ret = session_result(ret, frc, p, sizeof(mdk_calls), set, md_calls_set_count(set), out);
        if(ret) md_calls_set_free(set);
    } else if(ret == 0) mdk_plan_finish(p);
    if(getenv("MDK_HOST_PROFILE")) { struct timespec ts; clock_gettime(CLOCK_REALTIME, &ts); fprintf(stderr, "[mdk main] leaving at epoch %.3f (resident %.0f MB, of which file-backed/shared %.0f MB)\n", ts.tv_sec + 1e-9 * ts.tv_nsec, rss_mb(0), rss_mb(1)); }
    if(!S && fast_exit_wanted()) leave_fast_plan(p, ret);
    { double tc = now_s(), td;
      pthread_mutex_destroy(&X->mu); pthread_cond_destroy(&X->cv); free(X->ref_state); free(X);
      mdk_plan_detach_device(p);
      if(!S) md_dev_close(dev);
      td = now_s();
      mdk_plan_close(p);
      if(getenv("MDK_HOST_PROFILE")) fprintf(stderr, "[mdk main] device closed in %.3fs, plan (slabs, reference, mapped file) in %.3fs\n", td - tc, now_s() - td); }
    return ret;
}

static int extract_run(int argc, char *argv[], mdk_session *S, void **out) { return pipeline_run(argc, argv, S, out, RUN_EXTRACT); }
MDK_LOCAL int session_mbias_run(int argc, char *argv[], mdk_session *S, void **out) { return pipeline_run(argc, argv, S, out, RUN_MBIAS); }
static int cytosines_run(int argc, char *argv[], mdk_session *S, void **out) { return pipeline_run(argc, argv, S, out, RUN_CYTO); }

int extract_main(int argc, char *argv[]) {
    { int rk = 0, wd = 1, m = ranks_from_env(&rk, &wd); if(m < 0) return -1; if(m > 0) return extract_ranks(argc, argv, rk, wd); }       /* one process per GPU (mdk_ranks.c) */
    return extract_run(argc, argv, NULL, NULL);
}

int mdk_session_extract(mdk_session *s, int argc, char *argv[], mdk_calls **out) { return session_run(s, argc, argv, (void **)out, sizeof(mdk_calls), extract_run); }
int64_t mdk_calls_count(const mdk_calls *c) { return c ? c->r.n : -1; }
int mdk_calls_n_contigs(const mdk_calls *c) { return result_n_contigs(c ? &c->r : NULL); }
const char *mdk_calls_contig_name(const mdk_calls *c, int i) { return result_contig_name(c ? &c->r : NULL, i); }
int mdk_calls_merged(const mdk_calls *c) { return c ? c->r.merged : -1; }
int mdk_calls_contexts(const mdk_calls *c) { return c ? c->r.contexts : -1; }
int mdk_calls_copy(const mdk_calls *c, int column, void *dst, int to_host) {
    md_calls_cols d; memset(&d, 0, sizeof(d));
    if(!c || !dst || column < 0 || column > MDK_CALLS_STRAND) return MDK_ERR_ARG;
    if(!c->r.set || c->r.n == 0) return 0;
    switch(column) {
    case MDK_CALLS_CONTIG: d.contig = dst; break;
    case MDK_CALLS_START: d.start = dst; break;
    case MDK_CALLS_END: d.end = dst; break;
    case MDK_CALLS_NMETH: d.nmeth = dst; break;
    case MDK_CALLS_NUNMETH: d.nunmeth = dst; break;
    case MDK_CALLS_CONTEXT: d.context = dst; break;
    default: d.strand = dst; break;
    }
    return md_calls_set_copy(c->r.set, &d, to_host);
}
void mdk_calls_free(mdk_calls *c) { if(c) { md_calls_set_free(c->r.set); session_result_free(&c->r); } }

int mdk_session_cytosines(mdk_session *s, int argc, char *argv[], mdk_cytosines **out) { return session_run(s, argc, argv, (void **)out, sizeof(mdk_cytosines), cytosines_run); }
int64_t mdk_cytosines_count(const mdk_cytosines *c) { return c ? c->r.n : -1; }
int mdk_cytosines_n_contigs(const mdk_cytosines *c) { return result_n_contigs(c ? &c->r : NULL); }
const char *mdk_cytosines_contig_name(const mdk_cytosines *c, int i) { return result_contig_name(c ? &c->r : NULL, i); }
int mdk_cytosines_contexts(const mdk_cytosines *c) { return c ? c->r.contexts : -1; }
int mdk_cytosines_copy(const mdk_cytosines *c, int column, void *dst, int to_host) {
    md_cytosines_cols d; memset(&d, 0, sizeof(d));
    if(!c || !dst || column < 0 || column > MDK_CYTOSINES_TRINUCLEOTIDE) return MDK_ERR_ARG;
    if(!c->r.set || c->r.n == 0) return 0;
    switch(column) {
    case MDK_CYTOSINES_CONTIG: d.contig = dst; break;
    case MDK_CYTOSINES_POS: d.pos = dst; break;
    case MDK_CYTOSINES_STRAND: d.strand = dst; break;
    case MDK_CYTOSINES_NMETH: d.nmeth = dst; break;
    case MDK_CYTOSINES_NUNMETH: d.nunmeth = dst; break;
    case MDK_CYTOSINES_CONTEXT: d.context = dst; break;
    default: d.trinucleotide = dst; break;
    }
    return md_cytosines_set_copy(c->r.set, &d, to_host);
}
void mdk_cytosines_free(mdk_cytosines *c) { if(c) { md_cytosines_set_free(c->r.set); session_result_free(&c->r); } }
