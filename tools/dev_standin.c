/* dev_standin.c -- TEST INFRASTRUCTURE: the whole device library (include/mdk_hip.h) without a device, as a library to LD_PRELOAD in front of
 * libmdk_hip.so, so that the COMMAND ITSELF -- extract_main's uploader / collector / reference threads (csrc/host/mdk_extract.c) and the
 * one-process-per-GPU driver (csrc/host/mdk_ranks.c: schedule sharding, the ring of chunks in flight on rank 0, the control and data
 * connections, ordered emission, a chunk handed back to the host) -- runs on a CPU-only box: tests/test_ranks_cpu.py.
 * "Device memory" is host memory; BGZF pieces are tools/piece_standin.c (zlib); and what a slot "computes" is looked up, by the slot's
 * contig and interval, in the per-column counters the oracle dumped for the same command line (MDK_ORACLE_DUMP -> MDK_STANDIN_DUMP): the
 * counting itself is what the GPU tests check, everything AROUND it is what runs here.  MDK_STANDIN_HANDBACK=k makes every k-th uploaded chunk
 * come back with MDK_ERR_PREP_HOST once, as a chunk with an over-long read-name chain does on the device; MDK_STANDIN_US_PER_KREC=t makes a
 * chunk take t microseconds per 1000 records on the "device" ("compute time" in the background, for the work balance between ranks).
 * perRead (tests/test_reads_cpu.py): a chunk's reads are selected from its records as the device selects them, and their counts are the
 * oracle's `perRead` lines for the same command line, in order (MDK_STANDIN_PERREAD); md_dev_reads_* keep the rows in host memory.
 * mbias (tests/test_bias_cpu.py): the stand-in cannot count, so the histogram of the process's i-th mbias run is GIVEN -- the oracle's --noSVG
 * table, $MDK_STANDIN_MBIAS/<i>.txt, added when the run's first chunk is submitted; md_dev_bias_finish restates k_bias_rows' order rule.
 * cytosine report (tests/test_cytosines_cpu.py): md_dev_set_reference keeps a copy of each contig, and md_dev_cytosines_* restate the rules of
 * csrc/mdk_cytosines.hip over those bases and the slot's sites.
 *   build: gcc -O2 -shared -fPIC -Iinclude -o tools/_build/libmdk_dev_standin.so tools/dev_standin.c -lz -lpthread */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdio.h>
#include <time.h>
#include <unistd.h>
#include "piece_standin.c"

typedef struct { int32_t tid; uint32_t pos, nm, nu, meta, noff, nvar; } row_t;
static row_t *g_row; static size_t g_nrow; static pthread_once_t g_once = PTHREAD_ONCE_INIT;
static __thread char t_err[256];
static void load_dump(void) {
    const char *fn = getenv("MDK_STANDIN_DUMP"); FILE *f = fn ? fopen(fn, "r") : NULL; size_t cap = 0; int tid, pos, type, isg; unsigned a, b, c, d;
    if(!f) return;
    while(fscanf(f, "%d %d %d %d %u %u %u %u", &tid, &pos, &type, &isg, &a, &b, &c, &d) == 8) {
        if(g_nrow == cap) { cap = cap ? cap * 2 : 1 << 16; g_row = realloc(g_row, sizeof(row_t) * cap); if(!g_row) abort(); }
        g_row[g_nrow].tid = tid; g_row[g_nrow].pos = (uint32_t)pos; g_row[g_nrow].nm = a; g_row[g_nrow].nu = b; g_row[g_nrow].meta = (uint32_t)((isg ? 1 : 0) | (type << 1)); g_row[g_nrow].noff = c; g_row[g_nrow].nvar = d; g_nrow++;
    }
    fclose(f);
}
static double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
typedef struct { double ready_at; int used, launched, handed_back; int32_t tid; int64_t beg, end; uint8_t *raw; uint64_t raw_bytes, raw_cap; uint32_t *off; uint32_t n_rec, off_cap; md_site *site; md_site_var *var; int64_t cap; } sslot;
typedef struct { int32_t start, end, nm, nu; uint8_t ctx; int8_t strand; } crow_t;
typedef struct { uint32_t key; int32_t tid; crow_t *row; int64_t n; } cchunk_t;
typedef struct { int32_t pos, nm, nu; int8_t strand; uint8_t ctx, tri[3]; } yrow_t;
struct ychunk { uint32_t key; int32_t tid; yrow_t *row; int64_t n; };
typedef struct { uint32_t *kept; md_pr_count *cnt; int64_t n, cap; int pending; } prslot_t;       /* perRead: the kept reads of a slot's chunk and their counts */
struct md_dev { md_dev_cfg cfg; int n_slots; sslot *slot; long n_up; int handback; pthread_mutex_t mu; double busy_until; int us_per_krec;
                md_calls_cfg ccfg; int calls_on; cchunk_t *cch; int n_cch, cap_cch;
                md_prep_cfg prep; prslot_t *pr; int64_t pr_next;           /* pr_next: the oracle's perRead line the next kept read must match */
                uint32_t *mb_hist; int mb_len, mb_loaded;                  /* mbias: the given histogram [q][16], its rows, whether this run's table is in */
                char **ref; int64_t *reflen; int n_ref;                   /* the contigs' bases (md_dev_set_reference), for the cytosine report */
                md_cyto_cfg ycfg; int cyto_on; struct ychunk *ych; int n_ych, cap_ych;
                int reads_on; int32_t *r_contig, *r_pos, *r_nm, *r_nu; int64_t *r_off; uint8_t *r_bytes; int64_t r_n, r_cap, r_nb, r_capb; };
const char *md_dev_last_error(void) { return t_err; }
int md_dev_count(void) { return 1; }
int md_dev_warm(int device) { (void)device; return 0; }
void md_dev_quiesce(void) { }
void md_dev_reserve_hint(uint64_t device_bytes) { (void)device_bytes; }
int md_dev_open(int device, const md_dev_cfg *cfg, md_dev **out) {
    md_dev *h = calloc(1, sizeof(*h)); (void)device;
    pthread_once(&g_once, load_dump);
    if(!h || !cfg) return MDK_ERR_ARG;
    if(!g_row && getenv("MDK_STANDIN_DUMP") == NULL) { snprintf(t_err, sizeof t_err, "dev_standin: MDK_STANDIN_DUMP is not set"); free(h); return MDK_ERR_NODEVICE; }
    h->cfg = *cfg; h->n_slots = cfg->n_slots > 0 ? cfg->n_slots : 2; h->slot = calloc((size_t)h->n_slots, sizeof(sslot)); pthread_mutex_init(&h->mu, NULL);
    h->handback = getenv("MDK_STANDIN_HANDBACK") ? atoi(getenv("MDK_STANDIN_HANDBACK")) : 0;
    h->us_per_krec = getenv("MDK_STANDIN_US_PER_KREC") ? atoi(getenv("MDK_STANDIN_US_PER_KREC")) : 0;
    *out = h; return h->slot ? 0 : MDK_ERR_NOMEM;
}
static void calls_drop(md_dev *h) { int i; for(i = 0; i < h->n_cch; i++) free(h->cch[i].row); free(h->cch); h->cch = NULL; h->n_cch = h->cap_cch = 0; h->calls_on = 0; }
static void reads_drop(md_dev *h) { free(h->r_contig); free(h->r_pos); free(h->r_nm); free(h->r_nu); free(h->r_off); free(h->r_bytes); h->r_contig = h->r_pos = h->r_nm = h->r_nu = NULL; h->r_off = NULL; h->r_bytes = NULL; h->r_n = h->r_cap = h->r_nb = h->r_capb = 0; h->reads_on = 0; }
static void cyto_drop(md_dev *h) { int i; for(i = 0; i < h->n_ych; i++) free(h->ych[i].row); free(h->ych); h->ych = NULL; h->n_ych = h->cap_ych = 0; h->cyto_on = 0; }
static void refs_drop(md_dev *h) { int i; for(i = 0; i < h->n_ref; i++) free(h->ref[i]); free(h->ref); free(h->reflen); h->ref = NULL; h->reflen = NULL; h->n_ref = 0; }
void md_dev_close(md_dev *h) {
    int i; if(!h) return; calls_drop(h); reads_drop(h); cyto_drop(h); refs_drop(h); free(h->mb_hist);
    for(i = 0; i < h->n_slots; i++) { free(h->slot[i].raw); free(h->slot[i].off); free(h->slot[i].site); free(h->slot[i].var); if(h->pr) { free(h->pr[i].kept); free(h->pr[i].cnt); } }
    free(h->pr); free(h->slot); free(h);
}
int md_dev_tile(const md_dev *h) { (void)h; return 2048; }
int md_dev_reserve_contigs(md_dev *h, int32_t n) { (void)h; (void)n; return 0; }
int md_dev_set_reference(md_dev *h, int32_t tid, const char *seq, int64_t len) {      /* (a thread of its own calls this, next to the collector) */
    char *copy;
    if(!h || tid < 0 || !seq || len < 0) return MDK_ERR_ARG;
    if(!(copy = malloc((size_t)len + 1))) return MDK_ERR_NOMEM;
    memcpy(copy, seq, (size_t)len);
    pthread_mutex_lock(&h->mu);
    if(tid >= h->n_ref) {
        h->ref = realloc(h->ref, sizeof(char *) * (size_t)(tid + 1)); h->reflen = realloc(h->reflen, sizeof(int64_t) * (size_t)(tid + 1));
        if(!h->ref || !h->reflen) abort();
        while(h->n_ref <= tid) { h->ref[h->n_ref] = NULL; h->reflen[h->n_ref] = 0; h->n_ref++; }
    }
    free(h->ref[tid]); h->ref[tid] = copy; h->reflen[tid] = len;
    pthread_mutex_unlock(&h->mu);
    return 0;
}
int md_dev_set_regions(md_dev *h, int32_t tid, const md_region *runs, int64_t n) { (void)h; (void)tid; (void)runs; (void)n; return 0; }
int md_dev_set_mappability(md_dev *h, int32_t tid, const uint32_t *bits, int64_t n) { (void)h; (void)tid; (void)bits; (void)n; return 0; }
int md_dev_set_prep(md_dev *h, const md_prep_cfg *cfg) { if(h && cfg) h->prep = *cfg; return 0; }
int md_dev_pci_bus_id(const md_dev *h, char *buf, int cap) { (void)h; snprintf(buf, (size_t)cap, "standin:00.0"); return 0; }      /* every rank "on the same device": the site buffers travel over the ranks' TCP connections */
int md_dev_profile_text(char *buf, int cap) { if(buf && cap > 0) snprintf(buf, (size_t)cap, "device stand-in (tools/dev_standin.c)"); return 0; }
void *md_host_alloc(uint64_t bytes) { return malloc((size_t)bytes + 64); }
void md_host_free(void *p) { free(p); }
void md_host_set_pinned(int on) { (void)on; }
void md_host_profile(double *s, uint64_t *c, uint64_t *b) { if(s) *s = 0; if(c) *c = 0; if(b) *b = 0; }
int md_host_register_all(md_dev *h, int threads) { (void)h; (void)threads; return 0; }
static sslot *slot_of(md_dev *h, int slot) { if(!h || slot < 0 || slot >= h->n_slots) { snprintf(t_err, sizeof t_err, "bad slot"); return NULL; } return &h->slot[slot]; }
/* the records as the device would hold them: the ranges back to back, and every record's offset there (csrc/mdk_prep.hip copy_ranges) */
int md_dev_upload_raw(md_dev *h, int slot, const md_raw_batch *b) {
    sslot *s = slot_of(h, slot); uint64_t total = 0, o = 0; uint32_t idx = 0, hidx = 0; int i, any_tab = 0;
    if(!s || !b) return MDK_ERR_ARG;
    for(i = 0; i < b->n_ranges; i++) { total += b->range[i].bytes; if(b->range[i].d_rec_off || b->range[i].h_rec_off) any_tab = 1; }
    if(s->raw_cap < total + 64) { free(s->raw); s->raw_cap = total + total / 8 + 64; s->raw = malloc(s->raw_cap); }
    if(s->off_cap < (uint32_t)b->n_records + 1) { free(s->off); s->off_cap = (uint32_t)b->n_records + 1024; s->off = malloc(sizeof(uint32_t) * s->off_cap); }
    if(!s->raw || !s->off) return MDK_ERR_NOMEM;
    for(i = 0; i < b->n_ranges; i++) {
        const md_raw_range *r = &b->range[i]; uint32_t k;
        if(r->bytes) memcpy(s->raw + o, r->ptr, (size_t)r->bytes);
        if(r->d_rec_off || r->h_rec_off) { const uint32_t *t = r->d_rec_off ? r->d_rec_off : r->h_rec_off; for(k = 0; k < r->n_records; k++) s->off[idx + k] = t[k] - r->rec_delta + (uint32_t)o; idx += r->n_records; }
        else if(any_tab) { for(k = 0; k < r->n_records; k++) s->off[idx + k] = b->rec_off[hidx + k]; idx += r->n_records; hidx += r->n_records; }
        o += r->bytes;
    }
    if(!any_tab) { for(idx = 0; idx < (uint32_t)b->n_records; idx++) s->off[idx] = b->rec_off[idx]; }
    if(idx != (uint32_t)b->n_records) { snprintf(t_err, sizeof t_err, "dev_standin: %u record offsets for %d records", idx, b->n_records); return MDK_ERR_ARG; }
    for(idx = 0; idx < (uint32_t)b->n_records; idx++) {       /* every offset names a record inside the bytes, in order, back to back */
        const uint32_t at = s->off[idx]; uint32_t bs;
        if((uint64_t)at + 36 > total) { snprintf(t_err, sizeof t_err, "dev_standin: record %u at %u beyond %llu bytes", idx, at, (unsigned long long)total); return MDK_ERR_ARG; }
        memcpy(&bs, s->raw + at, 4);
        if(idx + 1 < (uint32_t)b->n_records && s->off[idx + 1] != at + 4 + bs) { snprintf(t_err, sizeof t_err, "dev_standin: record %u does not end where record %u begins", idx, idx + 1); return MDK_ERR_ARG; }
        if(idx + 1 == (uint32_t)b->n_records && (uint64_t)at + 4 + bs != total) { snprintf(t_err, sizeof t_err, "dev_standin: the last record does not end with the bytes"); return MDK_ERR_ARG; }
    }
    s->raw_bytes = total; s->n_rec = (uint32_t)b->n_records; s->tid = b->tid; s->beg = b->beg; s->end = b->end; s->used = 1; s->launched = 0; s->handed_back = 0;
    pthread_mutex_lock(&h->mu); h->n_up++; if(h->handback > 0 && h->n_up % h->handback == 0) s->handed_back = 1; pthread_mutex_unlock(&h->mu);
    return 0;
}
int md_dev_upload_raw_inplace(md_dev *h, int slot, const md_raw_batch *b) { return md_dev_upload_raw(h, slot, b); }      /* (the stand-in always copies) */
int md_dev_upload_wait(md_dev *h, int slot) { return slot_of(h, slot) ? 0 : MDK_ERR_ARG; }
int md_dev_upload_done(md_dev *h, int slot) { static __thread unsigned n; return slot_of(h, slot) ? (int)(++n % 3 != 0) : MDK_ERR_ARG; }      /* "not yet" now and then: the caller's waiting path runs too */
int md_dev_upload(md_dev *h, int slot, const md_read_batch *b) { sslot *s = slot_of(h, slot); if(!s || !b) return MDK_ERR_ARG; s->tid = b->tid; s->beg = b->beg; s->end = b->end; s->used = 1; s->launched = 0; s->handed_back = 0; return 0; }
/* "compute time": MDK_STANDIN_US_PER_KREC microseconds per 1000 records of the chunk, one chunk after the other, in the background -- a download
 * waits for what is left of it (tests of the work balance between ranks) */
int md_dev_launch(md_dev *h, int slot) {
    sslot *s = slot_of(h, slot); if(!s || !s->used) return MDK_ERR_ARG;
    if(h->us_per_krec > 0) { const double t = now_s(); pthread_mutex_lock(&h->mu); s->ready_at = (h->busy_until > t ? h->busy_until : t) + 1e-9 * h->us_per_krec * s->n_rec; h->busy_until = s->ready_at; pthread_mutex_unlock(&h->mu); }
    s->launched = 1; return 0;
}
int md_dev_launch_group(md_dev *h, const int *slots, int n) { int i; for(i = 0; i < n; i++) if(md_dev_launch(h, slots[i])) return MDK_ERR_ARG; return 0; }
int md_dev_group_max(void) { return 8; }
int md_dev_submit(md_dev *h, int slot, const md_read_batch *b) { int rc = md_dev_upload(h, slot, b); return rc ? rc : md_dev_launch(h, slot); }
int md_dev_submit_raw(md_dev *h, int slot, const md_raw_batch *b) { int rc = md_dev_upload_raw(h, slot, b); return rc ? rc : md_dev_launch(h, slot); }
int md_dev_read_raw(md_dev *h, int slot, uint8_t *bytes, uint64_t *n_bytes, uint32_t *rec_off, uint32_t *n_records) {
    sslot *s = slot_of(h, slot);
    if(!s || !s->raw || *n_bytes < s->raw_bytes || *n_records < s->n_rec) return MDK_ERR_ARG;
    memcpy(bytes, s->raw, (size_t)s->raw_bytes); memcpy(rec_off, s->off, sizeof(uint32_t) * s->n_rec); *n_bytes = s->raw_bytes; *n_records = s->n_rec;
    return 0;
}
int md_dev_download(md_dev *h, int slot, md_sites *out) {
    sslot *s = slot_of(h, slot); size_t a = 0, b = g_nrow, i; int64_t n = 0; const int variant = h && h->cfg.minOppositeDepth > 0;
    if(!s || !out || !s->launched) { snprintf(t_err, sizeof t_err, "dev_standin: slot not launched"); return MDK_ERR_ARG; }
    memset(out, 0, sizeof(*out));
    { const double t = now_s(); if(s->ready_at > t) usleep((useconds_t)((s->ready_at - t) * 1e6)); }      /* the "device" is still computing this chunk */
    if(s->handed_back) { s->handed_back = 0; snprintf(t_err, sizeof t_err, "dev_standin: this chunk goes back to the host preparation"); return MDK_ERR_PREP_HOST; }
    while(a < b) { const size_t m = (a + b) / 2; if(g_row[m].tid < s->tid || (g_row[m].tid == s->tid && (int64_t)g_row[m].pos < s->beg)) a = m + 1; else b = m; }
    for(i = a; i < g_nrow && g_row[i].tid == s->tid && (int64_t)g_row[i].pos < s->end; i++) n++;
    if(n > s->cap) { free(s->site); free(s->var); s->cap = n + 1024; s->site = malloc(sizeof(md_site) * (size_t)s->cap); s->var = malloc(sizeof(md_site_var) * (size_t)s->cap); if(!s->site || !s->var) return MDK_ERR_NOMEM; }
    for(i = a, n = 0; i < g_nrow && g_row[i].tid == s->tid && (int64_t)g_row[i].pos < s->end; i++) {
        if(!(g_row[i].nm + g_row[i].nu > 0 || (variant && g_row[i].noff > 0))) continue;
        s->site[n].pos = g_row[i].pos; s->site[n].nmeth = g_row[i].nm; s->site[n].nunmeth = g_row[i].nu; s->site[n].meta = g_row[i].meta; s->var[n].noff = g_row[i].noff; s->var[n].nvar = g_row[i].nvar; n++;
    }
    out->n_sites = n; out->site = s->site; out->var = variant ? s->var : NULL;
    return 0;
}
int md_dev_download_group(md_dev *h, const int *slots, int n, md_sites *out, int *rc) { int i; for(i = 0; i < n; i++) rc[i] = md_dev_download(h, slots[i], &out[i]); return 0; }
int md_dev_slot_sync(md_dev *h, int slot) { return slot_of(h, slot) ? 0 : MDK_ERR_ARG; }
int md_dev_sync(md_dev *h) { (void)h; return 0; }
/* the exchange between GPUs is not stood in for: ranks that "share a device" use the command's TCP connections */
int md_comm_unique_id(uint8_t *id) { (void)id; snprintf(t_err, sizeof t_err, "dev_standin: no RCCL"); return MDK_ERR_NODEVICE; }

/* ---- calls on the "device": the rows k_calls_compact makes (csrc/mdk_calls.hip), restated over the slot's ascending sites ---- */
struct md_calls_set { int64_t n; int32_t *contig, *start, *end, *nm, *nu; uint8_t *ctx; int8_t *strand; };
int md_dev_reset(md_dev *h, const md_dev_cfg *cfg) {
    int i;
    if(!h || !cfg || (cfg->n_slots > 0 ? cfg->n_slots : 2) != h->n_slots) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_reset"); return MDK_ERR_ARG; }
    calls_drop(h); reads_drop(h); cyto_drop(h); refs_drop(h); memset(&h->prep, 0, sizeof(h->prep));
    free(h->mb_hist); h->mb_hist = NULL; h->mb_len = h->mb_loaded = 0;
    for(i = 0; i < h->n_slots; i++) { sslot *s = &h->slot[i]; s->used = s->launched = s->handed_back = 0; s->ready_at = 0; if(h->pr) h->pr[i].pending = 0; }
    h->cfg = *cfg;
    return 0;
}
int md_dev_calls_begin(md_dev *h, const md_calls_cfg *cfg) {
    if(!h || !cfg || cfg->min_depth < 1) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_calls_begin"); return MDK_ERR_ARG; }
    calls_drop(h); h->ccfg = *cfg; h->calls_on = 1;
    return 0;
}
static int c_variant(const md_dev *h, const md_sites *s, int64_t i) {
    return s->var && h->ccfg.min_opposite_depth > 0 && s->var[i].noff >= (uint32_t)h->ccfg.min_opposite_depth && (double)s->var[i].nvar / (double)s->var[i].noff >= h->ccfg.max_variant_frac;
}
static int64_t c_find(const md_sites *s, int64_t i, int dir, uint32_t pos, int type, int is_g) {      /* the site at `pos` within two of i, of that type and base */
    int k;
    for(k = 1; k <= 2; k++) { const int64_t j = i + dir * k; if(j < 0 || j >= s->n_sites) break; if(s->site[j].pos == pos && (int)(s->site[j].meta & 1) == is_g && (int)((s->site[j].meta >> 1) & 3) == type) return j; }
    return -1;
}
static int chunk_rows(md_dev *h, const md_sites *s, cchunk_t *c) {
    const md_calls_cfg *q = &h->ccfg; int64_t i;
    c->row = malloc(sizeof(crow_t) * (size_t)(s->n_sites + 1)); c->n = 0;
    if(!c->row) return MDK_ERR_NOMEM;
    for(i = 0; i < s->n_sites; i++) {
        const md_site *x = &s->site[i]; const int type = (x->meta >> 1) & 3, is_g = x->meta & 1;
        const int surv = !c_variant(h, s, i) && x->nmeth + x->nunmeth > 0;
        crow_t r; int has = 0; uint32_t m = 0, u = 0;
        if(!q->ctx_on[type]) continue;
        memset(&r, 0, sizeof(r)); r.ctx = (uint8_t)type;
        if(!q->merge || type == 2) { if(surv) { has = 1; r.start = (int32_t)x->pos; r.end = r.start + 1; m = x->nmeth; u = x->nunmeth; r.strand = is_g ? -1 : 1; } }
        else {
            const int d = type + 1;
            if(!is_g) {
                const int64_t g = c_find(s, i, 1, x->pos + (uint32_t)d, type, 1);
                const int vg = g >= 0 && c_variant(h, s, g), sg = g >= 0 && !vg && s->site[g].nmeth + s->site[g].nunmeth > 0;
                if(surv || sg) {
                    has = 1; r.start = (int32_t)x->pos; r.end = r.start + d + 1;
                    m = (surv ? x->nmeth : 0) + (sg ? s->site[g].nmeth : 0); u = (surv ? x->nunmeth : 0) + (sg ? s->site[g].nunmeth : 0);
                    if(surv && vg) m = u = 0;
                }
            } else if(surv && (x->pos < (uint32_t)d || c_find(s, i, -1, x->pos - (uint32_t)d, type, 0) < 0)) { has = 1; r.start = (int32_t)x->pos - d; r.end = (int32_t)x->pos + 1; m = x->nmeth; u = x->nunmeth; }
        }
        if(!has || m + u == 0 || m + u < (uint32_t)q->min_depth) continue;
        r.nm = (int32_t)m; r.nu = (int32_t)u; c->row[c->n++] = r;
    }
    return 0;
}
int md_dev_calls_group(md_dev *h, const int *slots, const uint32_t *keys, int n, int *rc) {
    int i;
    if(!h || !slots || !keys || !rc || n < 1 || !h->calls_on) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_calls_group"); return MDK_ERR_ARG; }
    for(i = 0; i < n; i++) {
        md_sites st; cchunk_t c;
        rc[i] = md_dev_download(h, slots[i], &st);
        if(rc[i]) continue;
        c.key = keys[i]; c.tid = h->slot[slots[i]].tid;
        if((rc[i] = chunk_rows(h, &st, &c)) != 0) continue;
        if(h->n_cch == h->cap_cch) { h->cap_cch = h->cap_cch ? 2 * h->cap_cch : 64; h->cch = realloc(h->cch, sizeof(cchunk_t) * (size_t)h->cap_cch); if(!h->cch) return MDK_ERR_NOMEM; }
        h->cch[h->n_cch++] = c;
    }
    return 0;
}
static int cchunk_cmp(const void *a, const void *b) { const cchunk_t *x = a, *y = b; return x->key < y->key ? -1 : x->key > y->key; }
int md_dev_calls_finish(md_dev *h, md_calls_set **out) {
    md_calls_set *r; int64_t n = 0, o = 0; int i, k;
    if(!h || !out || !h->calls_on) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_calls_finish"); return MDK_ERR_ARG; }
    qsort(h->cch, (size_t)h->n_cch, sizeof(cchunk_t), cchunk_cmp);
    for(i = 0; i < h->n_cch; i++) n += h->cch[i].n;
    r = calloc(1, sizeof(*r)); if(!r) return MDK_ERR_NOMEM;
    r->n = n; r->contig = malloc(4 * (size_t)(n + 1)); r->start = malloc(4 * (size_t)(n + 1)); r->end = malloc(4 * (size_t)(n + 1)); r->nm = malloc(4 * (size_t)(n + 1)); r->nu = malloc(4 * (size_t)(n + 1));
    r->ctx = malloc((size_t)n + 1); r->strand = malloc((size_t)n + 1);
    for(i = 0; i < h->n_cch; i++) for(k = 0; k < h->cch[i].n; k++, o++) {
        const crow_t *x = &h->cch[i].row[k];
        r->contig[o] = h->cch[i].tid; r->start[o] = x->start; r->end[o] = x->end; r->nm[o] = x->nm; r->nu[o] = x->nu; r->ctx[o] = x->ctx; r->strand[o] = x->strand;
    }
    calls_drop(h);
    *out = r;
    return 0;
}
int64_t md_calls_set_count(const md_calls_set *c) { return c ? c->n : MDK_ERR_ARG; }
int md_calls_set_copy(const md_calls_set *c, const md_calls_cols *d, int to_host) {
    const size_t n = c ? (size_t)c->n : 0; (void)to_host;      /* ("device" memory is host memory here) */
    if(!c || !d) return MDK_ERR_ARG;
    if(d->contig) memcpy(d->contig, c->contig, 4 * n);
    if(d->start) memcpy(d->start, c->start, 4 * n);
    if(d->end) memcpy(d->end, c->end, 4 * n);
    if(d->nmeth) memcpy(d->nmeth, c->nm, 4 * n);
    if(d->nunmeth) memcpy(d->nunmeth, c->nu, 4 * n);
    if(d->context) memcpy(d->context, c->ctx, n);
    if(d->strand) memcpy(d->strand, c->strand, n);
    return 0;
}
void md_calls_set_free(md_calls_set *c) { if(!c) return; free(c->contig); free(c->start); free(c->end); free(c->nm); free(c->nu); free(c->ctx); free(c->strand); free(c); }

/* ---- the cytosine report on the "device": the rows k_cyto_fill makes (csrc/mdk_cytosines.hip), restated over the contig's bases and the slot's sites ---- */
struct md_cytosines_set { int64_t n; int32_t *contig, *pos, *nm, *nu; int8_t *strand; uint8_t *ctx, *tri; };
static int y_at(const char *seq, int64_t len, int64_t i) { return (i >= 0 && i < len) ? (unsigned char)seq[i] : 0; }      /* past either end: no base */
static int y_code(const char *seq, int64_t len, int64_t i) {       /* k_classify's code: 0, or 1 + 2 * type + isG */
    const int c = y_at(seq, len, i) & 0x5f;
    if(c == 'C') return (y_at(seq, len, i + 1) & 0x5f) == 'G' ? 1 : (y_at(seq, len, i + 2) & 0x5f) == 'G' ? 3 : 5;
    if(c == 'G') return (y_at(seq, len, i - 1) & 0x5f) == 'C' ? 2 : (y_at(seq, len, i - 2) & 0x5f) == 'C' ? 4 : 6;
    return 0;
}
static uint8_t y_fwd(int b) { b &= 0x5f; return (b == 'A' || b == 'C' || b == 'G' || b == 'T') ? (uint8_t)b : (uint8_t)'N'; }
static uint8_t y_comp(int b) { switch(b) { case 'A': case 'a': return 'T'; case 'C': case 'c': return 'G'; case 'G': case 'g': return 'C'; case 'T': case 't': return 'A'; default: return 'N'; } }
int md_dev_cytosines_begin(md_dev *h, const md_cyto_cfg *cfg) {
    if(!h || !cfg || (!cfg->ctx_on[0] && !cfg->ctx_on[1] && !cfg->ctx_on[2])) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_cytosines_begin"); return MDK_ERR_ARG; }
    cyto_drop(h); h->ycfg = *cfg; h->cyto_on = 1;
    return 0;
}
int md_dev_cytosines_group(md_dev *h, const int *slots, const md_cyto_chunk *chunks, int n, int *rc) {
    int i;
    if(!h || !slots || !chunks || !rc || n < 1 || n > 8 || !h->cyto_on) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_cytosines_group"); return MDK_ERR_ARG; }
    for(i = 0; i < n; i++) {
        const md_cyto_chunk *q = &chunks[i]; md_sites st; struct ychunk c; const char *seq; int64_t len, p, k = 0, end;
        memset(&st, 0, sizeof(st)); rc[i] = 0;
        pthread_mutex_lock(&h->mu);
        seq = (q->tid >= 0 && q->tid < h->n_ref) ? h->ref[q->tid] : NULL; len = seq ? h->reflen[q->tid] : 0;
        pthread_mutex_unlock(&h->mu);
        if(!seq) { snprintf(t_err, sizeof t_err, "dev_standin: reference for tid %d not uploaded", q->tid); return MDK_ERR_NOREF; }
        if(slots[i] >= 0) {
            sslot *s = slot_of(h, slots[i]);
            if(!s || s->tid != q->tid || s->beg != q->beg || s->end != q->end) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_cytosines_group: the slot holds another chunk"); return MDK_ERR_ARG; }
            rc[i] = md_dev_download(h, slots[i], &st);
            if(rc[i]) continue;
        }
        end = q->end < len ? q->end : len;
        c.key = q->key; c.tid = q->tid; c.n = 0; c.row = malloc(sizeof(yrow_t) * (size_t)((end > q->beg ? end - q->beg : 0) + 1));
        if(!c.row) return MDK_ERR_NOMEM;
        for(p = q->beg; p < end; p++) {
            const int code = y_code(seq, len, p); yrow_t *r; int is_g;
            if(!code || !h->ycfg.ctx_on[(code - 1) >> 1]) continue;
            r = &c.row[c.n++]; is_g = !(code & 1);
            r->pos = (int32_t)p + 1; r->strand = is_g ? -1 : 1; r->ctx = (uint8_t)((code - 1) >> 1); r->nm = r->nu = 0;
            r->tri[0] = 'C'; r->tri[1] = is_g ? y_comp(y_at(seq, len, p - 1)) : y_fwd(y_at(seq, len, p + 1)); r->tri[2] = is_g ? y_comp(y_at(seq, len, p - 2)) : y_fwd(y_at(seq, len, p + 2));
            while(k < st.n_sites && (int64_t)st.site[k].pos < p) k++;
            if(k < st.n_sites && (int64_t)st.site[k].pos == p) {      /* the site's counts, unless the variant filter drops it */
                const int var = st.var && h->ycfg.min_opposite_depth > 0 && st.var[k].noff >= (uint32_t)h->ycfg.min_opposite_depth && (double)st.var[k].nvar / (double)st.var[k].noff >= h->ycfg.max_variant_frac;
                if(!var) { r->nm = (int32_t)st.site[k].nmeth; r->nu = (int32_t)st.site[k].nunmeth; }
            }
        }
        if(h->n_ych == h->cap_ych) { h->cap_ych = h->cap_ych ? 2 * h->cap_ych : 64; h->ych = realloc(h->ych, sizeof(struct ychunk) * (size_t)h->cap_ych); if(!h->ych) return MDK_ERR_NOMEM; }
        h->ych[h->n_ych++] = c;
    }
    return 0;
}
static int ychunk_cmp(const void *a, const void *b) { const struct ychunk *x = a, *y = b; return x->key < y->key ? -1 : x->key > y->key; }
int md_dev_cytosines_finish(md_dev *h, md_cytosines_set **out) {
    md_cytosines_set *r; int64_t n = 0, o = 0, k; int i;
    if(!h || !out || !h->cyto_on) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_cytosines_finish"); return MDK_ERR_ARG; }
    qsort(h->ych, (size_t)h->n_ych, sizeof(struct ychunk), ychunk_cmp);
    for(i = 0; i < h->n_ych; i++) n += h->ych[i].n;
    if(!(r = calloc(1, sizeof(*r)))) return MDK_ERR_NOMEM;
    r->n = n; r->contig = malloc(4 * (size_t)(n + 1)); r->pos = malloc(4 * (size_t)(n + 1)); r->nm = malloc(4 * (size_t)(n + 1)); r->nu = malloc(4 * (size_t)(n + 1));
    r->strand = malloc((size_t)n + 1); r->ctx = malloc((size_t)n + 1); r->tri = malloc(3 * (size_t)n + 1);
    for(i = 0; i < h->n_ych; i++) for(k = 0; k < h->ych[i].n; k++, o++) {
        const yrow_t *x = &h->ych[i].row[k];
        r->contig[o] = h->ych[i].tid; r->pos[o] = x->pos; r->nm[o] = x->nm; r->nu[o] = x->nu; r->strand[o] = x->strand; r->ctx[o] = x->ctx; memcpy(r->tri + 3 * o, x->tri, 3);
    }
    cyto_drop(h);
    *out = r;
    return 0;
}
int64_t md_cytosines_set_count(const md_cytosines_set *c) { return c ? c->n : MDK_ERR_ARG; }
int md_cytosines_set_copy(const md_cytosines_set *c, const md_cytosines_cols *d, int to_host) {
    const size_t n = c ? (size_t)c->n : 0; (void)to_host;      /* ("device" memory is host memory here) */
    if(!c || !d) return MDK_ERR_ARG;
    if(d->contig) memcpy(d->contig, c->contig, 4 * n);
    if(d->pos) memcpy(d->pos, c->pos, 4 * n);
    if(d->strand) memcpy(d->strand, c->strand, n);
    if(d->nmeth) memcpy(d->nmeth, c->nm, 4 * n);
    if(d->nunmeth) memcpy(d->nunmeth, c->nu, 4 * n);
    if(d->context) memcpy(d->context, c->ctx, n);
    if(d->trinucleotide) memcpy(d->trinucleotide, c->tri, 3 * n);
    return 0;
}
void md_cytosines_set_free(md_cytosines_set *c) { if(!c) return; free(c->contig); free(c->pos); free(c->nm); free(c->nu); free(c->strand); free(c->ctx); free(c->tri); free(c); }

/* ---- perRead: the device's selection of a chunk's reads (perRead.c:178-183, k_prep_scan_ordered) restated over the uploaded records; the
 * counts (k_perread_raw's) are taken in order from the oracle's `perRead` output for the same command line (MDK_STANDIN_PERREAD), and each
 * kept read's name and position must be the line's ---- */
typedef struct { char *name; int32_t pos; uint32_t nm, nu; } prline_t;
static prline_t *g_pr; static int64_t g_npr; static pthread_once_t g_pr_once = PTHREAD_ONCE_INIT;
static void load_perread(void) {
    const char *fn = getenv("MDK_STANDIN_PERREAD"); FILE *f = fn ? fopen(fn, "r") : NULL; char line[4096]; int64_t cap = 0;
    if(!f) return;
    while(fgets(line, sizeof line, f)) {
        char *t[5]; int k = 0; char *q = line;
        for(k = 0; k < 5; k++) { t[k] = strsep(&q, "\t\n"); if(!t[k]) break; }
        if(k < 5) continue;
        if(g_npr == cap) { cap = cap ? 2 * cap : 1 << 14; g_pr = realloc(g_pr, sizeof(prline_t) * (size_t)cap); if(!g_pr) abort(); }
        { const uint32_t tot = (uint32_t)strtoul(t[4], NULL, 10); const double pct = strtod(t[3], NULL); const uint32_t m = (uint32_t)(pct * tot / 100.0 + 0.5);
          g_pr[g_npr].name = strdup(t[0]); g_pr[g_npr].pos = (int32_t)strtol(t[2], NULL, 10); g_pr[g_npr].nm = m; g_pr[g_npr].nu = tot - m; g_npr++; }
    }
    fclose(f);
}
int md_dev_perread_submit_raw(md_dev *h, int slot, const md_raw_batch *b) {
    sslot *s = slot_of(h, slot); prslot_t *q; uint32_t i; int rc;
    pthread_once(&g_pr_once, load_perread);
    if(!s || !b) return MDK_ERR_ARG;
    if(!h->prep.perread) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_set_prep with perread first"); return MDK_ERR_ARG; }
    if(!h->pr && !(h->pr = calloc((size_t)h->n_slots, sizeof(prslot_t)))) return MDK_ERR_NOMEM;
    if((rc = md_dev_upload_raw(h, slot, b)) != 0) return rc;
    q = &h->pr[slot]; q->n = 0; q->pending = 1;
    if(q->cap < (int64_t)s->n_rec + 1) { free(q->kept); free(q->cnt); q->cap = (int64_t)s->n_rec + 1024; q->kept = malloc(sizeof(uint32_t) * (size_t)q->cap); q->cnt = malloc(sizeof(md_pr_count) * (size_t)q->cap); if(!q->kept || !q->cnt) return MDK_ERR_NOMEM; }
    for(i = 0; i < s->n_rec; i++) {
        const uint8_t *r = s->raw + s->off[i] + 4; int32_t pos; uint16_t flag; const uint8_t mapq = r[9], lqn = r[8]; const prline_t *L; size_t nl;
        memcpy(&pos, r + 4, 4); memcpy(&flag, r + 14, 2);
        if((int64_t)pos < b->beg || (int64_t)pos >= b->end) continue;
        if(h->prep.require_flags && (h->prep.require_flags & flag) != h->prep.require_flags) continue;
        if(h->prep.ignore_flags && (h->prep.ignore_flags & flag) != 0) continue;
        if((int)mapq < h->prep.min_mapq) continue;
        if(h->pr_next >= g_npr) { snprintf(t_err, sizeof t_err, "dev_standin: kept read %lld is past the oracle's perRead lines", (long long)h->pr_next); return MDK_ERR_ARG; }
        L = &g_pr[h->pr_next++]; nl = strnlen((const char *)r + 32, lqn);
        if((int32_t)L->pos != pos || strlen(L->name) != nl || memcmp(L->name, r + 32, nl)) { snprintf(t_err, sizeof t_err, "dev_standin: kept read %.60s at %d, the oracle's line is %.60s at %d", (const char *)r + 32, pos, L->name, L->pos); return MDK_ERR_ARG; }
        q->kept[q->n] = i; q->cnt[q->n].nmeth = L->nm; q->cnt[q->n].nunmeth = L->nu; q->n++;
    }
    return 0;
}
int md_dev_perread_download_raw(md_dev *h, int slot, const uint32_t **kept, const md_pr_count **counts, int64_t *n) {
    if(!slot_of(h, slot) || !h->pr || !h->pr[slot].pending || !kept || !counts || !n) { snprintf(t_err, sizeof t_err, "dev_standin: nothing submitted on this slot"); return MDK_ERR_ARG; }
    *kept = h->pr[slot].kept; *counts = h->pr[slot].cnt; *n = h->pr[slot].n;
    return 0;
}

/* ---- reads on the "device": the rows of csrc/mdk_reads.hip, in host memory ---- */
struct md_reads_set { int64_t n, nb; int32_t *contig, *pos, *nm, *nu; int64_t *off; uint8_t *bytes; };
int md_dev_reads_begin(md_dev *h) { if(!h) return MDK_ERR_ARG; reads_drop(h); h->reads_on = 1; h->pr_next = 0; return 0; }
int md_dev_reads_slot(md_dev *h, int slot) { if(!slot_of(h, slot) || !h->reads_on || !h->pr || !h->pr[slot].pending) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_reads_slot"); return MDK_ERR_ARG; } return 0; }
static int reads_room(md_dev *h, int64_t n, int64_t nb) {
    if(h->r_n + n + 1 > h->r_cap) {
        const int64_t c = 2 * (h->r_n + n + 1) + 1024;
        h->r_contig = realloc(h->r_contig, 4 * (size_t)c); h->r_pos = realloc(h->r_pos, 4 * (size_t)c); h->r_nm = realloc(h->r_nm, 4 * (size_t)c); h->r_nu = realloc(h->r_nu, 4 * (size_t)c); h->r_off = realloc(h->r_off, 8 * (size_t)c);
        if(!h->r_contig || !h->r_pos || !h->r_nm || !h->r_nu || !h->r_off) return MDK_ERR_NOMEM;
        h->r_cap = c;
    }
    if(h->r_nb + nb > h->r_capb) { const int64_t c = 2 * (h->r_nb + nb) + 4096; h->r_bytes = realloc(h->r_bytes, (size_t)c); if(!h->r_bytes) return MDK_ERR_NOMEM; h->r_capb = c; }
    if(h->r_n == 0) h->r_off[0] = 0;
    return 0;
}
static void reads_put(md_dev *h, int32_t tid, int32_t pos, uint32_t nm, uint32_t nu, const uint8_t *name, size_t nl) {
    const int64_t i = h->r_n++;
    h->r_contig[i] = tid; h->r_pos[i] = pos; h->r_nm[i] = (int32_t)nm; h->r_nu[i] = (int32_t)nu;
    memcpy(h->r_bytes + h->r_nb, name, nl); h->r_nb += (int64_t)nl; h->r_off[i + 1] = h->r_nb;
}
int md_dev_reads_collect(md_dev *h, int slot, int64_t *n) {
    sslot *s = slot_of(h, slot); prslot_t *q; int64_t i; int rc;
    if(!s || !n || !h->reads_on || !h->pr || !h->pr[slot].pending) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_reads_collect"); return MDK_ERR_ARG; }
    q = &h->pr[slot]; q->pending = 0; *n = 0;
    if((rc = reads_room(h, q->n, (int64_t)s->raw_bytes)) != 0) return rc;
    for(i = 0; i < q->n; i++) { const uint8_t *r = s->raw + s->off[q->kept[i]] + 4; int32_t pos; memcpy(&pos, r + 4, 4); reads_put(h, s->tid, pos, q->cnt[i].nmeth, q->cnt[i].nunmeth, r + 32, strnlen((const char *)r + 32, r[8])); }
    *n = q->n;
    return 0;
}
int md_dev_reads_host(md_dev *h, int32_t tid, int64_t n, const int32_t *pos, const md_pr_count *counts, const uint64_t *name_off, const uint8_t *names) {
    int64_t i; int rc;
    if(!h || !h->reads_on || n < 0 || (n && (!pos || !name_off))) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_reads_host"); return MDK_ERR_ARG; }
    if(!n) return 0;
    if((rc = reads_room(h, n, (int64_t)(name_off[n] - name_off[0]))) != 0) return rc;
    for(i = 0; i < n; i++) reads_put(h, tid, pos[i], counts ? counts[i].nmeth : 0, counts ? counts[i].nunmeth : 0, names + name_off[i], (size_t)(name_off[i + 1] - name_off[i]));
    return 0;
}
int md_dev_reads_finish(md_dev *h, md_reads_set **out) {
    md_reads_set *r; const int64_t n = h ? h->r_n : 0;
    if(!h || !out || !h->reads_on) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_reads_finish"); return MDK_ERR_ARG; }
    if(!(r = calloc(1, sizeof(*r)))) return MDK_ERR_NOMEM;
    r->n = n; r->nb = h->r_nb;
    r->contig = malloc(4 * (size_t)(n + 1)); r->pos = malloc(4 * (size_t)(n + 1)); r->nm = malloc(4 * (size_t)(n + 1)); r->nu = malloc(4 * (size_t)(n + 1)); r->off = malloc(8 * (size_t)(n + 1)); r->bytes = malloc((size_t)r->nb + 1);
    if(n) { memcpy(r->contig, h->r_contig, 4 * (size_t)n); memcpy(r->pos, h->r_pos, 4 * (size_t)n); memcpy(r->nm, h->r_nm, 4 * (size_t)n); memcpy(r->nu, h->r_nu, 4 * (size_t)n); memcpy(r->off, h->r_off, 8 * (size_t)(n + 1)); memcpy(r->bytes, h->r_bytes, (size_t)r->nb); }
    else r->off[0] = 0;
    reads_drop(h);
    *out = r;
    return 0;
}
int64_t md_reads_set_count(const md_reads_set *r) { return r ? r->n : MDK_ERR_ARG; }
int64_t md_reads_set_name_bytes(const md_reads_set *r) { return r ? r->nb : MDK_ERR_ARG; }
int md_reads_set_copy(const md_reads_set *r, const md_reads_cols *d, int to_host) {
    const size_t n = r ? (size_t)r->n : 0; (void)to_host;      /* ("device" memory is host memory here) */
    if(!r || !d) return MDK_ERR_ARG;
    if(d->contig) memcpy(d->contig, r->contig, 4 * n);
    if(d->pos) memcpy(d->pos, r->pos, 4 * n);
    if(d->nmeth) memcpy(d->nmeth, r->nm, 4 * n);
    if(d->nunmeth) memcpy(d->nunmeth, r->nu, 4 * n);
    if(d->name_off) memcpy(d->name_off, r->off, 8 * (n + 1));
    if(d->name_bytes) memcpy(d->name_bytes, r->bytes, (size_t)r->nb);
    return 0;
}
void md_reads_set_free(md_reads_set *r) { if(!r) return; free(r->contig); free(r->pos); free(r->nm); free(r->nu); free(r->off); free(r->bytes); free(r); }

/* ---- mbias: the histogram is the oracle's table for this run; the rows and the dense counts of csrc/mdk_bias.hip, in host memory ---- */
static int g_mb_run;                  /* mbias runs of the process that have submitted a chunk */
static int mbias_given(md_dev *h) {
    static const char *AB[4] = {"OT", "OB", "CTOT", "CTOB"};
    const char *dir = getenv("MDK_STANDIN_MBIAS"); char fn[4096], line[256]; FILE *f; int run;
    pthread_mutex_lock(&h->mu);
    if(h->mb_loaded) { pthread_mutex_unlock(&h->mu); return 0; }
    h->mb_loaded = 1; run = g_mb_run++;
    pthread_mutex_unlock(&h->mu);
    if(!dir) { snprintf(t_err, sizeof t_err, "dev_standin: MDK_STANDIN_MBIAS is not set"); return MDK_ERR_ARG; }
    snprintf(fn, sizeof fn, "%s/%d.txt", dir, run);
    if(!(f = fopen(fn, "r"))) { snprintf(t_err, sizeof t_err, "dev_standin: no table %.200s", fn); return MDK_ERR_ARG; }
    while(fgets(line, sizeof line, f)) {
        char ab[16]; int rd, pos, st; unsigned m, u;
        if(sscanf(line, "%15s %d %d %u %u", ab, &rd, &pos, &m, &u) != 5) continue;       /* (the header line) */
        for(st = 0; st < 4 && strcmp(ab, AB[st]); st++) ;
        if(st == 4 || rd < 1 || rd > 2 || pos < 1) { fclose(f); snprintf(t_err, sizeof t_err, "dev_standin: bad table line %.100s", line); return MDK_ERR_ARG; }
        if(pos > h->mb_len) { h->mb_hist = realloc(h->mb_hist, sizeof(uint32_t) * 16 * (size_t)pos); if(!h->mb_hist) abort(); memset(h->mb_hist + 16 * (size_t)h->mb_len, 0, sizeof(uint32_t) * 16 * (size_t)(pos - h->mb_len)); h->mb_len = pos; }
        h->mb_hist[(size_t)(pos - 1) * 16 + st * 4 + 2 * (rd - 1)] += m; h->mb_hist[(size_t)(pos - 1) * 16 + st * 4 + 2 * (rd - 1) + 1] += u;
    }
    fclose(f);
    return 0;
}
int md_dev_mbias_submit(md_dev *h, int slot, const md_read_batch *b) { int rc = md_dev_upload(h, slot, b); return rc ? rc : mbias_given(h); }
int md_dev_mbias_group(md_dev *h, const int *slots, int n) {
    int i;
    if(!h || !slots || n < 1 || n > 8 || !h->prep.no_pairing) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_mbias_group"); return MDK_ERR_ARG; }
    for(i = 0; i < n; i++) { sslot *s = slot_of(h, slots[i]); if(!s || !s->used || s->launched) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_mbias_group: slot not freshly uploaded"); return MDK_ERR_ARG; } s->launched = 1; }
    return mbias_given(h);
}
int md_dev_mbias_collect(md_dev *h, const int *slots, int n, int *rc) {
    int i;
    if(!h || !slots || !rc || n < 1) return MDK_ERR_ARG;
    for(i = 0; i < n; i++) {
        sslot *s = slot_of(h, slots[i]);
        if(!s || !s->launched) { snprintf(t_err, sizeof t_err, "dev_standin: md_dev_mbias_collect: slot not launched"); return MDK_ERR_ARG; }
        s->launched = 0; rc[i] = 0;
        if(s->handed_back) { s->handed_back = 0; snprintf(t_err, sizeof t_err, "dev_standin: this chunk goes back to the host preparation"); rc[i] = MDK_ERR_PREP_HOST; }
    }
    return 0;
}
int md_dev_mbias_redone(const md_dev *h) { (void)h; return 0; }
struct md_bias_set { int64_t n; int len; int8_t *strand, *read; int32_t *pos; int64_t *nm, *nu, *dense; uint32_t *hist; };
int md_dev_bias_finish(md_dev *h, md_bias_set **out) {
    md_bias_set *b; int st, q, r; const int len = h ? h->mb_len : 0; const size_t cap = 8 * (size_t)len + 1;
    if(!h || !out) return MDK_ERR_ARG;
    if(!(b = calloc(1, sizeof(*b)))) return MDK_ERR_NOMEM;
    b->len = len; b->strand = malloc(cap); b->read = malloc(cap); b->pos = malloc(4 * cap); b->nm = malloc(8 * cap); b->nu = malloc(8 * cap); b->dense = malloc(8 * 2 * cap); b->hist = calloc(2 * cap, 4);
    for(q = 0; q < 16 * len; q++) { b->hist[q] = h->mb_hist[q]; b->dense[q] = (int64_t)h->mb_hist[q]; }
    /* the order the command prints: strand, then position, then read; a row only where it has a call */
    for(st = 0; st < 4; st++) for(q = 0; q < len; q++) for(r = 0; r < 2; r++) {
        const uint32_t m = h->mb_hist[(size_t)q * 16 + st * 4 + 2 * r], u = h->mb_hist[(size_t)q * 16 + st * 4 + 2 * r + 1];
        if(!m && !u) continue;
        b->strand[b->n] = (int8_t)st; b->read[b->n] = (int8_t)(r + 1); b->pos[b->n] = q + 1; b->nm[b->n] = m; b->nu[b->n] = u; b->n++;
    }
    h->mb_loaded = 0;                 /* the next run's table is the next file (its histogram starts empty: md_dev_reset) */
    *out = b;
    return 0;
}
int64_t md_bias_set_count(const md_bias_set *b) { return b ? b->n : MDK_ERR_ARG; }
int md_bias_set_len(const md_bias_set *b) { return b ? b->len : MDK_ERR_ARG; }
int md_bias_set_redone(const md_bias_set *b) { (void)b; return 0; }
int md_bias_set_hist(const md_bias_set *b, md_mbias *out) { if(!b || !out) return MDK_ERR_ARG; out->len = b->len; out->count = b->hist; return 0; }
int md_bias_set_copy(const md_bias_set *b, int column, void *dst, int to_host) {
    const size_t n = b ? (size_t)b->n : 0; (void)to_host;
    if(!b || !dst) return MDK_ERR_ARG;
    switch(column) {
    case MD_BIAS_STRAND: memcpy(dst, b->strand, n); break;
    case MD_BIAS_READ: memcpy(dst, b->read, n); break;
    case MD_BIAS_POS: memcpy(dst, b->pos, 4 * n); break;
    case MD_BIAS_NMETH: memcpy(dst, b->nm, 8 * n); break;
    case MD_BIAS_NUNMETH: memcpy(dst, b->nu, 8 * n); break;
    case MD_BIAS_COUNTS: memcpy(dst, b->dense, 8 * 16 * (size_t)b->len); break;
    default: return MDK_ERR_ARG;
    }
    return 0;
}
void md_bias_set_free(md_bias_set *b) { if(!b) return; free(b->strand); free(b->read); free(b->pos); free(b->nm); free(b->nu); free(b->dense); free(b->hist); free(b); }
