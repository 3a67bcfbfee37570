// mdk_calls.hip -- the final calls of `extract` as device-resident columns (include/mdk_hip.h, "calls on the device").
//
// What emit_format (csrc/host/mdk_emit.c:72-121) does to a chunk's sites on the host -- the variant filter, --mergeContext, the
// depth test and the contexts switched on -- done by k_calls_compact on the sites the pileup left in the slot (md_tile_seg /
// md_site / md_site_var), for the chunks of one group.  No per-site data crosses to the host.
//
// Order.  A tile's sites are ascending, tiles are in position order, but a tile's segment lies wherever its atomic reservation put
// it.  The host reserves, per chunk, as many rows as the chunk has site slots in use (an upper bound on its rows) in a row arena;
// workgroup (chunk, tile t) writes its rows at the chunk's reservation + the site count of tiles 0..t-1, i.e. each tile into a
// window as long as its own site count, and notes how many it wrote in a tile table.  md_dev_calls_finish closes the gaps with one
// gather pass (k_calls_gather) over the tiles of every chunk, the chunks ordered by the key the caller gave them (schedule order).
#include "mdk_hip_internal.hpp"
#include <algorithm>

#define CALLS_WG 256

struct CallsTile { uint64_t src; uint32_t n, pad; };              // rows of a tile: arena index of the first, count (written by the kernel)
struct CallsChunk { uint32_t key; int32_t tid; uint64_t tile0; int32_t ntiles; };    // a compacted chunk: its tiles are tiles[tile0 .. tile0 + ntiles)
// columns of the row arena, of the tile table and of a result set (md_calls_cols' order)
enum { A_START = 0, A_END, A_NM, A_NU, A_CTX, A_STRAND };
static const ColSpec ARENA_COLS[] = {{4, 0}, {4, 0}, {4, 0}, {4, 0}, {1, 0}, {1, 0}};
static const ColSpec TILE_COLS[] = {{sizeof(CallsTile), 0}};
enum { R_CONTIG = 0, R_START, R_END, R_NM, R_NU, R_CTX, R_STRAND };
static const ColSpec SET_COLS[] = {{4, 0}, {4, 0}, {4, 0}, {4, 0}, {4, 0}, {1, 0}, {1, 0}};
struct CallsState {
    md_calls_cfg cfg; bool on = false;
    TableLane lane;                                          // the compactions run here
    ColTable rows{ARENA_COLS, 6, "hipMalloc(call arena)"}; uint64_t used_rows = 0;       // kept across runs
    ColTable tiles{TILE_COLS, 1, "hipMalloc(call tiles)"}; uint64_t used_tiles = 0;
    uint32_t *d_err = nullptr;
    std::vector<CallsChunk> chunks;
};

struct md_calls_set { int device = 0; int64_t n = 0; ColTable cols{SET_COLS, 7, "hipMalloc(calls)"}; };

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
struct KCallsSlot { const md_site *site; const md_site_var *var; const md_tile_seg *seg; uint64_t row_base, tile_base; uint32_t reserved, site_cap; int ntiles; };
struct KCalls {
    int n; int tstart[MAXM + 1]; KCallsSlot S[MAXM];
    int32_t min_depth, merge, min_opp, ctx_mask; double max_vf;
    int32_t *start, *end, *nm, *nu; uint8_t *ctx; int8_t *strand; CallsTile *tiles; uint32_t *err;
};

// the site at index i + delta of the chunk's ascending order, where i indexes tile t's run; false past either end of the chunk
__device__ __forceinline__ bool calls_nbr(const KCallsSlot &S, int t, int i, int delta, md_site &o, md_site_var &ov) {
    int k = i + delta;
    for(int guard = 0; guard < S.ntiles + 1; guard++) {
        if(k < 0) { if(--t < 0) return false; k += (int)S.seg[t].cnt; continue; }
        const md_tile_seg g = S.seg[t];
        if(k >= (int)g.cnt) { k -= (int)g.cnt; if(++t >= S.ntiles) return false; continue; }
        if((uint64_t)g.off + g.cnt > S.site_cap) return false;
        o = S.site[g.off + k]; ov.noff = ov.nvar = 0; if(S.var) ov = S.var[g.off + k];
        return true;
    }
    return false;
}
// the variant filter (site_is_variant, mdk_hip_internal.hpp) with this launch's thresholds
__device__ __forceinline__ bool calls_variant(const KCalls &K, bool has_var, const md_site_var &v) { return site_is_variant(K.min_opp, K.max_vf, has_var, v); }

__global__ __launch_bounds__(CALLS_WG) void k_calls_compact(const KCalls K) {
    const int b = blockIdx.x;
    if(b >= K.tstart[K.n]) return;
    int j = 0;
    while(j + 1 < K.n && b >= K.tstart[j + 1]) j++;
    const KCallsSlot &S = K.S[j];
    const int t = b - K.tstart[j], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ uint64_t red[CALLS_WG / 64];
    __shared__ uint32_t wcnt[CALLS_WG / 64];
    // where this tile's window starts: the site counts of the tiles before it
    uint64_t pre = 0;
    for(int u = tid; u < t; u += CALLS_WG) pre += S.seg[u].cnt;
    for(int o = 32; o > 0; o >>= 1) pre += __shfl_xor(pre, o, 64);
    if(lane == 0) red[wave] = pre;
    __syncthreads();
    pre = 0;
    for(int w = 0; w < CALLS_WG / 64; w++) pre += red[w];
    const md_tile_seg me = S.seg[t];
    if((uint64_t)me.off + me.cnt > S.site_cap || pre + me.cnt > S.reserved) {      // inconsistent tile table: nothing is written, the host is told
        if(tid == 0) { atomicOr(K.err, 1u); CallsTile e; e.src = S.row_base; e.n = 0; e.pad = 0; K.tiles[S.tile_base + t] = e; }
        return;
    }
    const bool has_var = S.var != nullptr;
    const uint64_t base = S.row_base + pre;
    uint32_t written = 0;
    for(uint32_t r0 = 0; r0 < me.cnt; r0 += CALLS_WG) {
        const int i = (int)(r0 + tid);
        bool has = false; int32_t rs = 0, re = 0; uint32_t m = 0, u = 0; int type = 0, strand = 0;
        if(i < (int)me.cnt) {
            const md_site s = S.site[me.off + i];
            md_site_var v; v.noff = v.nvar = 0; if(has_var) v = S.var[me.off + i];
            type = (s.meta >> 1) & 3; const bool is_g = s.meta & 1;
            const bool surv = !calls_variant(K, has_var, v) && s.nmeth + s.nunmeth > 0;
            if((K.ctx_mask >> type) & 1) {
                if(!K.merge || type == 2) {
                    if(surv) { has = true; rs = (int32_t)s.pos; re = rs + 1; m = s.nmeth; u = s.nunmeth; strand = is_g ? -1 : 1; }
                } else {
                    const int d = type + 1;      // CpG: the G is one past the C, CHG: two
                    if(!is_g) {                  // a C: it owns its key's row
                        bool sg = false, vg = false; md_site g; md_site_var gv;
                        for(int k = 1; k <= d; k++)
                            if(calls_nbr(S, t, i, k, g, gv) && g.pos == s.pos + (uint32_t)d && (g.meta & 1) && (int)((g.meta >> 1) & 3) == type) {
                                vg = calls_variant(K, has_var, gv); sg = !vg && g.nmeth + g.nunmeth > 0; break;
                            }
                        if(surv || sg) {
                            has = true; rs = (int32_t)s.pos; re = rs + d + 1;
                            m = (surv ? s.nmeth : 0) + (sg ? g.nmeth : 0); u = (surv ? s.nunmeth : 0) + (sg ? g.nunmeth : 0);
                            if(surv && vg) m = u = 0;      // the C's counts are zeroed by a variant G (mdk_emit.c:86-88): the row fails the depth test
                        }
                    } else {                     // a G: its row, unless the C of its key is a site of the chunk (which owns it)
                        bool c_here = false; md_site c; md_site_var cv;
                        if(s.pos >= (uint32_t)d)
                            for(int k = 1; k <= d; k++)
                                if(calls_nbr(S, t, i, -k, c, cv) && c.pos == s.pos - (uint32_t)d && !(c.meta & 1) && (int)((c.meta >> 1) & 3) == type) { c_here = true; break; }
                        if(!c_here && surv) { has = true; rs = (int32_t)s.pos - d; re = (int32_t)s.pos + 1; m = s.nmeth; u = s.nunmeth; }
                    }
                }
            }
            if(has && (m + u == 0 || m + u < (uint32_t)K.min_depth)) has = false;
        }
        // exclusive scan of `has` over the workgroup: ballot per wave, wave totals in LDS
        const uint64_t bal = __ballot(has);
        const uint32_t below = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if(lane == 0) wcnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = below, tot = 0;
        for(int w = 0; w < CALLS_WG / 64; w++) { if(w < wave) off += wcnt[w]; tot += wcnt[w]; }
        if(has) {
            const uint64_t o = base + written + off;
            K.start[o] = rs; K.end[o] = re; K.nm[o] = (int32_t)m; K.nu[o] = (int32_t)u; K.ctx[o] = (uint8_t)type; K.strand[o] = (int8_t)strand;
        }
        written += tot;
        __syncthreads();                 // (wcnt is rewritten by the next round)
    }
    if(tid == 0) { CallsTile e; e.src = base; e.n = written; e.pad = 0; K.tiles[S.tile_base + t] = e; }
}

// rows of tile e: src .. src + n of the arena to dst .. dst + n of the result, with the chunk's contig
struct GatherEnt { uint64_t src, dst; uint32_t n; int32_t tid; };
struct KGather {
    const GatherEnt *ent; uint64_t n_ent;
    const int32_t *start, *end, *nm, *nu; const uint8_t *ctx; const int8_t *strand;
    int32_t *o_contig, *o_start, *o_end, *o_nm, *o_nu; uint8_t *o_ctx; int8_t *o_strand;
};
__global__ __launch_bounds__(CALLS_WG) void k_calls_gather(const KGather G) {
    for(uint64_t e = blockIdx.x; e < G.n_ent; e += gridDim.x) {
        const GatherEnt g = G.ent[e];
        for(uint32_t i = threadIdx.x; i < g.n; i += CALLS_WG) {
            const uint64_t s = g.src + i, d = g.dst + i;
            G.o_contig[d] = g.tid; G.o_start[d] = G.start[s]; G.o_end[d] = G.end[s]; G.o_nm[d] = G.nm[s]; G.o_nu[d] = G.nu[s];
            G.o_ctx[d] = G.ctx[s]; G.o_strand[d] = G.strand[s];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
void calls_state_free(md_dev *h) {
    CallsState *c = h->calls; if(!c) return;
    c->lane.close();
    c->rows.release(); c->tiles.release();
    if(c->d_err) (void)hipFree(c->d_err);
    delete c; h->calls = nullptr;
}

extern "C" int md_dev_calls_begin(md_dev *h, const md_calls_cfg *cfg) {
    if(!h || !cfg || cfg->min_depth < 1) return fail(MDK_ERR_ARG, "md_dev_calls_begin", hipSuccess);
    HIPCHK(hipSetDevice(h->device));
    if(!h->calls) h->calls = new CallsState();
    CallsState *c = h->calls;
    { const int rc = c->lane.open(h->device); if(rc) return rc; }
    if(!c->d_err) HIPCHK(hipMalloc((void **)&c->d_err, sizeof(uint32_t)));
    HIPCHK(hipMemsetAsync(c->d_err, 0, sizeof(uint32_t), c->lane.st));
    c->cfg = *cfg; c->on = true; c->used_rows = 0; c->used_tiles = 0; c->chunks.clear();
    h->no_pack = true;            // group launches stop copying their sites to pinned host memory: nobody downloads them
    return 0;
}

extern "C" int md_dev_calls_group(md_dev *h, const int *slots, const uint32_t *keys, int n, int *rcs) {
    if(!h || !slots || !keys || !rcs || n < 1 || n > MAXM || !h->calls || !h->calls->on) return fail(MDK_ERR_ARG, "md_dev_calls_group", hipSuccess);
    HIPCHK(hipSetDevice(h->device));
    CallsState *c = h->calls;
    // wait for the group as md_dev_download_group does (one copy of the status blocks when the slots shared one launch)
    int lo = 0x7fffffff, hi = -1; hipStream_t st = nullptr; Slot *ss[MAXM]; int64_t cnt[MAXM];
    for(int i = 0; i < n; i++) {
        Slot *s = get_slot(h, slots[i]); if(!s || !s->launched) return fail(MDK_ERR_ARG, "md_dev_calls_group: slot not launched", hipSuccess);
        ss[i] = s; rcs[i] = 0;
        if(i == 0) st = s->run; else if(s->run != st) st = nullptr;
        lo = std::min(lo, s->index); hi = std::max(hi, s->index);
    }
    if(st) {
        ProfScope pf(PF_FIN_WAIT);
        HIPCHK(hipMemcpyAsync(h->h_status.p + lo, h->d_status.p + lo, sizeof(SlotStatus) * (size_t)(hi - lo + 1), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for(int i = 0; i < n; i++) { cnt[i] = finish_eval(h, ss[i]); if(cnt[i] < 0) rcs[i] = (int)cnt[i]; }
    } else
        for(int i = 0; i < n; i++) { cnt[i] = finish_count(h, ss[i]); if(cnt[i] < 0) rcs[i] = (int)cnt[i]; }
    for(int i = 0; i < n; i++) if(!rcs[i]) HIPCHK(hipStreamSynchronize(ss[i]->run ? ss[i]->run : ss[i]->stream));     // (a chunk prepared and piled up again inside finish_eval)
    uint64_t rows = 0, tiles = 0;
    for(int i = 0; i < n; i++) if(!rcs[i]) { rows += (uint64_t)cnt[i]; tiles += (uint64_t)std::max(ss[i]->ntiles, 0); }
    // room for the group's rows and tiles (growing copies what is there, behind every compaction queued so far)
    { int rc = c->rows.reserve(c->used_rows, rows, CALLS_ROWS_FLOOR, c->lane.st); if(!rc) rc = c->tiles.reserve(c->used_tiles, tiles, CALLS_TILES_FLOOR, c->lane.st); if(rc) return rc; }
    KCalls K; memset(&K, 0, sizeof(K));
    K.min_depth = c->cfg.min_depth; K.merge = c->cfg.merge; K.min_opp = c->cfg.min_opposite_depth; K.max_vf = c->cfg.max_variant_frac;
    K.ctx_mask = (c->cfg.ctx_on[0] ? 1 : 0) | (c->cfg.ctx_on[1] ? 2 : 0) | (c->cfg.ctx_on[2] ? 4 : 0);
    K.start = c->rows.col<int32_t>(A_START); K.end = c->rows.col<int32_t>(A_END); K.nm = c->rows.col<int32_t>(A_NM); K.nu = c->rows.col<int32_t>(A_NU);
    K.ctx = c->rows.col<uint8_t>(A_CTX); K.strand = c->rows.col<int8_t>(A_STRAND); K.tiles = c->tiles.col<CallsTile>(0); K.err = c->d_err;
    int total = 0;
    for(int i = 0; i < n; i++) {
        Slot *s = ss[i];
        if(rcs[i]) continue;
        const int nt = std::max(s->ntiles, 0);
        if(cnt[i] > 0xfffffff0ll) { rcs[i] = fail(MDK_ERR_ARG, "md_dev_calls_group: chunk too large", hipSuccess); continue; }
        CallsChunk ch; ch.key = keys[i]; ch.tid = s->tid; ch.tile0 = c->used_tiles; ch.ntiles = cnt[i] > 0 ? nt : 0;
        c->chunks.push_back(ch);
        if(cnt[i] <= 0 || nt == 0) continue;
        KCallsSlot &S = K.S[K.n];
        S.site = s->b_site ? s->b_site : s->d_site.p; S.var = h->variant ? (s->b_site ? s->b_var : s->d_var.p) : nullptr; S.seg = s->b_site ? s->b_seg : s->d_seg.p;
        S.row_base = c->used_rows; S.tile_base = c->used_tiles; S.reserved = (uint32_t)cnt[i];
        S.site_cap = (uint32_t)std::min<int64_t>(cnt[i], 0xfffffff0ll); S.ntiles = nt;
        K.tstart[K.n] = total; total += nt; K.n++;
        c->used_rows += (uint64_t)cnt[i]; c->used_tiles += (uint64_t)nt;
    }
    K.tstart[K.n] = total;
    if(total > 0) {
        hipLaunchKernelGGL(k_calls_compact, dim3((unsigned)total), dim3(CALLS_WG), 0, c->lane.st, K);
        HIPCHK(hipGetLastError());
    }
    // the slots' next uploads and launches come after the compaction has read their sites
    { const int rc = c->lane.fence(ss, n); if(rc) return rc; }
    for(int i = 0; i < n; i++) ss[i]->busy = false;
    return 0;
}

extern "C" int md_dev_calls_finish(md_dev *h, md_calls_set **out) {
    if(!h || !out || !h->calls || !h->calls->on) return fail(MDK_ERR_ARG, "md_dev_calls_finish", hipSuccess);
    *out = nullptr;
    HIPCHK(hipSetDevice(h->device));
    CallsState *c = h->calls;
    hipStream_t st = c->lane.st;
    HIPCHK(hipStreamSynchronize(st));
    uint32_t err = 0;
    HIPCHK(hipMemcpy(&err, c->d_err, sizeof(err), hipMemcpyDeviceToHost));
    if(err) return fail(MDK_ERR_ARG, "md_dev_calls_finish: inconsistent tile segments", hipSuccess);
    std::vector<CallsTile> tt((size_t)c->used_tiles);
    if(c->used_tiles) { const int rc = c->tiles.copy_out(0, c->used_tiles, tt.data(), hipMemcpyDeviceToHost); if(rc) return rc; }
    std::vector<CallsChunk> ch = c->chunks;
    std::stable_sort(ch.begin(), ch.end(), [](const CallsChunk &a, const CallsChunk &b) { return a.key < b.key; });
    std::vector<GatherEnt> ge; uint64_t n = 0;
    for(const CallsChunk &k : ch)
        for(int t = 0; t < k.ntiles; t++) {
            const CallsTile &e = tt[(size_t)(k.tile0 + (uint64_t)t)];
            if(!e.n) continue;
            if(e.src + e.n > c->used_rows) return fail(MDK_ERR_ARG, "md_dev_calls_finish: a tile's rows lie outside the arena", hipSuccess);
            GatherEnt g; g.src = e.src; g.dst = n; g.n = e.n; g.tid = k.tid; ge.push_back(g); n += e.n;
        }
    md_calls_set *r = new md_calls_set(); r->device = h->device; r->n = (int64_t)n;
    { const int rc = r->cols.reserve(0, n + 64, 0, st); if(rc) { delete r; return rc; } }
    if(!ge.empty()) {
        GatherEnt *d_ge = nullptr;
        hipError_t e = hipMalloc((void **)&d_ge, sizeof(GatherEnt) * ge.size());
        if(e == hipSuccess) e = hipMemcpyAsync(d_ge, ge.data(), sizeof(GatherEnt) * ge.size(), hipMemcpyHostToDevice, st);
        if(e == hipSuccess) {
            const ColTable &a = c->rows, &o = r->cols;
            KGather G; G.ent = d_ge; G.n_ent = ge.size();
            G.start = a.col<int32_t>(A_START); G.end = a.col<int32_t>(A_END); G.nm = a.col<int32_t>(A_NM); G.nu = a.col<int32_t>(A_NU);
            G.ctx = a.col<uint8_t>(A_CTX); G.strand = a.col<int8_t>(A_STRAND);
            G.o_contig = o.col<int32_t>(R_CONTIG); G.o_start = o.col<int32_t>(R_START); G.o_end = o.col<int32_t>(R_END); G.o_nm = o.col<int32_t>(R_NM);
            G.o_nu = o.col<int32_t>(R_NU); G.o_ctx = o.col<uint8_t>(R_CTX); G.o_strand = o.col<int8_t>(R_STRAND);
            const unsigned grid = (unsigned)std::min<size_t>(ge.size(), 65536);
            hipLaunchKernelGGL(k_calls_gather, dim3(grid), dim3(CALLS_WG), 0, st, G);
            e = hipGetLastError();
            if(e == hipSuccess) e = hipStreamSynchronize(st);
        }
        if(d_ge) (void)hipFree(d_ge);
        if(e != hipSuccess) { r->cols.release(); delete r; return fail(MDK_ERR_HIP, "k_calls_gather", e); }
    }
    c->on = false; c->used_rows = 0; c->used_tiles = 0; c->chunks.clear();
    h->no_pack = false;
    *out = r;
    return 0;
}

extern "C" int64_t md_calls_set_count(const md_calls_set *c) { return c ? c->n : MDK_ERR_ARG; }

extern "C" int md_calls_set_copy(const md_calls_set *c, const md_calls_cols *dst, int to_host) {
    if(!c || !dst) return fail(MDK_ERR_ARG, "md_calls_set_copy", hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if(!c->n) return 0;
    void *const to[] = {dst->contig, dst->start, dst->end, dst->nmeth, dst->nunmeth, dst->context, dst->strand};        // R_CONTIG .. R_STRAND
    for(int i = 0; i < 7; i++) if(to[i]) { const int rc = c->cols.copy_out(i, (uint64_t)c->n, to[i], kind); if(rc) return rc; }
    return 0;
}

extern "C" void md_calls_set_free(md_calls_set *c) {
    if(!c) return;
    (void)hipSetDevice(c->device);
    c->cols.release();
    delete c;
}
