// mdk_cytosines.hip -- the rows of `extract --cytosine_report` as device-resident columns (include/mdk_hip.h, "the cytosine report on the
// device").
//
// What emit_format and put_blanks (csrc/host/mdk_emit.c:56-120) do on the host for this format -- walk the contig's bases between the
// sites the device returned, print a row for every cytosine of a context that is switched on, with the site's counts where there is a
// site the variant filter keeps and 0 0 elsewhere -- done here from the resident BASES of the contig (h->ref; not the context codes, which
// md_dev_set_regions masks under -l: the report lists every cytosine of a chunk a BED interval touches) and the sites the pileup left in
// the slot.
//
// Sizing.  How many rows a chunk has depends on its bases alone, between 2 % (CpG only) and some 40 % (all contexts) of its length, and
// nothing the slot knows bounds it short of the chunk's length.  So the rows are counted first: k_cyto_count runs over the bases of the
// group's chunks, one workgroup per pileup tile, and leaves a count per tile and a total per chunk.  It is queued before the host waits
// for the group's pileup, so the at most eight totals are there when that wait returns; the run's arena is then reserved for exactly
// that many rows more, and k_cyto_fill -- the same tiles, the same classification -- writes tile t's rows at the chunk's reservation + the
// counts of tiles 0..t-1.  A chunk's rows are dense and in position order where they lie; md_dev_cytosines_finish copies the chunks in
// key order into a set of the exact size (k_cyto_gather).
#include "mdk_hip_internal.hpp"
#include <algorithm>

#define CYTO_WG 256
#define CYTO_TILE_MAX 2048                      // positions per tile at most (the pileup's largest tile)
#define CYTO_SRAW (CYTO_TILE_MAX + 48)          // staged bases: up to 15 bytes of alignment, the tile, two bases of halo on each side, rounded up to 16

struct CytoChunk { uint32_t key; uint64_t row0, n; };         // a filled chunk: its rows are arena rows [row0, row0 + n)
enum { Y_CONTIG = 0, Y_POS, Y_STRAND, Y_NM, Y_NU, Y_CTX, Y_TRI };
static const ColSpec CYTO_COLS[] = {{4, 0}, {4, 0}, {1, 0}, {4, 0}, {4, 0}, {1, 0}, {3, 0}};
struct CytoState {
    md_cyto_cfg cfg; bool on = false;
    TableLane lane;                                          // the counting and filling kernels run here, in order
    ColTable rows{CYTO_COLS, 7, "hipMalloc(cytosine arena)"}; uint64_t used_rows = 0;       // kept across runs
    uint32_t *d_tilecnt = nullptr; uint64_t tile_cap = 0;    // rows per tile of the group being worked on (k_cyto_count -> k_cyto_fill)
    unsigned long long *d_tot = nullptr;                     // rows per chunk of that group
    uint32_t *d_err = nullptr;
    std::vector<CytoChunk> chunks;
};
struct md_cytosines_set { int device = 0; int64_t n = 0; ColTable cols{CYTO_COLS, 7, "hipMalloc(cytosines)"}; };

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
struct KCytoChunk {
    const uint8_t *ref; int64_t reflen, beg, end; int32_t tile, ntiles, tid;
    const md_site *site; const md_site_var *var; const md_tile_seg *seg; uint32_t site_cap;      // seg == nullptr: no sites (every row 0 0)
    uint64_t row_base, total, tile_base;
};
struct KCyto {
    int n; int tstart[MAXM + 1]; KCytoChunk C[MAXM];
    int32_t min_opp, ctx_mask; double max_vf;
    uint32_t *tilecnt; unsigned long long *tot;
    int32_t *contig, *pos, *nm, *nu; int8_t *strand; uint8_t *ctx, *tri; uint32_t *err;
};

// The bases of positions [T0 - 2, T0 + span + 2) into LDS with 16-byte loads: sraw[i] is the base at (T0 - 2 - mis) + i, where mis (returned)
// is what aligns the first load; a position outside [0, reflen) reads as 0, which is no base: not a C or G, never the G or C that decides a
// context, 'N' in a trinucleotide -- the contig-end rules of k_classify and of trinuc() (mdk_emit.c) without a branch at the reader.
// The contig's array is 16-byte aligned and 16 bytes longer than the contig (md_dev_set_reference), so every load lies inside it.
__device__ __forceinline__ uint32_t cyto_keep(uint32_t w, int nb) { return nb >= 4 ? w : nb <= 0 ? 0u : (w & ((1u << (8 * nb)) - 1u)); }
__device__ __forceinline__ int cyto_stage(const uint8_t *ref, int64_t reflen, int64_t T0, int span, uint8_t *sraw) {
    const int64_t g0 = T0 - 2;
    const int mis = (int)(g0 & 15);
    const int64_t pa = g0 - mis;
    const int nvec = (mis + span + 4 + 15) >> 4;
    for(int k = threadIdx.x; k < nvec; k += CYTO_WG) {
        const int64_t q = pa + 16 * (int64_t)k;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if(q >= 0 && q < reflen) {
            v = *(const uint4 *)(ref + q);
            if(q + 16 > reflen) { const int nb = (int)(reflen - q); v.x = cyto_keep(v.x, nb); v.y = cyto_keep(v.y, nb - 4); v.z = cyto_keep(v.z, nb - 8); v.w = cyto_keep(v.w, nb - 12); }
        }
        *(uint4 *)(sraw + 16 * k) = v;
    }
    return mis;
}
// context code of the staged position at sb[j], as k_classify's (mdk_hip.hip): 0 = not C/G, else 1 + 2 * type + isG
__device__ __forceinline__ int cyto_code(const uint8_t *sb, int j) {
    const int c = sb[j] & 0x5f;
    if(c == 'C') return ((sb[j + 1] & 0x5f) == 'G') ? 1 : ((sb[j + 2] & 0x5f) == 'G') ? 3 : 5;
    if(c == 'G') return ((sb[j - 1] & 0x5f) == 'C') ? 2 : ((sb[j - 2] & 0x5f) == 'C') ? 4 : 6;
    return 0;
}
// a letter of the trinucleotide (extract.c:120-180 as trinuc() in mdk_emit.c restates it): after a C the base folded to upper case, before
// a G its complement; what is not one of ACGT is N
__device__ __forceinline__ uint8_t cyto_fwd(uint8_t b) { b &= 0x5f; return (b == 'A' || b == 'C' || b == 'G' || b == 'T') ? b : (uint8_t)'N'; }
__device__ __forceinline__ uint8_t cyto_comp(uint8_t b) {
    switch(b) { case 'A': case 'a': return 'T'; case 'C': case 'c': return 'G'; case 'G': case 'g': return 'C'; case 'T': case 't': return 'A'; default: return 'N'; }
}
// the chunk and the tile of workgroup b; false: past the launch's last tile
__device__ __forceinline__ bool cyto_where(const KCyto &K, int b, int &j, int &t) {
    if(b >= K.tstart[K.n]) return false;
    j = 0;
    while(j + 1 < K.n && b >= K.tstart[j + 1]) j++;
    t = b - K.tstart[j];
    return true;
}

__global__ __launch_bounds__(CYTO_WG) void k_cyto_count(const KCyto K) {
    int j, t;
    if(!cyto_where(K, blockIdx.x, j, t)) return;
    const KCytoChunk &S = K.C[j];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ __align__(16) uint8_t sraw[CYTO_SRAW];
    __shared__ uint32_t wcnt[CYTO_WG / 64];
    const int64_t T0 = S.beg + (int64_t)t * S.tile;
    const int span = (int)((S.end - T0 < (int64_t)S.tile) ? S.end - T0 : (int64_t)S.tile);
    const uint8_t *sb = sraw + cyto_stage(S.ref, S.reflen, T0, span, sraw);          // sb[i + 2]: the base at T0 + i
    __syncthreads();
    uint32_t cnt = 0;
    for(int i = tid; i < span; i += CYTO_WG) { const int code = cyto_code(sb, i + 2); if(code && ((K.ctx_mask >> ((code - 1) >> 1)) & 1)) cnt++; }
    for(int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if(lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    if(tid == 0) {
        uint32_t tot = 0;
        for(int w = 0; w < CYTO_WG / 64; w++) tot += wcnt[w];
        K.tilecnt[S.tile_base + t] = tot;
        if(tot) atomicAdd(&K.tot[j], (unsigned long long)tot);
    }
}

__global__ __launch_bounds__(CYTO_WG) void k_cyto_fill(const KCyto K) {
    int j, t;
    if(!cyto_where(K, blockIdx.x, j, t)) return;
    const KCytoChunk &S = K.C[j];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ __align__(16) uint8_t sraw[CYTO_SRAW];
    __shared__ uint32_t nm[CYTO_TILE_MAX], nu[CYTO_TILE_MAX];
    __shared__ uint64_t red[CYTO_WG / 64];
    __shared__ uint32_t wcnt[CYTO_WG / 64];
    const int64_t T0 = S.beg + (int64_t)t * S.tile;
    const int span = (int)((S.end - T0 < (int64_t)S.tile) ? S.end - T0 : (int64_t)S.tile);
    // where this tile's rows start: the counts of the tiles before it
    uint64_t pre = 0;
    for(int u = tid; u < t; u += CYTO_WG) pre += K.tilecnt[S.tile_base + u];
    for(int o = 32; o > 0; o >>= 1) pre += __shfl_xor(pre, o, 64);
    if(lane == 0) red[wave] = pre;
    for(int i = tid; i < span; i += CYTO_WG) { nm[i] = 0; nu[i] = 0; }
    const uint8_t *sb = sraw + cyto_stage(S.ref, S.reflen, T0, span, sraw);
    __syncthreads();
    pre = 0;
    for(int w = 0; w < CYTO_WG / 64; w++) pre += red[w];
    const uint32_t mine = K.tilecnt[S.tile_base + t];
    if(pre + mine > S.total) { if(tid == 0) atomicOr(K.err, 2u); return; }      // the counts do not add up to the reservation: nothing is written, the host is told
    // the counts of the tile's sites, at their positions; a site the variant filter drops leaves its zeros (mdk_emit.c:82-91)
    if(S.seg) {
        const md_tile_seg me = S.seg[t];
        if((uint64_t)me.off + me.cnt > S.site_cap) { if(tid == 0) atomicOr(K.err, 1u); }
        else
            for(uint32_t i = tid; i < me.cnt; i += CYTO_WG) {
                const md_site s = S.site[me.off + i];
                md_site_var v; v.noff = v.nvar = 0; if(S.var) v = S.var[me.off + i];
                const int64_t at = (int64_t)s.pos - T0;
                if(at >= 0 && at < span && !site_is_variant(K.min_opp, K.max_vf, S.var != nullptr, v)) { nm[at] = s.nmeth; nu[at] = s.nunmeth; }
            }
    }
    __syncthreads();
    const uint64_t base = S.row_base + pre;
    uint32_t written = 0;
    for(int r0 = 0; r0 < span; r0 += CYTO_WG) {
        const int i = r0 + tid;
        int code = 0;
        if(i < span) { code = cyto_code(sb, i + 2); if(code && !((K.ctx_mask >> ((code - 1) >> 1)) & 1)) code = 0; }
        const bool has = code != 0;
        // exclusive scan of `has` over the workgroup: ballot per wave, wave totals in LDS
        const uint64_t bal = __ballot(has);
        const uint32_t below = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if(lane == 0) wcnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = below, tot = 0;
        for(int w = 0; w < CYTO_WG / 64; w++) { if(w < wave) off += wcnt[w]; tot += wcnt[w]; }
        if(has && written + off < mine) {
            const uint64_t o = base + written + off;
            const bool is_g = !(code & 1);
            const int p = i + 2;
            K.contig[o] = S.tid; K.pos[o] = (int32_t)(T0 + i + 1); K.strand[o] = is_g ? (int8_t)-1 : (int8_t)1;
            K.nm[o] = (int32_t)nm[i]; K.nu[o] = (int32_t)nu[i]; K.ctx[o] = (uint8_t)((code - 1) >> 1);
            uint8_t *tr = K.tri + 3 * o;
            tr[0] = 'C'; tr[1] = is_g ? cyto_comp(sb[p - 1]) : cyto_fwd(sb[p + 1]); tr[2] = is_g ? cyto_comp(sb[p - 2]) : cyto_fwd(sb[p + 2]);
        }
        written += tot;
        __syncthreads();                 // (wcnt is rewritten by the next round)
    }
    if(tid == 0 && written != mine) atomicOr(K.err, 2u);
}

// rows src .. src + n of the arena to dst .. dst + n of the result
struct CytoEnt { uint64_t src, dst; uint32_t n, pad; };
struct KCytoGather {
    const CytoEnt *ent; uint64_t n_ent;
    const int32_t *contig, *pos, *nm, *nu; const int8_t *strand; const uint8_t *ctx, *tri;
    int32_t *o_contig, *o_pos, *o_nm, *o_nu; int8_t *o_strand; uint8_t *o_ctx, *o_tri;
};
__global__ __launch_bounds__(CYTO_WG) void k_cyto_gather(const KCytoGather G) {
    for(uint64_t e = blockIdx.x; e < G.n_ent; e += gridDim.x) {
        const CytoEnt g = G.ent[e];
        for(uint32_t i = threadIdx.x; i < g.n; i += CYTO_WG) {
            const uint64_t s = g.src + i, d = g.dst + i;
            G.o_contig[d] = G.contig[s]; G.o_pos[d] = G.pos[s]; G.o_strand[d] = G.strand[s]; G.o_nm[d] = G.nm[s]; G.o_nu[d] = G.nu[s]; G.o_ctx[d] = G.ctx[s];
        }
        for(uint32_t i = threadIdx.x; i < 3 * g.n; i += CYTO_WG) G.o_tri[3 * g.dst + i] = G.tri[3 * g.src + i];
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
void cyto_state_free(md_dev *h) {
    CytoState *c = h->cyto; if(!c) return;
    c->lane.close();
    c->rows.release();
    if(c->d_tilecnt) (void)hipFree(c->d_tilecnt);
    if(c->d_tot) (void)hipFree(c->d_tot);
    if(c->d_err) (void)hipFree(c->d_err);
    delete c; h->cyto = nullptr;
}

extern "C" int md_dev_cytosines_begin(md_dev *h, const md_cyto_cfg *cfg) {
    if(!h || !cfg || (!cfg->ctx_on[0] && !cfg->ctx_on[1] && !cfg->ctx_on[2])) return fail(MDK_ERR_ARG, "md_dev_cytosines_begin", hipSuccess);
    if(h->tile > CYTO_TILE_MAX) return fail(MDK_ERR_ARG, "md_dev_cytosines_begin: the handle's tile is larger than the report's kernels stage", hipSuccess);
    HIPCHK(hipSetDevice(h->device));
    if(!h->cyto) h->cyto = new CytoState();
    CytoState *c = h->cyto;
    { const int rc = c->lane.open(h->device); if(rc) return rc; }
    if(!c->d_err) HIPCHK(hipMalloc((void **)&c->d_err, sizeof(uint32_t)));
    if(!c->d_tot) HIPCHK(hipMalloc((void **)&c->d_tot, sizeof(unsigned long long) * MAXM));
    HIPCHK(hipMemsetAsync(c->d_err, 0, sizeof(uint32_t), c->lane.st));
    c->cfg = *cfg; c->on = true; c->used_rows = 0; c->chunks.clear();
    h->no_pack = true;            // group launches stop copying their sites to pinned host memory: nobody downloads them
    return 0;
}

extern "C" int md_dev_cytosines_group(md_dev *h, const int *slots, const md_cyto_chunk *chunks, int n, int *rcs) {
    if(!h || !slots || !chunks || !rcs || n < 1 || n > MAXM || !h->cyto || !h->cyto->on) return fail(MDK_ERR_ARG, "md_dev_cytosines_group", hipSuccess);
    HIPCHK(hipSetDevice(h->device));
    CytoState *c = h->cyto;
    Slot *ss[MAXM], *ls[MAXM]; int64_t cnt[MAXM]; int nl = 0;
    KCyto K; memset(&K, 0, sizeof(K));
    // the chunks' geometry: the slot's tiles where there is a slot, the handle's otherwise
    uint64_t tiles = 0;
    for(int i = 0; i < n; i++) {
        const md_cyto_chunk &q = chunks[i];
        ss[i] = nullptr; rcs[i] = 0; cnt[i] = 0;
        if(q.tid < 0 || (size_t)q.tid >= h->ref.size() || !h->ref[q.tid]) { snprintf(mdk_err_buf(), MDK_ERR_BYTES, "reference for tid %d not uploaded", q.tid); return MDK_ERR_NOREF; }
        if(q.beg < 0 || q.end < q.beg || ((uintptr_t)h->ref[q.tid] & 15)) return fail(MDK_ERR_ARG, "md_dev_cytosines_group: bad chunk", hipSuccess);
        int tile = h->tile;
        if(slots[i] >= 0) {
            Slot *s = get_slot(h, slots[i]);
            if(!s || !s->launched) return fail(MDK_ERR_ARG, "md_dev_cytosines_group: slot not launched", hipSuccess);
            if(s->tid != q.tid || s->beg != q.beg || s->end != q.end) return fail(MDK_ERR_ARG, "md_dev_cytosines_group: the slot holds another chunk", hipSuccess);
            for(int k = 0; k < nl; k++) if(ls[k] == s) return fail(MDK_ERR_ARG, "md_dev_cytosines_group: a slot named twice", hipSuccess);
            ss[i] = s; ls[nl++] = s; tile = s->tile;
        }
        if(tile < 1 || tile > CYTO_TILE_MAX) return fail(MDK_ERR_ARG, "md_dev_cytosines_group: tile", hipSuccess);
        const int64_t nt = (q.end - q.beg + tile - 1) / tile;
        if(nt > 0x3fffffff) return fail(MDK_ERR_ARG, "md_dev_cytosines_group: chunk too large", hipSuccess);
        if(ss[i] && (int64_t)std::max(ss[i]->ntiles, 0) != nt) return fail(MDK_ERR_ARG, "md_dev_cytosines_group: the slot's tiles do not cover the chunk", hipSuccess);
        KCytoChunk &S = K.C[i];
        S.ref = (const uint8_t *)h->ref[q.tid]; S.reflen = h->reflen[q.tid]; S.beg = q.beg; S.end = q.end; S.tile = tile; S.ntiles = (int32_t)nt; S.tid = q.tid;
        S.tile_base = tiles; K.tstart[i] = (int)tiles; tiles += (uint64_t)nt;
        if(tiles > 0x7fffffffull) return fail(MDK_ERR_ARG, "md_dev_cytosines_group: too many tiles", hipSuccess);
    }
    K.n = n; K.tstart[n] = (int)tiles;
    K.min_opp = c->cfg.min_opposite_depth; K.max_vf = c->cfg.max_variant_frac;
    K.ctx_mask = (c->cfg.ctx_on[0] ? 1 : 0) | (c->cfg.ctx_on[1] ? 2 : 0) | (c->cfg.ctx_on[2] ? 4 : 0);
    // the counting pass, queued before the wait for the group: it needs the bases alone
    if(tiles > c->tile_cap) {      // (nothing queued here reads the old table once the lane is idle)
        HIPCHK(hipStreamSynchronize(c->lane.st));
        if(c->d_tilecnt) (void)hipFree(c->d_tilecnt);
        c->d_tilecnt = nullptr; c->tile_cap = 0;
        const uint64_t want = std::max<uint64_t>(tiles + tiles / 2, 1u << 14);
        hipError_t e = hipMalloc((void **)&c->d_tilecnt, sizeof(uint32_t) * want);
        if(e != hipSuccess) return fail(MDK_ERR_NOMEM, "hipMalloc(cytosine tile counts)", e);
        c->tile_cap = want;
    }
    K.tilecnt = c->d_tilecnt; K.tot = c->d_tot; K.err = c->d_err;
    HIPCHK(hipMemsetAsync(c->d_tot, 0, sizeof(unsigned long long) * MAXM, c->lane.st));
    if(tiles > 0) {
        hipLaunchKernelGGL(k_cyto_count, dim3((unsigned)tiles), dim3(CYTO_WG), 0, c->lane.st, K);
        HIPCHK(hipGetLastError());
    }
    // wait for the group as md_dev_calls_group does (one copy of the status blocks when the slots shared one launch)
    if(nl) {
        int lo = 0x7fffffff, hi = -1; hipStream_t st = nullptr;
        for(int k = 0; k < nl; k++) {
            if(k == 0) st = ls[k]->run; else if(ls[k]->run != st) st = nullptr;
            lo = std::min(lo, ls[k]->index); hi = std::max(hi, ls[k]->index);
        }
        if(st) {
            ProfScope pf(PF_FIN_WAIT);
            HIPCHK(hipMemcpyAsync(h->h_status.p + lo, h->d_status.p + lo, sizeof(SlotStatus) * (size_t)(hi - lo + 1), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for(int i = 0; i < n; i++) if(ss[i]) { cnt[i] = finish_eval(h, ss[i]); if(cnt[i] < 0) rcs[i] = (int)cnt[i]; }
        } else
            for(int i = 0; i < n; i++) if(ss[i]) { cnt[i] = finish_count(h, ss[i]); if(cnt[i] < 0) rcs[i] = (int)cnt[i]; }
        for(int i = 0; i < n; i++) if(ss[i] && !rcs[i]) HIPCHK(hipStreamSynchronize(ss[i]->run ? ss[i]->run : ss[i]->stream));     // (a chunk prepared and piled up again inside finish_eval)
    }
    // the totals (the counting pass is short next to a pileup: it has run by now)
    unsigned long long tot[MAXM];
    HIPCHK(hipStreamSynchronize(c->lane.st));
    HIPCHK(hipMemcpy(tot, c->d_tot, sizeof(tot), hipMemcpyDeviceToHost));
    uint64_t rows = 0;
    for(int i = 0; i < n; i++) if(!rcs[i]) rows += tot[i];
    // room for exactly the group's rows (growing copies what is there, behind every fill queued so far)
    { const int rc = c->rows.reserve(c->used_rows, rows, CYTO_ROWS_FLOOR, c->lane.st); if(rc) return rc; }
    K.contig = c->rows.col<int32_t>(Y_CONTIG); K.pos = c->rows.col<int32_t>(Y_POS); K.strand = c->rows.col<int8_t>(Y_STRAND);
    K.nm = c->rows.col<int32_t>(Y_NM); K.nu = c->rows.col<int32_t>(Y_NU); K.ctx = c->rows.col<uint8_t>(Y_CTX); K.tri = c->rows.col<uint8_t>(Y_TRI);
    // the filling pass over the chunks that have rows: the same tiles (tile_base stays), renumbered workgroups
    KCyto F = K; F.n = 0; int total = 0;
    for(int i = 0; i < n; i++) {
        if(rcs[i]) continue;
        CytoChunk ch; ch.key = chunks[i].key; ch.row0 = c->used_rows; ch.n = tot[i];
        c->chunks.push_back(ch);
        if(!tot[i]) continue;
        KCytoChunk &S = F.C[F.n]; S = K.C[i];
        S.row_base = c->used_rows; S.total = tot[i];
        Slot *s = ss[i];
        if(s && cnt[i] > 0) {
            S.site = s->b_site ? s->b_site : s->d_site.p; S.var = h->variant ? (s->b_site ? s->b_var : s->d_var.p) : nullptr; S.seg = s->b_site ? s->b_seg : s->d_seg.p;
            S.site_cap = (uint32_t)std::min<int64_t>(cnt[i], 0xfffffff0ll);
        }
        F.tstart[F.n] = total; total += S.ntiles; F.n++;
        c->used_rows += tot[i];
    }
    F.tstart[F.n] = total;
    if(total > 0) {
        hipLaunchKernelGGL(k_cyto_fill, dim3((unsigned)total), dim3(CYTO_WG), 0, c->lane.st, F);
        HIPCHK(hipGetLastError());
    }
    // the slots' next uploads and launches come after the fill has read their sites
    if(nl) { const int rc = c->lane.fence(ls, nl); if(rc) return rc; }
    for(int k = 0; k < nl; k++) ls[k]->busy = false;
    return 0;
}

extern "C" int md_dev_cytosines_finish(md_dev *h, md_cytosines_set **out) {
    if(!h || !out || !h->cyto || !h->cyto->on) return fail(MDK_ERR_ARG, "md_dev_cytosines_finish", hipSuccess);
    *out = nullptr;
    HIPCHK(hipSetDevice(h->device));
    CytoState *c = h->cyto;
    hipStream_t st = c->lane.st;
    HIPCHK(hipStreamSynchronize(st));
    uint32_t err = 0;
    HIPCHK(hipMemcpy(&err, c->d_err, sizeof(err), hipMemcpyDeviceToHost));
    c->on = false; h->no_pack = false;
    if(err) { c->used_rows = 0; c->chunks.clear(); return fail(MDK_ERR_ARG, (err & 1) ? "md_dev_cytosines_finish: inconsistent tile segments" : "md_dev_cytosines_finish: the counting and the filling pass disagree", hipSuccess); }
    std::vector<CytoChunk> ch = c->chunks;
    std::stable_sort(ch.begin(), ch.end(), [](const CytoChunk &a, const CytoChunk &b) { return a.key < b.key; });
    std::vector<CytoEnt> ge; uint64_t n = 0;
    for(const CytoChunk &k : ch) {
        if(k.row0 + k.n > c->used_rows) return fail(MDK_ERR_ARG, "md_dev_cytosines_finish: a chunk's rows lie outside the arena", hipSuccess);
        for(uint64_t o = 0; o < k.n; o += 1u << 16) { CytoEnt g; g.src = k.row0 + o; g.dst = n + o; g.n = (uint32_t)std::min<uint64_t>(k.n - o, 1u << 16); g.pad = 0; ge.push_back(g); }
        n += k.n;
    }
    md_cytosines_set *r = new md_cytosines_set(); r->device = h->device; r->n = (int64_t)n;
    { const int rc = r->cols.reserve(0, n + 64, 0, st); if(rc) { delete r; return rc; } }
    if(!ge.empty()) {
        CytoEnt *d_ge = nullptr;
        hipError_t e = hipMalloc((void **)&d_ge, sizeof(CytoEnt) * ge.size());
        if(e == hipSuccess) e = hipMemcpyAsync(d_ge, ge.data(), sizeof(CytoEnt) * ge.size(), hipMemcpyHostToDevice, st);
        if(e == hipSuccess) {
            const ColTable &a = c->rows, &o = r->cols;
            KCytoGather G; G.ent = d_ge; G.n_ent = ge.size();
            G.contig = a.col<int32_t>(Y_CONTIG); G.pos = a.col<int32_t>(Y_POS); G.strand = a.col<int8_t>(Y_STRAND); G.nm = a.col<int32_t>(Y_NM);
            G.nu = a.col<int32_t>(Y_NU); G.ctx = a.col<uint8_t>(Y_CTX); G.tri = a.col<uint8_t>(Y_TRI);
            G.o_contig = o.col<int32_t>(Y_CONTIG); G.o_pos = o.col<int32_t>(Y_POS); G.o_strand = o.col<int8_t>(Y_STRAND); G.o_nm = o.col<int32_t>(Y_NM);
            G.o_nu = o.col<int32_t>(Y_NU); G.o_ctx = o.col<uint8_t>(Y_CTX); G.o_tri = o.col<uint8_t>(Y_TRI);
            const unsigned grid = (unsigned)std::min<size_t>(ge.size(), 65536);
            hipLaunchKernelGGL(k_cyto_gather, dim3(grid), dim3(CYTO_WG), 0, st, G);
            e = hipGetLastError();
            if(e == hipSuccess) e = hipStreamSynchronize(st);
        }
        if(d_ge) (void)hipFree(d_ge);
        if(e != hipSuccess) { r->cols.release(); delete r; return fail(MDK_ERR_HIP, "k_cyto_gather", e); }
    }
    c->used_rows = 0; c->chunks.clear();
    *out = r;
    return 0;
}

extern "C" int64_t md_cytosines_set_count(const md_cytosines_set *c) { return c ? c->n : MDK_ERR_ARG; }

extern "C" int md_cytosines_set_copy(const md_cytosines_set *c, const md_cytosines_cols *dst, int to_host) {
    if(!c || !dst) return fail(MDK_ERR_ARG, "md_cytosines_set_copy", hipSuccess);
    HIPCHK(hipSetDevice(c->device));
    const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if(!c->n) return 0;
    void *const to[] = {dst->contig, dst->pos, dst->strand, dst->nmeth, dst->nunmeth, dst->context, dst->trinucleotide};        // Y_CONTIG .. Y_TRI
    for(int i = 0; i < 7; i++) if(to[i]) { const int rc = c->cols.copy_out(i, (uint64_t)c->n, to[i], kind); if(rc) return rc; }
    return 0;
}

extern "C" void md_cytosines_set_free(md_cytosines_set *c) {
    if(!c) return;
    (void)hipSetDevice(c->device);
    c->cols.release();
    delete c;
}
