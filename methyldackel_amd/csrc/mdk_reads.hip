// mdk_reads.hip -- the rows of `perRead` as device-resident columns (include/mdk_hip.h, "reads on the device").
//
// What addRead (perRead.c:16-36) prints for a kept read -- name, contig, position and the read's CpG calls -- kept as columns for a
// resident session instead of formatted by the host.  For a chunk the device selected (k_prep_scan_ordered) and walked (k_perread_raw),
// no per-read data crosses to the host:
//   k_reads_len     (slot stream, behind k_perread_raw) per kept read the length of its name -- l_read_name, then a bounded scan for
//                   the first NUL -- and the exclusive scan of those lengths inside its workgroup (ballot-free: wave64 __shfl_up, wave
//                   totals in LDS); the workgroup's total to a per-slot table;
//   k_reads_blocks  (slot stream, one workgroup) the exclusive scan of those totals, and the chunk's name bytes into the slot's status
//                   block, which the host copies back anyway (PrepCounters.name_bytes next to n_adm);
//   k_reads_rows    (the handle's reads stream, once the host knows the two totals) contig, pos, counts and the int64 name offsets of
//                   the chunk's rows, at the run arena's exact end;
//   k_reads_names   (reads stream) the name bytes, one output byte per lane: consecutive lanes store consecutive bytes, each found by
//                   a binary search over the offsets k_reads_rows wrote.
// Chunks are appended in the order md_dev_reads_collect is called (the caller's schedule order): the arena needs no final gather.
#include "mdk_hip_internal.hpp"
#include <algorithm>

#define READS_WG 256
#define READS_SCAN_WG 1024
#define READS_NAME_OFF 36u           // the name's offset from a record's block_size word; l_read_name at +12, pos at +8

struct ReadsSlot { DBuf<uint32_t> loc, boff; };       // per kept read: its name's offset inside its workgroup's; per workgroup: the offset of its names in the chunk
// columns of the rows (md_reads_cols' order; the name offsets hold one entry more: the end of the last name) and of the name bytes
enum { C_CONTIG = 0, C_POS, C_NM, C_NU, C_OFF };
static const ColSpec ROW_COLS[] = {{4, 0}, {4, 0}, {4, 0}, {4, 0}, {8, 1}};
static const ColSpec BYTE_COLS[] = {{1, 0}};
struct ReadsTables {
    ColTable rows{ROW_COLS, 5, "hipMalloc(read rows)"}, bytes{BYTE_COLS, 1, "hipMalloc(read names)"};
    int32_t *i32(int i) const { return rows.col<int32_t>(i); }
    int64_t *off() const { return rows.col<int64_t>(C_OFF); }
    uint8_t *names() const { return bytes.col<uint8_t>(0); }
    void release() { rows.release(); bytes.release(); }
};
struct ReadsState {
    TableLane lane;                                           // the appends run here
    ReadsTables t; uint64_t used_rows = 0, used_bytes = 0;    // the run's rows: kept across runs
    std::vector<ReadsSlot> slots;
};

struct md_reads_set { int device = 0; int64_t n = 0, n_bytes = 0; ReadsTables t; };

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
struct KReadsScan { const uint8_t *raw; uint64_t raw_span; const uint32_t *rec_at, *aidx; PrepCounters *cnt; uint32_t *loc, *boff; };

// the name of the record at `o`: l_read_name bytes up to the first NUL, never past the chunk's records
__device__ __forceinline__ uint32_t name_len(const uint8_t *raw, uint64_t raw_span, uint32_t o) {
    if((uint64_t)o + READS_NAME_OFF > raw_span) return 0;
    const uint64_t room = raw_span - o - READS_NAME_OFF;
    const uint32_t lim = room < raw[o + 12] ? (uint32_t)room : (uint32_t)raw[o + 12];
    const uint8_t *q = raw + o + READS_NAME_OFF;
    uint32_t k = 0;
    for(; k + 4 <= lim; k += 4) {                  // a word at a time while it stays inside l_read_name
        uint32_t w; __builtin_memcpy(&w, q + k, 4);
        if(!(w & 0xffu)) return k;
        if(!(w & 0xff00u)) return k + 1;
        if(!(w & 0xff0000u)) return k + 2;
        if(!(w & 0xff000000u)) return k + 3;
    }
    for(; k < lim; k++) if(!q[k]) return k;
    return lim;
}

__global__ __launch_bounds__(READS_WG) void k_reads_len(const KReadsScan K) {
    __shared__ uint32_t wtot[READS_WG / 64];
    const uint32_t n = K.cnt->n_adm;
    if(blockIdx.x * READS_WG >= n) return;                      // (the grid covers every candidate record; the kept ones are fewer)
    const uint32_t a = blockIdx.x * READS_WG + threadIdx.x;
    const uint32_t len = a < n ? name_len(K.raw, K.raw_span, K.rec_at[K.aidx[a]]) : 0u;
    uint32_t total;
    const uint32_t ex = block_excl_scan<READS_WG>(len, wtot, total);
    if(a < n) K.loc[a] = ex;
    if(threadIdx.x == 0) K.boff[blockIdx.x] = total;
}

__global__ __launch_bounds__(READS_SCAN_WG) void k_reads_blocks(const KReadsScan K) {
    __shared__ uint32_t wtot[READS_SCAN_WG / 64];
    const uint32_t n = K.cnt->n_adm, nb = (n + READS_WG - 1) / READS_WG;
    uint32_t carry = 0;
    for(uint32_t b0 = 0; b0 < nb; b0 += READS_SCAN_WG) {        // (uniform trip count: every thread takes part in every scan)
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < nb ? K.boff[b] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan<READS_SCAN_WG>(v, wtot, total);
        if(b < nb) K.boff[b] = carry + ex;
        carry += total;
    }
    if(threadIdx.x == 0) K.cnt->name_bytes = carry;
}

struct KReadsRows {
    const uint8_t *raw; const uint32_t *rec_at, *aidx, *loc, *boff; const md_pr_count *prc; uint32_t n, total; int32_t tid;
    uint64_t row, byte_base;
    int32_t *contig, *pos, *nm, *nu; int64_t *off;
};
__global__ __launch_bounds__(READS_WG) void k_reads_rows(const KReadsRows K) {
    const uint32_t a = blockIdx.x * READS_WG + threadIdx.x;
    if(a > K.n) return;
    const uint64_t r = K.row + a;
    if(a == K.n) { K.off[r] = (int64_t)(K.byte_base + K.total); return; }      // the end of the chunk's names (the next chunk's first offset)
    int32_t p; __builtin_memcpy(&p, K.raw + K.rec_at[K.aidx[a]] + 8, 4);
    const md_pr_count c = K.prc[a];
    K.contig[r] = K.tid; K.pos[r] = p; K.nm[r] = (int32_t)c.nmeth; K.nu[r] = (int32_t)c.nunmeth;
    K.off[r] = (int64_t)(K.byte_base + K.boff[a / READS_WG] + K.loc[a]);
}

struct KReadsNames { const uint8_t *raw; const uint32_t *rec_at, *aidx; const int64_t *off; uint32_t n, total; uint64_t row, byte_base; uint8_t *bytes; };
// the largest a in [lo, hi] with off[a] <= p (off ascending, off[lo] <= p)
__device__ __forceinline__ uint32_t reads_find(const int64_t *off, uint32_t lo, uint32_t hi, int64_t p) {
    while(lo < hi) { const uint32_t m = lo + (hi - lo + 1) / 2; if(off[m] <= p) lo = m; else hi = m - 1; }
    return lo;
}
__global__ __launch_bounds__(READS_WG) void k_reads_names(const KReadsNames K) {
    __shared__ uint32_t s_lo, s_hi;
    const int64_t *off = K.off + K.row;                          // off[0 .. n]: this chunk's rows, absolute
    for(uint64_t t0 = (uint64_t)blockIdx.x * READS_WG; t0 < K.total; t0 += (uint64_t)gridDim.x * READS_WG) {
        const uint64_t last = (t0 + READS_WG < K.total ? t0 + READS_WG : (uint64_t)K.total) - 1;
        if(threadIdx.x == 0) s_lo = reads_find(off, 0, K.n - 1, (int64_t)(K.byte_base + t0));
        if(threadIdx.x == 1) s_hi = reads_find(off, 0, K.n - 1, (int64_t)(K.byte_base + last));
        __syncthreads();
        const uint64_t j = t0 + threadIdx.x;
        if(j < K.total) {
            const int64_t p = (int64_t)(K.byte_base + j);
            const uint32_t a = reads_find(off, s_lo, s_hi, p);
            K.bytes[p] = K.raw[K.rec_at[K.aidx[a]] + READS_NAME_OFF + (uint64_t)(p - off[a])];
        }
        __syncthreads();             // (s_lo / s_hi are rewritten by the next tile)
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// room for `rows` more rows and `bytes` more name bytes (growing copies what is there, behind every append queued so far)
static int reads_reserve(ReadsState *r, uint64_t rows, uint64_t bytes) {
    const int rc = r->t.rows.reserve(r->used_rows, rows, READS_ROWS_FLOOR, r->lane.st);
    return rc ? rc : r->t.bytes.reserve(r->used_bytes, bytes, READS_BYTES_FLOOR, r->lane.st);
}

void reads_state_free(md_dev *h) {
    ReadsState *r = h->reads; if(!r) return;
    r->lane.close();
    r->t.release();
    for(ReadsSlot &s : r->slots) { s.loc.release(); s.boff.release(); }
    delete r; h->reads = nullptr; h->reads_on = false;
}

extern "C" int md_dev_reads_begin(md_dev *h) {
    if(!h) return fail(MDK_ERR_ARG, "md_dev_reads_begin", hipSuccess);
    HIPCHK(hipSetDevice(h->device));
    if(!h->reads) h->reads = new ReadsState();
    ReadsState *r = h->reads;
    { const int rc = r->lane.open(h->device); if(rc) return rc; }
    if(r->slots.size() < (size_t)h->n_slots) r->slots.resize((size_t)h->n_slots);
    r->used_rows = 0; r->used_bytes = 0;
    h->reads_on = true;
    return 0;
}

extern "C" int md_dev_reads_slot(md_dev *h, int slot) {
    Slot *s = get_slot(h, slot);
    if(!s || !h->reads || !h->reads_on || s->pr_n < 0 || !s->raw_layout) return fail(MDK_ERR_ARG, "md_dev_reads_slot: md_dev_reads_begin and md_dev_perread_submit_raw on the slot first", hipSuccess);
    HIPCHK(hipSetDevice(h->device));
    ReadsSlot &rs = h->reads->slots[(size_t)slot];
    const int n = s->pr_nrec, nb = (n + READS_WG - 1) / READS_WG;
    if(rs.loc.need((size_t)n + 1) || rs.boff.need((size_t)nb + 1)) return MDK_ERR_NOMEM;
    KReadsScan K; K.raw = s->raw_at; K.raw_span = s->raw_span; K.rec_at = s->rec_at; K.aidx = s->d_aidx.p; K.cnt = s->d_pcnt.p; K.loc = rs.loc.p; K.boff = rs.boff.p;
    if(nb > 0) hipLaunchKernelGGL(k_reads_len, dim3((unsigned)nb), dim3(READS_WG), 0, s->stream, K);
    hipLaunchKernelGGL(k_reads_blocks, dim3(1), dim3(READS_SCAN_WG), 0, s->stream, K);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s->h_st.p, h->d_status.p + s->index, sizeof(SlotStatus), hipMemcpyDeviceToHost, s->stream));
    return 0;
}

extern "C" int md_dev_reads_collect(md_dev *h, int slot, int64_t *n_out) {
    Slot *s = get_slot(h, slot);
    if(!s || !n_out || !h->reads || !h->reads_on || s->pr_n < 0) return fail(MDK_ERR_ARG, "md_dev_reads_collect: nothing submitted on this slot", hipSuccess);
    *n_out = 0;
    HIPCHK(hipSetDevice(h->device));
    ReadsState *r = h->reads; ReadsSlot &rs = r->slots[(size_t)slot];
    HIPCHK(hipStreamSynchronize(s->stream));
    const PrepCounters &c = s->h_st.p->pc;
    if(c.malformed) { snprintf(mdk_err_buf(), MDK_ERR_BYTES, "malformed BAM record in the chunk"); return MDK_ERR_ARG; }
    const uint32_t n = c.n_adm, total = c.name_bytes;
    if(n > (uint32_t)std::max(s->pr_nrec, 0) || total > s->raw_span) return fail(MDK_ERR_ARG, "md_dev_reads_collect: inconsistent counts", hipSuccess);
    if(n == 0) return 0;
    { const int rc = reads_reserve(r, n, total); if(rc) return rc; }
    KReadsRows R; R.raw = s->raw_at; R.rec_at = s->rec_at; R.aidx = s->d_aidx.p; R.loc = rs.loc.p; R.boff = rs.boff.p; R.prc = s->d_prc.p; R.n = n; R.total = total; R.tid = s->tid;
    R.row = r->used_rows; R.byte_base = r->used_bytes; R.contig = r->t.i32(C_CONTIG); R.pos = r->t.i32(C_POS); R.nm = r->t.i32(C_NM); R.nu = r->t.i32(C_NU); R.off = r->t.off();
    hipLaunchKernelGGL(k_reads_rows, dim3((n + 1 + READS_WG - 1) / READS_WG), dim3(READS_WG), 0, r->lane.st, R);
    if(total) {
        KReadsNames N; N.raw = s->raw_at; N.rec_at = s->rec_at; N.aidx = s->d_aidx.p; N.off = r->t.off(); N.n = n; N.total = total; N.row = r->used_rows; N.byte_base = r->used_bytes; N.bytes = r->t.names();
        const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)total + READS_WG - 1) / READS_WG, 1u << 16);
        hipLaunchKernelGGL(k_reads_names, dim3(grid), dim3(READS_WG), 0, r->lane.st, N);
    }
    HIPCHK(hipGetLastError());
    // the slot's next submit comes after the appends have read its records, kept reads and counts
    { const int rc = r->lane.fence(&s, 1); if(rc) return rc; }
    r->used_rows += n; r->used_bytes += total;
    *n_out = n;
    return 0;
}

extern "C" int md_dev_reads_host(md_dev *h, int32_t tid, int64_t n, const int32_t *pos, const md_pr_count *counts, const uint64_t *name_off, const uint8_t *names) {
    if(!h || !h->reads || !h->reads_on || tid < 0 || n < 0 || (n && (!pos || !name_off || (name_off[n] > name_off[0] && !names)))) return fail(MDK_ERR_ARG, "md_dev_reads_host", hipSuccess);
    if(n == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    ReadsState *r = h->reads;
    const uint64_t total = name_off[n] - name_off[0];
    { const int rc = reads_reserve(r, (uint64_t)n, total); if(rc) return rc; }
    std::vector<int32_t> ct((size_t)n, tid), nm((size_t)n, 0), nu((size_t)n, 0); std::vector<int64_t> off((size_t)n + 1);
    for(int64_t i = 0; i < n; i++) { if(counts) { nm[(size_t)i] = (int32_t)counts[i].nmeth; nu[(size_t)i] = (int32_t)counts[i].nunmeth; } off[(size_t)i] = (int64_t)(r->used_bytes + name_off[i] - name_off[0]); }
    off[(size_t)n] = (int64_t)(r->used_bytes + total);
    const size_t row = (size_t)r->used_rows; hipStream_t st = r->lane.st;
    HIPCHK(hipMemcpyAsync(r->t.i32(C_CONTIG) + row, ct.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(r->t.i32(C_POS) + row, pos, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(r->t.i32(C_NM) + row, nm.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(r->t.i32(C_NU) + row, nu.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(r->t.off() + row, off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    if(total) HIPCHK(hipMemcpyAsync(r->t.names() + r->used_bytes, names + name_off[0], (size_t)total, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));        // (the host arrays go when this returns)
    r->used_rows += (uint64_t)n; r->used_bytes += total;
    return 0;
}

extern "C" int md_dev_reads_finish(md_dev *h, md_reads_set **out) {
    if(!h || !out || !h->reads || !h->reads_on) return fail(MDK_ERR_ARG, "md_dev_reads_finish", hipSuccess);
    *out = nullptr;
    HIPCHK(hipSetDevice(h->device));
    ReadsState *r = h->reads;
    h->reads_on = false;
    hipStream_t st = r->lane.st;
    HIPCHK(hipStreamSynchronize(st));
    md_reads_set *q = new md_reads_set(); q->device = h->device; q->n = (int64_t)r->used_rows; q->n_bytes = (int64_t)r->used_bytes;
    const uint64_t n = r->used_rows;
    // at their exact size (an empty set still holds its one offset, 0); the run's columns copied one by one
    int rc = q->t.rows.reserve(0, std::max<uint64_t>(n, 1), 0, st);
    if(!rc) rc = q->t.bytes.reserve(0, r->used_bytes, 0, st);
    if(rc) { q->t.release(); delete q; return rc; }
    hipError_t e = hipSuccess;
    if(n) {
        for(int i = 0; i < 5 && e == hipSuccess; i++) e = hipMemcpyAsync(q->t.rows.col<char>(i), r->t.rows.col<char>(i), (size_t)(n + ROW_COLS[i].extra) * ROW_COLS[i].elem, hipMemcpyDeviceToDevice, st);
        if(e == hipSuccess && q->n_bytes) e = hipMemcpyAsync(q->t.names(), r->t.names(), (size_t)q->n_bytes, hipMemcpyDeviceToDevice, st);
    } else e = hipMemsetAsync(q->t.off(), 0, 8, st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) { q->t.release(); delete q; return fail(MDK_ERR_HIP, "md_dev_reads_finish: copies", e); }
    r->used_rows = 0; r->used_bytes = 0;
    *out = q;
    return 0;
}

extern "C" int64_t md_reads_set_count(const md_reads_set *r) { return r ? r->n : MDK_ERR_ARG; }
extern "C" int64_t md_reads_set_name_bytes(const md_reads_set *r) { return r ? r->n_bytes : MDK_ERR_ARG; }

extern "C" int md_reads_set_copy(const md_reads_set *r, const md_reads_cols *dst, int to_host) {
    if(!r || !dst) return fail(MDK_ERR_ARG, "md_reads_set_copy", hipSuccess);
    HIPCHK(hipSetDevice(r->device));
    const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const uint64_t n = (uint64_t)r->n;
    void *const to[] = {dst->contig, dst->pos, dst->nmeth, dst->nunmeth, dst->name_off};        // C_CONTIG .. C_OFF
    for(int i = 0; i < 5; i++)         // (an empty set still copies its one name offset, 0)
        if(to[i] && n + ROW_COLS[i].extra) { const int rc = r->t.rows.copy_out(i, n + ROW_COLS[i].extra, to[i], kind); if(rc) return rc; }
    if(dst->name_bytes && r->n_bytes) return r->t.bytes.copy_out(0, (uint64_t)r->n_bytes, dst->name_bytes, kind);
    return 0;
}

extern "C" void md_reads_set_free(md_reads_set *r) {
    if(!r) return;
    (void)hipSetDevice(r->device);
    r->t.release();
    delete r;
}
