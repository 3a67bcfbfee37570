// mdk_bias.hip -- the result of an `mbias` run as device-resident columns (include/mdk_hip.h, "the methylation-bias table on the device").
//
// At the end of a run the device histogram [q][16] (mdk_hip.hip: k_mbias, k_mbias_multi) becomes what a resident session hands out:
//   * the rows of the command's table, in the order mdk_mbias_report prints them -- strand OT, OB, CTOT, CTOB; within a strand ascending
//     position; within a position read 1 then read 2; a row only where nmeth || nunmeth -- as the columns strand, read, position (1-based),
//     nmeth, nunmeth;
//   * the dense histogram as int64 [len][4][2][2] (position, strand, read, methylated/unmethylated): the histogram's own layout, widened.
// k_bias_rows runs twice, one workgroup each time (a histogram is 16 x the longest read: some thousand entries).  The first pass widens the
// histogram, copies it to a staging array and counts the rows behind it, so that ONE copy brings the host the histogram it computes the
// inclusion bounds from and the row count; the table is then reserved at its exact size and the second pass fills it.  Both passes walk the
// (strand, position, read) entries in output order, 256 at a time: wave64 ballot, the lanes below in the mask, wave totals through LDS.
#include "mdk_hip_internal.hpp"
#include <algorithm>

#define BIAS_WG 256

enum { B_STRAND = 0, B_READ, B_POS, B_NM, B_NU };
static const ColSpec BIAS_ROW_COLS[] = {{1, 0}, {1, 0}, {4, 0}, {8, 0}, {8, 0}};
static const ColSpec BIAS_DENSE_COLS[] = {{8, 0}};

struct md_bias_set {
    int device = 0; int64_t n = 0; int len = 0, redone = 0;
    ColTable rows{BIAS_ROW_COLS, 5, "hipMalloc(mbias rows)"}, dense{BIAS_DENSE_COLS, 1, "hipMalloc(mbias counts)"};
    std::vector<uint32_t> hist;                  // the histogram on the host: rows [q][16], q < len
    void release() { rows.release(); dense.release(); }
};

struct KBias {
    const uint32_t *hist; int len;
    int64_t *dense; uint32_t *stage;                                      // first pass: [16 * len] each; stage[16 * len] = the number of rows
    int8_t *strand, *read; int32_t *pos; int64_t *nm, *nu; uint32_t cap;  // second pass: the table's columns and their size
};

template <bool WRITE>
__global__ __launch_bounds__(BIAS_WG) void k_bias_rows(const KBias K) {
    __shared__ uint32_t wtot[BIAS_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int items = 2 * K.len;
    uint32_t carry = 0;
    for(int s = 0; s < 4; s++) {
        for(int i0 = 0; i0 < items; i0 += BIAS_WG) {           // (uniform trip count: every thread takes part in every ballot and barrier)
            const int i = i0 + tid, q = i >> 1, r = i & 1;
            uint32_t m = 0, u = 0;
            if(i < items) { const int at = q * 16 + s * 4 + 2 * r; m = K.hist[at]; u = K.hist[at + 1]; if(!WRITE) { K.dense[at] = (int64_t)m; K.dense[at + 1] = (int64_t)u; K.stage[at] = m; K.stage[at + 1] = u; } }
            const bool present = (m | u) != 0;
            const unsigned long long mask = __ballot(present);
            const uint32_t below = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if(lane == 0) wtot[wave] = (uint32_t)__popcll(mask);
            __syncthreads();
            uint32_t before = 0, total = 0;
            for(int w = 0; w < BIAS_WG / 64; w++) { const uint32_t t = wtot[w]; if(w < wave) before += t; total += t; }
            __syncthreads();                                    // (wtot is rewritten by the next round)
            if(WRITE && present) {
                const uint32_t o = carry + before + below;
                if(o < K.cap) { K.strand[o] = (int8_t)s; K.read[o] = (int8_t)(r + 1); K.pos[o] = q + 1; K.nm[o] = (int64_t)m; K.nu[o] = (int64_t)u; }
            }
            carry += total;
        }
    }
    if(!WRITE && tid == 0) K.stage[16 * K.len] = carry;
}

extern "C" int md_dev_bias_finish(md_dev *h, md_bias_set **out) {
    if(!h || !out) return fail(MDK_ERR_ARG, "md_dev_bias_finish", hipSuccess);
    *out = nullptr;
    HIPCHK(hipSetDevice(h->device));
    { const int rc = mbias_drain(h); if(rc) return rc; }
    if(h->slots.empty()) return fail(MDK_ERR_ARG, "md_dev_bias_finish: a handle without slots", hipSuccess);
    hipStream_t st = h->slots[0].stream;
    const int len = h->hist_len > 0 ? h->hist_len : 0;
    if(len > h->hist_cap) return fail(MDK_ERR_ARG, "md_dev_bias_finish: the histogram is shorter than its longest read", hipSuccess);
    md_bias_set *q = new md_bias_set(); q->device = h->device; q->len = len; q->redone = h->mb_redone;
    h->mb_redone = 0; if(len > 0) h->mb_hint = len;
    q->hist.assign((size_t)len * 16 + 1, 0u);
    if(len == 0) { *out = q; return 0; }
    const size_t words = (size_t)len * 16;
    uint32_t *stage = nullptr;
    hipError_t e = hipMalloc((void **)&stage, (words + 1) * sizeof(uint32_t));
    if(e != hipSuccess) { delete q; return fail(MDK_ERR_NOMEM, "hipMalloc(mbias staging)", e); }
    int rc = q->dense.reserve(0, words, 0, st);
    if(!rc) {
        KBias K; memset(&K, 0, sizeof(K));
        K.hist = h->d_hist; K.len = len; K.dense = q->dense.col<int64_t>(0); K.stage = stage;
        hipLaunchKernelGGL(k_bias_rows<false>, dim3(1), dim3(BIAS_WG), 0, st, K);
        e = hipGetLastError();
        if(e == hipSuccess) e = hipStreamSynchronize(st);
        if(e == hipSuccess) e = hipMemcpy(q->hist.data(), stage, (words + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost);      // (pageable memory: a synchronous copy, as md_dev_mbias_read's)
        if(e != hipSuccess) rc = fail(MDK_ERR_HIP, "md_dev_bias_finish: counting the rows", e);
        if(!rc) {
            q->n = (int64_t)q->hist[words];
            if((uint64_t)q->n > 8ull * (uint64_t)len) rc = fail(MDK_ERR_ARG, "md_dev_bias_finish: more rows than the histogram has entries", hipSuccess);
        }
        if(!rc && q->n) rc = q->rows.reserve(0, (uint64_t)q->n, 0, st);
        if(!rc && q->n) {
            K.strand = q->rows.col<int8_t>(B_STRAND); K.read = q->rows.col<int8_t>(B_READ); K.pos = q->rows.col<int32_t>(B_POS); K.nm = q->rows.col<int64_t>(B_NM); K.nu = q->rows.col<int64_t>(B_NU); K.cap = (uint32_t)q->n;
            hipLaunchKernelGGL(k_bias_rows<true>, dim3(1), dim3(BIAS_WG), 0, st, K);
            e = hipGetLastError();
            if(e == hipSuccess) e = hipStreamSynchronize(st);
            if(e != hipSuccess) rc = fail(MDK_ERR_HIP, "md_dev_bias_finish: writing the rows", e);
        }
    }
    (void)hipFree(stage);
    if(rc) { q->release(); delete q; return rc; }
    q->hist.resize(words);
    *out = q;
    return 0;
}

extern "C" int64_t md_bias_set_count(const md_bias_set *b) { return b ? b->n : MDK_ERR_ARG; }
extern "C" int md_bias_set_len(const md_bias_set *b) { return b ? b->len : MDK_ERR_ARG; }
extern "C" int md_bias_set_redone(const md_bias_set *b) { return b ? b->redone : MDK_ERR_ARG; }
extern "C" int md_bias_set_hist(const md_bias_set *b, md_mbias *out) {
    if(!b || !out) return fail(MDK_ERR_ARG, "md_bias_set_hist", hipSuccess);
    out->len = b->len; out->count = const_cast<uint32_t *>(b->hist.data());
    return 0;
}

extern "C" int md_bias_set_copy(const md_bias_set *b, int column, void *dst, int to_host) {
    if(!b || !dst || column < 0 || column > MD_BIAS_COUNTS) return fail(MDK_ERR_ARG, "md_bias_set_copy", hipSuccess);
    HIPCHK(hipSetDevice(b->device));
    const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if(column == MD_BIAS_COUNTS) return b->len ? b->dense.copy_out(0, (uint64_t)b->len * 16, dst, kind) : 0;
    return b->n ? b->rows.copy_out(column, (uint64_t)b->n, dst, kind) : 0;
}

extern "C" void md_bias_set_free(md_bias_set *b) {
    if(!b) return;
    (void)hipSetDevice(b->device);
    b->release();
    delete b;
}
