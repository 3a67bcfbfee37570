// mdk_tabix.hip -- libmdk_index.so (include/mdk_index.h): the per-line half of a tabix index on the device.  The rule is mdk_tabix_core.h's.
// A library of its own -- one code object, its own stream, its own error text -- that links nothing of libmdk_hip.so.
//
// The text comes piece by piece, whole lines each.  Per piece, measure first, fill second:
//   k_tbx<false>   a workgroup of 256 owns a span of 4096 bytes, 16 per lane in one load (k_parse_len's scheme, mdk_parse_core.h's word
//                  arithmetic for the newlines; nothing past `bytes` is read).  Line starts are counted and scanned, and go into a list in LDS
//                  that is worked off in rounds of 256: one lane per line parses from the LDS copy of the span plus 512 bytes of look-ahead
//                  (tbx_line).  An entry then needs the entry before it: the lane walks back over the text in global memory -- the line
//                  before its own, further over `meta` lines -- and parses that line as well (the same cache lines its neighbours read); at
//                  the piece's first byte the entry before is the carried line, the last entry of the pieces before, kept on the device.
//                  tbx_flags says whether the entry leaves a record (it starts a run, begins a name, or lies above the leaf bins).  A refused
//                  line leaves (offset << 8 | code) in a 64-bit atomicMin.  The workgroup's counts -- lines, entries, records, names -- go
//                  to a table
//   k_tbx_scan     the exclusive scan of that table (one workgroup) and the totals
//   k_tbx<true>    the same again; every record is written at its scanned place (measured counts are the capacity: a text that changed in
//                  between sets a flag and never writes past them), a name's bytes in a slot of 256.  The lane of the piece's last entry
//                  copies its line into the other carry buffer
// The host keeps the rest small: records are few next to the lines (a run of a human CpG table is a 16 kb window's rows) unless bins
// alternate line by line, which is why they are measured.  tbx_builder (host) joins them across pieces, and md_index_finish lays the payload out.
// Only vector stores and plain C++ in the kernels.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include "mdk_index.h"
#include "mdk_parse_core.h"
#include "mdk_tabix_core.h"

#define TBX_WG 256
static_assert(TBX_SPAN == TBX_WG * TBX_LANE && TBX_SPAN == PARSE_SPAN && TBX_LANE == PARSE_LANE, "a span is 16 bytes per lane");

struct TbxStatus { unsigned long long refusal, last_end, newlines; uint32_t tot[4]; uint32_t changed, carry_len, skip_left; uint32_t pad; long long skip_rel; };

struct KTbx {
    const uint8_t *text; int64_t bytes, offset, skip_rel;
    tbx_conf cf;
    uint4 *btot, *boff; TbxStatus *st;
    const uint8_t *carry_in; uint32_t carry_len; uint64_t prev_last_end; uint8_t *carry_out;
    tbx_rec *recs; uint8_t *names; uint32_t cap_recs, cap_names, n_entries;
};

__device__ __forceinline__ uint32_t tbx_wg_scan(uint32_t v, uint32_t *wsum, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t x = v;
    for(uint32_t d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d, 64); if(lane >= d) x += y; }
    __syncthreads();                                            // (the sums of the scan before this one have been read)
    if(lane == 63) wsum[w] = x;
    __syncthreads();
    uint32_t base = 0;
    for(uint32_t i = 0; i < w; i++) base += wsum[i];
    total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return base + x - v;
}

__device__ __forceinline__ uint4 tbx_quad(const KTbx &K, int64_t at) {
    if(at + TBX_LANE <= K.bytes) return *(const uint4 *)(K.text + at);
    uint32_t w[4] = {0, 0, 0, 0};
    for(int i = 0; i < 16; i++) if(at + i < K.bytes) w[i >> 2] |= (uint32_t)K.text[at + i] << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the entry before the line that starts at byte `pos` of the piece: its line, its fields and where its line ends
__device__ __forceinline__ bool tbx_prev(const KTbx &K, int64_t pos, const uint8_t *&pp, tbx_entry &pe, uint64_t &prev_end) {
    for(;;) {
        if(pos == 0) {
            if(!K.carry_len) return false;
            pp = K.carry_in; prev_end = K.prev_last_end;
            return tbx_line(pp, (int64_t)K.carry_len, false, K.cf, pe) == 0;
        }
        int64_t ps = pos - 1; uint32_t n = 0;                   // (byte pos - 1 is the newline)
        while(ps > 0 && K.text[ps - 1] != '\n' && n < TBX_MAX_LINE) { ps--; n++; }
        if(ps < K.skip_rel || n >= TBX_MAX_LINE) return false;  // one of the skipped lines, or a line that is refused where it stands
        const int rc = tbx_line(K.text + ps, K.bytes - ps, false, K.cf, pe);
        if(rc == 0) { pp = K.text + ps; prev_end = (uint64_t)(K.offset + pos); return true; }
        if(rc > 0) return false;                                // (refused where it stands, and earlier than this line)
        pos = ps;                                               // a meta line: further back
    }
}

template<bool FILL> __global__ __launch_bounds__(TBX_WG) void k_tbx(const KTbx K) {
    __shared__ __attribute__((aligned(16))) uint8_t img[TBX_SPAN + TBX_MAX_LINE];
    __shared__ uint16_t list[TBX_SPAN];
    __shared__ uint32_t wsum[4];
    const uint32_t t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * TBX_SPAN, at0 = base + TBX_LANE * t;
    const uint4 q = tbx_quad(K, at0);
    *(uint4 *)(img + TBX_LANE * t) = q;
    for(uint32_t k = t; k < TBX_MAX_LINE / TBX_LANE; k += TBX_WG) {
        const int64_t a = base + TBX_SPAN + TBX_LANE * k;
        *(uint4 *)(img + TBX_SPAN + TBX_LANE * k) = a < K.bytes ? tbx_quad(K, a) : make_uint4(0, 0, 0, 0);
    }
    const uint32_t nl = prs_newlines(q.x, q.y, q.z, q.w);
    const uint32_t below = __shfl_up(nl >> 15, 1, 64);          // (every lane of the wavefront takes part)
    bool prev_nl = (below & 1u) != 0;
    if((t & 63u) == 0) prev_nl = at0 == 0 || (at0 <= K.bytes && K.text[at0 - 1] == '\n');
    const uint32_t starts = prs_starts(nl, prev_nl, at0, K.bytes);
    uint32_t total;
    {
        uint32_t j = tbx_wg_scan((uint32_t)__popc(starts), wsum, total);
        for(uint32_t m = starts; m; m &= m - 1) list[j++] = (uint16_t)(TBX_LANE * t + (uint32_t)__ffs(m) - 1u);
    }
    __syncthreads();
    uint4 off = make_uint4(0, 0, 0, 0);
    if(FILL) off = K.boff[blockIdx.x];
    uint32_t run_e = 0, run_r = 0, run_n = 0;
    for(uint32_t r0 = 0; r0 < total; r0 += TBX_WG) {
        const uint32_t r = r0 + t;
        uint32_t fl = 0; bool entry = false; int64_t at = 0; uint32_t s = 0;
        tbx_entry e, pe; uint64_t prev_end = 0;
        if(r < total) {
            s = list[r]; at = base + s;
            int rc = tbx_line(img + s, K.bytes - at, at < K.skip_rel, K.cf, e);
            if(rc == 0) {
                const uint8_t *pp = nullptr; bool unordered;
                const bool have = tbx_prev(K, at, pp, pe, prev_end);
                fl = tbx_flags(have, pp, pe, img + s, e, unordered);
                if(!have) prev_end = 0;
                if(unordered) rc = TBX_E_ORDER;
                entry = true;
            }
            if(rc > 0 && !FILL) atomicMin(&K.st->refusal, ((unsigned long long)(K.offset + at) << 8) | (unsigned long long)rc);
        }
        uint32_t sum;
        const uint32_t ex = tbx_wg_scan((entry ? 1u : 0u) | (fl ? 1u << 10 : 0u) | (fl & TBX_F_NAME ? 1u << 20 : 0u), wsum, sum);
        if(FILL && entry) {
            const uint32_t ord = off.y + run_e + (ex & 1023u);
            if(fl) {
                const uint32_t ri = off.z + run_r + (ex >> 10 & 1023u);
                if(ri < K.cap_recs) {
                    tbx_rec x;
                    x.begin = (uint64_t)(K.offset + at); x.prev_end = prev_end; x.bin = e.bin; x.beg0 = e.beg0; x.end0 = e.end0; x.flags = fl; x.ord = ord; x.name_len = e.name_len;
                    K.recs[ri] = x;
                } else K.st->changed = 1;
                if(fl & TBX_F_NAME) {
                    const uint32_t ni = off.w + run_n + (ex >> 20 & 1023u);
                    if(ni < K.cap_names) { uint8_t *d = K.names + (size_t)ni * TBX_NAME_SLOT; for(uint32_t i = 0; i < e.name_len; i++) d[i] = img[s + e.name_off + i]; }
                    else K.st->changed = 1;
                }
            }
            if(ord + 1 == K.n_entries) {                        // the piece's last entry: the entry before the next piece's first
                for(uint32_t i = 0; i < e.line_len; i++) K.carry_out[i] = img[s + i];
                K.st->carry_len = e.line_len;
                const int64_t end = at + e.line_len;
                K.st->last_end = (unsigned long long)(K.offset + (end < K.bytes ? end + 1 : end));
            }
        }
        run_e += sum & 1023u; run_r += sum >> 10 & 1023u; run_n += sum >> 20 & 1023u;
    }
    if(!FILL && t == 0) K.btot[blockIdx.x] = make_uint4(total, run_e, run_r, run_n);
}

// the exclusive scan of the workgroups' counts: a lane takes a stretch of them
__global__ __launch_bounds__(TBX_WG) void k_tbx_scan(const uint4 *btot, uint4 *boff, TbxStatus *st, uint32_t nb) {
    __shared__ uint32_t wsum[4];
    const uint32_t per = (nb + TBX_WG - 1) / TBX_WG, b0 = threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    uint32_t mine[4] = {0, 0, 0, 0}, start[4], tot[4];
    for(uint32_t b = b0; b < b1; b++) { const uint4 v = btot[b]; mine[0] += v.x; mine[1] += v.y; mine[2] += v.z; mine[3] += v.w; }
    for(int k = 0; k < 4; k++) start[k] = tbx_wg_scan(mine[k], wsum, tot[k]);
    for(uint32_t b = b0; b < b1; b++) {
        const uint4 v = btot[b];
        boff[b] = make_uint4(start[0], start[1], start[2], start[3]);
        start[0] += v.x; start[1] += v.y; start[2] += v.z; start[3] += v.w;
    }
    if(threadIdx.x == 0) for(int k = 0; k < 4; k++) st->tot[k] = tot[k];
}

// where the lines that are skipped end in this piece: one lane, for the one or two header lines of a file
__global__ void k_tbx_skip(const uint8_t *text, int64_t bytes, TbxStatus *st) {
    uint32_t left = st->skip_left; int64_t i = 0;
    while(left && i < bytes) { if(text[i] == '\n') left--; i++; }
    st->skip_left = left; st->skip_rel = left ? bytes : i;
}

// the newlines of text[0, n): the line number of a refusal
__global__ __launch_bounds__(TBX_WG) void k_tbx_newlines(const uint8_t *text, int64_t n, TbxStatus *st) {
    unsigned long long c = 0;
    for(int64_t i = (int64_t)blockIdx.x * TBX_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * TBX_WG) c += text[i] == '\n';
    if(c) atomicAdd(&st->newlines, c);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
#define SIDE_ERR_ARG MD_INDEX_ERR_ARG
#define SIDE_ERR_HIP MD_INDEX_ERR_HIP
#define SIDE_ERR_NOMEM MD_INDEX_ERR_NOMEM
#include "mdk_side.hpp"
extern "C" const char *md_index_last_error(void) { return g_err; }

struct md_index : SideStream {
    tbx_builder B;
    TbxStatus *d_st = nullptr; TbxStatus h_st;
    SideBuf<uint4> d_btot, d_boff; SideBuf<tbx_rec> d_recs; SideBuf<uint8_t> d_names;
    uint8_t *d_carry = nullptr; int cur = 0; uint32_t carry_len = 0;
    int64_t offset = 0, lines = 0, entries = 0, records = 0, names = 0, pieces = 0;
    uint64_t last_end = 0; uint32_t skip_left = 0;
    bool open_tail = false, refused = false, finished = false;
    int64_t refused_line = 0; int refused_code = 0;
    std::vector<uint8_t> payload;
};

// room for what a piece asks and a quarter more
template <class T> static int reserve(SideBuf<T> &b, uint32_t want, const char *what) { return b.need(want, (size_t)want + want / 4 + 64, what); }

extern "C" int md_index_open(int device, const md_index_conf *conf, md_index **out) {
    if(!conf || !out || conf->col_seq < 1 || conf->col_beg < 1 || conf->col_end < 1 || conf->col_seq > 64 || conf->col_beg > 64 || conf->col_end > 64 || conf->skip < 0 ||
       conf->meta < 0 || conf->meta > 255 || (conf->format & ~TBX_UCSC) != 0)
        return fail(MD_INDEX_ERR_ARG, "md_index_open: columns from 1 to 64, meta a byte, skip not negative, format 0 or 0x10000", hipSuccess);
    *out = nullptr;
    SIDECHK(hipSetDevice(device));
    md_index *h = new md_index();
    h->skip_left = (uint32_t)conf->skip;
    h->B.cf = tbx_conf{conf->format, conf->col_seq, conf->col_beg, conf->col_end, conf->meta, conf->skip};
    hipError_t e = h->open(device);
    if(e == hipSuccess) e = hipMalloc((void **)&h->d_st, sizeof(TbxStatus));
    if(e == hipSuccess) e = hipMalloc((void **)&h->d_carry, 2 * TBX_MAX_LINE);
    if(e != hipSuccess) { md_index_close(h); return fail(MD_INDEX_ERR_NOMEM, "md_index_open", e); }
    *out = h;
    return 0;
}

extern "C" void md_index_close(md_index *h) {
    if(!h) return;
    h->close();
    (void)hipFree(h->d_st); h->d_btot.release(); h->d_boff.release(); h->d_recs.release(); h->d_names.release(); (void)hipFree(h->d_carry);
    delete h;
}

extern "C" int md_index_feed(md_index *h, const void *d_text, int64_t bytes) {
    const char *const what = "md_index_feed";
    if(!h || bytes < 0 || bytes > (int64_t)INT32_MAX || (bytes && !d_text)) return fail(MD_INDEX_ERR_ARG, what, hipSuccess);
    if(h->refused || h->finished) return fail(MD_INDEX_ERR_ARG, "md_index_feed: the handle is refused or finished", hipSuccess);
    if(!bytes) return 0;
    if((uintptr_t)d_text & 15u) return fail(MD_INDEX_ERR_ARG, "md_index_feed: the text must be 16-byte aligned", hipSuccess);
    if(h->open_tail) return fail(MD_INDEX_ERR_ARG, "md_index_feed: the piece before this one did not end at a line's end", hipSuccess);
    SIDECHK(hipSetDevice(h->device));
    const uint32_t nb = (uint32_t)((bytes + TBX_SPAN - 1) / TBX_SPAN);
    { const int rc = reserve(h->d_btot, nb, "hipMalloc(block table)"); if(rc) return rc; }
    { const int rc = reserve(h->d_boff, nb, "hipMalloc(block offsets)"); if(rc) return rc; }
    memset(&h->h_st, 0, sizeof h->h_st);
    h->h_st.refusal = ~0ull; h->h_st.skip_left = h->skip_left;
    SIDECHK(hipMemcpyAsync(h->d_st, &h->h_st, sizeof(TbxStatus), hipMemcpyHostToDevice, h->st));
    KTbx K;
    memset(&K, 0, sizeof K);
    K.text = (const uint8_t *)d_text; K.bytes = bytes; K.offset = h->offset; K.cf = h->B.cf; K.btot = h->d_btot; K.boff = h->d_boff; K.st = h->d_st;
    K.carry_in = h->d_carry + (size_t)h->cur * TBX_MAX_LINE; K.carry_out = h->d_carry + (size_t)(h->cur ^ 1) * TBX_MAX_LINE; K.carry_len = h->carry_len; K.prev_last_end = h->last_end;
    if(h->skip_left) {
        hipLaunchKernelGGL(k_tbx_skip, dim3(1), dim3(1), 0, h->st, K.text, bytes, h->d_st);
        SIDECHK(hipGetLastError());
        SIDECHK(hipMemcpyAsync(&h->h_st, h->d_st, sizeof(TbxStatus), hipMemcpyDeviceToHost, h->st));
        SIDECHK(hipStreamSynchronize(h->st));
        K.skip_rel = h->h_st.skip_rel; h->skip_left = h->h_st.skip_left;
    }
    hipLaunchKernelGGL(k_tbx<false>, dim3(nb), dim3(TBX_WG), 0, h->st, K);
    hipLaunchKernelGGL(k_tbx_scan, dim3(1), dim3(TBX_WG), 0, h->st, (const uint4 *)h->d_btot, h->d_boff, h->d_st, nb);
    SIDECHK(hipGetLastError());
    SIDECHK(hipMemcpyAsync(&h->h_st, h->d_st, sizeof(TbxStatus), hipMemcpyDeviceToHost, h->st));
    SIDECHK(hipStreamSynchronize(h->st));
    const uint32_t n_lines = h->h_st.tot[0], n_entries = h->h_st.tot[1], n_recs = h->h_st.tot[2], n_names = h->h_st.tot[3];
    unsigned long long refusal = h->h_st.refusal;
    std::vector<tbx_rec> recs(n_recs); std::vector<uint8_t> names((size_t)n_names * TBX_NAME_SLOT);
    if(n_entries) {
        { const int rc = reserve(h->d_recs, n_recs, "hipMalloc(records)"); if(rc) return rc; }
        { const int rc = reserve(h->d_names, n_names * TBX_NAME_SLOT, "hipMalloc(names)"); if(rc) return rc; }
        K.recs = h->d_recs; K.names = h->d_names; K.cap_recs = n_recs; K.cap_names = n_names; K.n_entries = n_entries;
        hipLaunchKernelGGL(k_tbx<true>, dim3(nb), dim3(TBX_WG), 0, h->st, K);
        SIDECHK(hipGetLastError());
        if(n_recs) SIDECHK(hipMemcpyAsync(recs.data(), h->d_recs, (size_t)n_recs * sizeof(tbx_rec), hipMemcpyDeviceToHost, h->st));
        if(n_names) SIDECHK(hipMemcpyAsync(names.data(), h->d_names, names.size(), hipMemcpyDeviceToHost, h->st));
        SIDECHK(hipMemcpyAsync(&h->h_st, h->d_st, sizeof(TbxStatus), hipMemcpyDeviceToHost, h->st));
        SIDECHK(hipStreamSynchronize(h->st));
        if(h->h_st.changed) return fail(MD_INDEX_ERR_ARG, "md_index_feed: the text is not the one that was measured", hipSuccess);
        uint32_t ni = 0;
        for(uint32_t i = 0; i < n_recs; i++) {
            const uint8_t *nm = nullptr;
            if(recs[i].flags & TBX_F_NAME) { if(ni >= n_names) return fail(MD_INDEX_ERR_ARG, "md_index_feed: the text is not the one that was measured", hipSuccess); nm = names.data() + (size_t)ni++ * TBX_NAME_SLOT; }
            h->B.add(recs[i], (uint64_t)h->entries + recs[i].ord, nm);
        }
        if(h->B.returned >= 0) { const unsigned long long key = (unsigned long long)h->B.returned << 8 | TBX_E_RETURN; if(key < refusal) refusal = key; }
    }
    if(refusal != ~0ull) {
        const int64_t rel = (int64_t)(refusal >> 8) - h->offset;          // the refused line starts here in this piece
        h->h_st.newlines = 0;
        SIDECHK(hipMemcpyAsync(h->d_st, &h->h_st, sizeof(TbxStatus), hipMemcpyHostToDevice, h->st));
        if(rel > 0) hipLaunchKernelGGL(k_tbx_newlines, dim3((uint32_t)((rel + 65535) / 65536)), dim3(TBX_WG), 0, h->st, K.text, rel, h->d_st);
        SIDECHK(hipGetLastError());
        SIDECHK(hipMemcpyAsync(&h->h_st, h->d_st, sizeof(TbxStatus), hipMemcpyDeviceToHost, h->st));
        SIDECHK(hipStreamSynchronize(h->st));
        h->refused = true; h->refused_line = h->lines + (int64_t)h->h_st.newlines + 1; h->refused_code = (int)(refusal & 0xff);
        if(h->refused_code == TBX_E_RETURN) snprintf(g_err, sizeof g_err, "line %lld: not sorted: contig %s appears in two places", (long long)h->refused_line, h->B.returned_name.c_str());
        else snprintf(g_err, sizeof g_err, "line %lld: %s", (long long)h->refused_line, tbx_error_text(h->refused_code));
        return MD_INDEX_REFUSED;
    }
    if(n_entries) { h->cur ^= 1; h->carry_len = h->h_st.carry_len; h->last_end = h->h_st.last_end; }
    {
        uint8_t last = 0;
        SIDECHK(hipMemcpy(&last, K.text + bytes - 1, 1, hipMemcpyDeviceToHost));
        h->open_tail = last != '\n';
    }
    h->offset += bytes; h->lines += n_lines; h->entries += n_entries; h->records += n_recs; h->names += n_names; h->pieces++;
    return 0;
}

extern "C" int md_index_refusal(const md_index *h, int64_t *line, int *code) {
    if(!h || !h->refused) return fail(MD_INDEX_ERR_ARG, "md_index_refusal: nothing was refused", hipSuccess);
    if(line) *line = h->refused_line;
    if(code) *code = h->refused_code;
    return 0;
}

extern "C" int md_index_finish(md_index *h, const md_index_member *members, int64_t n_members, uint64_t c_end, int64_t *payload_bytes) {
    if(!h || !payload_bytes || n_members < 0 || (n_members && !members) || h->refused || h->finished) return fail(MD_INDEX_ERR_ARG, "md_index_finish", hipSuccess);
    std::vector<tbx_member> m((size_t)n_members);
    uint64_t u = 0;
    for(int64_t i = 0; i < n_members; i++) {
        if(members[i].u_off != u || !members[i].isize || members[i].isize > 65536 || (i && members[i].c_off <= members[i - 1].c_off))
            return fail(MD_INDEX_ERR_ARG, "md_index_finish: the members must hold bytes, follow each other and cover the text", hipSuccess);
        m[(size_t)i] = tbx_member{members[i].c_off, members[i].u_off, members[i].isize};
        u += members[i].isize;
    }
    if(u != (uint64_t)h->offset) return fail(MD_INDEX_ERR_ARG, "md_index_finish: the members do not hold as many bytes as the text that was fed", hipSuccess);
    h->B.finish(h->last_end, (uint64_t)h->entries);
    h->payload = h->B.payload(m, c_end);
    h->finished = true;
    *payload_bytes = (int64_t)h->payload.size();
    return 0;
}

extern "C" int md_index_payload(md_index *h, void *dst, int64_t bytes) {
    if(!h || !h->finished || !dst || bytes != (int64_t)h->payload.size()) return fail(MD_INDEX_ERR_ARG, "md_index_payload: md_index_finish first, then a buffer of exactly its size", hipSuccess);
    memcpy(dst, h->payload.data(), h->payload.size());
    return 0;
}

extern "C" int64_t md_index_count(const md_index *h, int which) {
    if(!h) return -1;
    return which == 0 ? h->lines : which == 1 ? h->entries : which == 2 ? h->records : which == 3 ? h->names : which == 4 ? h->pieces : -1;
}
