// mdk_deflate.hip -- device bytes compressed into BGZF members on the device (include/mdk_hip.h, "BGZF made on the device"): the encoder
// between k_text_fill, which leaves a block of text on the device, and the single copy of that block to the host.
//
// Member i holds input bytes [65280 i, min(65280 (i + 1), n)), bgzip's cut; every member is a function of its input alone
// (mdk_deflate_core.h has the phases and why no order of lanes changes a byte).  Measure first, fill second, as the text itself:
//   k_deflate_crc   a wavefront per member (four to a workgroup, the tables in LDS): the CRC32 of its input, as k_crc32 checks it on the way in
//   k_deflate       ONE WAVEFRONT PER MEMBER, a workgroup of 64 lanes; workgroup g takes members g, g + grid, ...  The member is compressed
//                   into a slot of its own (64 KiB apart), its tokens pass through a strip of global memory per workgroup (4 bytes per token,
//                   up to one token per input byte: too much for LDS, and read back coalesced).  LDS holds the hash table (16 KiB), the counts,
//                   codes and trees and the output window: ~29 KiB, five wavefronts per CU.  The input is read from global memory as it
//                   lies (a stripe and its sources 30 bytes back are cache hits); a 64 KiB copy in LDS would leave two wavefronts per CU.
//   k_deflate_scan  one workgroup: the members' lengths as int64 offsets, and their sum
//   k_deflate_pack  a workgroup per member: the slot's bytes to their place in the result; one more workgroup writes the EOF member
// The slots, the lengths and the token strips hang on the md_text handle and are kept; they grow with the largest input seen.
#include "mdk_text_internal.hpp"
#include "mdk_deflate_core.h"
#include "mdk_crc32_core.h"

#define DFL_E_SLOT 1u                      // a member left its slot or is longer than its stored form: never, by the sizes counted in dfl_choose
#define DFL_MAX_BYTES ((1ll << 31) - 1)

struct KDeflate {
    const uint8_t *in; int64_t n; uint32_t n_mem, eof;
    uint8_t *slab; uint32_t *tok; uint32_t *crc; uint32_t *len; int64_t *off; const CrcConst *C; TextStatus *st;
    uint8_t *dst; int64_t bytes;
};

template <typename T> struct DflBuf {
    T *p = nullptr; size_t cap = 0;
    int need(size_t n, const char *what) {
        if(n <= cap) return 0;
        release();
        const size_t want = n + n / 8 + 64;
        const hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if(e != hipSuccess) { p = nullptr; return fail(MDK_ERR_NOMEM, what, e); }
        cap = want; return 0;
    }
    void release() { if(p) (void)hipFree(p); p = nullptr; cap = 0; }
};
struct DeflateState {
    DflBuf<uint8_t> slab; DflBuf<uint32_t> tok, crc, len; DflBuf<int64_t> off; CrcConst *d_const = nullptr;
    KDeflate K; bool measured = false; int grid_max = 0;
};

__device__ __forceinline__ uint32_t dfl_member_bytes(const KDeflate &K, uint32_t m) { const int64_t left = K.n - (int64_t)m * DFL_MEMBER; return left < (int64_t)DFL_MEMBER ? (uint32_t)left : DFL_MEMBER; }

#define CRC_WAVES 4
__global__ __launch_bounds__(64 * CRC_WAVES) void k_deflate_crc(const KDeflate K) {
    __shared__ uint32_t T[4][256], Z[4][256]; __shared__ uint32_t lvl[6], p8[17];
    for(int i = threadIdx.x; i < 1024; i += 64 * CRC_WAVES) { (&T[0][0])[i] = (&K.C->T[0][0])[i]; (&Z[0][0])[i] = (&K.C->Z[0][0])[i]; }
    if(threadIdx.x < 6) lvl[threadIdx.x] = K.C->lvl[threadIdx.x];
    if(threadIdx.x < 17) p8[threadIdx.x] = K.C->p8[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t m = blockIdx.x * CRC_WAVES + wave;
    if(m >= K.n_mem) return;
    const uint32_t L = dfl_member_bytes(K, m);
    uint32_t c = crc_lane(T, Z, K.in + (int64_t)m * DFL_MEMBER, L, lane);
#pragma unroll
    for(int l = 0; l < 6; l++) { const uint32_t left = (uint32_t)__shfl((int)c, lane - (1 << l)); c ^= crc_mul(left, lvl[l]); }      // only the last lane of each group of 2^(l+1) matters
    if(lane == 63) K.crc[m] = crc_finish(c, L, p8);
}

__device__ __forceinline__ uint32_t wave_incl_sum_u32(uint32_t v, int lane) {
    for(int d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)v, d, 64); if(lane >= d) v += y; }
    return v;
}

// the code lengths of the alphabet [a0, a0 + nsym) from its counts (mdk_deflate_core.h "codes"); lens of [a0, a0 + nall) are written
__device__ __forceinline__ void dfl_build_tree(dfl_state &S, uint32_t a0, uint32_t nsym, uint32_t nall, uint32_t limit, uint32_t lane) {
    dfl_tree_counts(S, a0, nsym, lane);
    __syncthreads();
    if(lane == 0) dfl_tree_two(S, nsym);
    __syncthreads();
    for(;;) {
        dfl_tree_rank(S, nsym, lane);
        __syncthreads();
        if(lane == 0) dfl_tree_merge(S);
        __syncthreads();
        if(S.maxdepth <= limit) break;
        dfl_tree_halve(S, nsym, lane);
        __syncthreads();
    }
    dfl_tree_clear(S, a0, nall, lane);
    __syncthreads();
    dfl_tree_lens(S, a0, lane);
    __syncthreads();
}

__global__ __launch_bounds__(64) void k_deflate(const KDeflate K) {
    __shared__ dfl_state S;
    const uint32_t lane = threadIdx.x;
    uint32_t *const tok = K.tok + (size_t)blockIdx.x * DFL_MEMBER;
    for(uint32_t mem = blockIdx.x; mem < K.n_mem; mem += gridDim.x) {
        const uint8_t *const in = K.in + (int64_t)mem * DFL_MEMBER;
        const uint32_t n = dfl_member_bytes(K, mem);
        uint8_t *const slot = K.slab + (size_t)mem * DFL_SLOT;
        uint32_t *const slot32 = (uint32_t *)slot;
        __syncthreads();                                           // the previous member's state is done with
        for(uint32_t i = lane; i < DFL_HASH; i += 64) S.head[i] = 0;
        for(uint32_t i = lane; i < DFL_NSYM; i += 64) S.freq[i] = 0;
        __syncthreads();
        // ---- stripes ----
        uint32_t e = 0, ntok = 0;
        for(uint32_t s0 = 0; s0 < n; s0 += 64) {
            dfl_stripe_load(S, in, n, s0, lane);
            __syncthreads();
            const bool skip = e >= s0 + 64;                        // the whole stripe lies inside a match
            uint32_t m = 0;
            if(!skip) m = dfl_stripe_match(S, in, n, s0, e, lane);
            __syncthreads();                                       // every lookup of the stripe is made: its positions may enter the table
            dfl_stripe_enter(S, n, s0, lane);
            if(!skip) {
                uint32_t cur = e - s0; uint64_t sel = 0;           // the greedy walk: uniform, a register read per token
                while(cur < 64 && s0 + cur < n) { sel |= 1ull << cur; cur += (uint32_t)__builtin_amdgcn_readlane((int)m, (int)cur) & 511u; }
                e = s0 + cur;
                if(sel >> lane & 1) tok[ntok + (uint32_t)__popcll(sel & ((1ull << lane) - 1))] = dfl_token(S, in, s0 + lane, m);
                ntok += (uint32_t)__popcll(sel);
            }
            __syncthreads();                                       // the table is settled for the next stripe, and `w` may be rewritten
        }
        if(lane == 0) S.freq[DFL_EOB] = 1;
        __syncthreads();
        // ---- codes and the form ----
        dfl_build_tree(S, DFL_LIT0, 286, 286, 15, lane);
        dfl_build_tree(S, DFL_DIST0, 30, 30, 15, lane);
        if(lane == 0) dfl_rle(S);
        __syncthreads();
        dfl_build_tree(S, DFL_CL0, 19, 19, 7, lane);
        dfl_assign_codes(S, DFL_CL0, 19, lane);
        __syncthreads();
        if(lane == 0) dfl_choose(S, n);
        __syncthreads();
        const uint32_t mode = S.mode, crc = K.crc[mem];
        uint32_t stream_bytes;
        if(mode == DFL_MODE_STORED) {
            stream_bytes = 5 + n;
            if(lane == 0) { S.first_dw = 0x01u << 16 | (n & 255u) << 24; slot[20] = (uint8_t)(n >> 8); slot[21] = (uint8_t)~n; slot[22] = (uint8_t)(~n >> 8); }
            for(uint32_t i = lane; i < n; i += 64) slot[23 + i] = in[i];
        } else {
            dfl_assign_codes(S, DFL_LIT0, 286, lane); dfl_assign_codes(S, DFL_DIST0, 30, lane);
            for(uint32_t k = lane; k < DFL_WIN; k += 64) S.win[k] = 0;
            __syncthreads();
            // ---- emission ----
            const uint32_t nh = dfl_header_items(S), total = nh + ntok + 1;
            uint32_t bitpos = 0;
            for(uint32_t i0 = 0; i0 < total; i0 += 64) {
                const uint32_t i = i0 + lane;
                uint64_t v = 0;
                const uint32_t nb = i < nh ? dfl_header_item(S, i, v) : i < nh + ntok ? dfl_token_bits(S, tok[i - nh], v) : i == nh + ntok ? dfl_token_bits(S, DFL_EOB, v) : 0u;
                const uint32_t incl = wave_incl_sum_u32(nb, (int)lane), run = (uint32_t)__shfl((int)incl, 63);
                const uint32_t abs0 = DFL_STREAM_BIT0 + bitpos, wd0 = abs0 >> 5;
                dfl_win_or(S.win, (abs0 & 31u) + incl - nb, v, nb);
                bitpos += run;
                const uint32_t nd = ((DFL_STREAM_BIT0 + bitpos) >> 5) - wd0;
                __syncthreads();
                for(uint32_t k = lane; k < nd; k += 64) { const uint32_t d = S.win[k]; if(wd0 + k == 4) S.first_dw = d; else if(wd0 + k < DFL_SLOT / 4) slot32[wd0 + k] = d; }
                const uint32_t carry = S.win[nd];
                __syncthreads();
                for(uint32_t k = lane; k < DFL_WIN; k += 64) S.win[k] = k == 0 ? carry : 0u;
                __syncthreads();
            }
            stream_bytes = (bitpos + 7) >> 3;
            const uint32_t wd0 = (DFL_STREAM_BIT0 + bitpos) >> 5, end = 18 + stream_bytes;
            if(wd0 == 4) { if(lane == 0) S.first_dw = S.win[0]; }
            else if(wd0 * 4 + lane < end && wd0 * 4 + lane < DFL_SLOT) slot[wd0 * 4 + lane] = (uint8_t)(S.win[0] >> (8 * (lane & 3u)));      // (at most 3 bytes are left)
        }
        __syncthreads();
        const uint32_t member = 18 + stream_bytes + 8;
        if(member > DFL_SLOT || member > 18 + 5 + n + 8) { if(lane == 0) { atomicOr(&K.st->err, DFL_E_SLOT); K.len[mem] = 0; } continue; }
        if(lane < 5) slot32[lane] = dfl_header_dword(lane, member, S.first_dw);
        if(lane < 8) slot[18 + stream_bytes + lane] = dfl_trailer_byte(lane, crc, n);
        if(lane == 0) K.len[mem] = member;
    }
}

__global__ __launch_bounds__(TEXT_SCAN_WG) void k_deflate_scan(const KDeflate K) {
    __shared__ int64_t wtot[TEXT_SCAN_WG / 64];
    text_scan_blocks(K.len, K.off, K.st, K.n_mem, wtot);
}

__global__ __launch_bounds__(256) void k_deflate_pack(const KDeflate K) {
    const uint32_t m = blockIdx.x;
    if(m == K.n_mem) {                                             // the EOF member, behind the last one
        const int64_t at = K.bytes - 28;
        if(threadIdx.x < 28) K.dst[at + threadIdx.x] = dfl_eof_byte(threadIdx.x);
        return;
    }
    const uint32_t len = K.len[m]; const int64_t off = K.off[m];
    if(off < 0 || off + (int64_t)len > K.bytes - (K.eof ? 28 : 0)) { if(threadIdx.x == 0) atomicOr(&K.st->err, DFL_E_SLOT); return; }
    const uint8_t *const src = K.slab + (size_t)m * DFL_SLOT; uint8_t *const dst = K.dst + off;
    // the destination's aligned dwords from the slot's bytes, the up to 3 bytes before and after them singly
    const uint32_t head = (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3), h = head < len ? head : len, nq = (len - h) >> 2, tail0 = h + 4 * nq;
    if(threadIdx.x < h) dst[threadIdx.x] = src[threadIdx.x];
    for(uint32_t k = threadIdx.x; k < nq; k += 256) ((uint32_t *)(dst + h))[k] = dfl_load32(src + h + 4 * k);
    if(tail0 + threadIdx.x < len) dst[tail0 + threadIdx.x] = src[tail0 + threadIdx.x];
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
void text_deflate_free(md_text *t) {
    DeflateState *s = t->deflate;
    if(!s) return;
    s->slab.release(); s->tok.release(); s->crc.release(); s->len.release(); s->off.release();
    if(s->d_const) (void)hipFree(s->d_const);
    delete s; t->deflate = nullptr;
}

static int deflate_status(md_text *t, const char *what) {
    HIPCHK(hipMemcpyAsync(t->h_st, t->d_st, sizeof(TextStatus), hipMemcpyDeviceToHost, t->st));
    HIPCHK(hipStreamSynchronize(t->st));
    if(!t->h_st->err) return 0;
    snprintf(mdk_err_buf(), MDK_ERR_BYTES, "%s: a member does not fit its slot, or the lengths are not the measured ones", what);
    return MDK_ERR_ARG;
}

extern "C" int md_text_deflate_measure(md_text *t, const uint8_t *d_in, int64_t n, int eof, int64_t *out_bytes) {
    const char *const what = "md_text_deflate_measure";
    if(!t || !out_bytes || n < 0 || n > DFL_MAX_BYTES || (n && !d_in)) return fail(MDK_ERR_ARG, what, hipSuccess);
    *out_bytes = 0;
    HIPCHK(hipSetDevice(t->device));
    if(!t->deflate) t->deflate = new DeflateState();
    DeflateState *s = t->deflate;
    s->measured = false;
    const uint32_t n_mem = (uint32_t)((n + DFL_MEMBER - 1) / DFL_MEMBER);
    if(!s->d_const) {
        CrcConst *C = new CrcConst(); crc_make_const(*C);
        hipError_t e = hipMalloc((void **)&s->d_const, sizeof(CrcConst));
        if(e == hipSuccess) e = hipMemcpy(s->d_const, C, sizeof(CrcConst), hipMemcpyHostToDevice);
        delete C;
        if(e != hipSuccess) { if(s->d_const) (void)hipFree(s->d_const); s->d_const = nullptr; return fail(MDK_ERR_NOMEM, "md_text_deflate_measure: CRC tables", e); }
        int cus = 0;
        if(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device) != hipSuccess || cus < 1) cus = 64;
        s->grid_max = 4 * cus;                                     // wavefronts at work at once: each has a strip of 255 KiB for its tokens
    }
    const uint32_t grid = n_mem < (uint32_t)s->grid_max ? n_mem : (uint32_t)s->grid_max;
    if(n_mem) {
        int rc;
        if((rc = s->slab.need((size_t)n_mem * DFL_SLOT, what)) || (rc = s->tok.need((size_t)grid * DFL_MEMBER, what)) || (rc = s->crc.need(n_mem, what)) ||
           (rc = s->len.need(n_mem, what)) || (rc = s->off.need(n_mem, what))) return rc;
    }
    KDeflate &K = s->K;
    K.in = d_in; K.n = n; K.n_mem = n_mem; K.eof = eof ? 1u : 0u; K.slab = s->slab.p; K.tok = s->tok.p; K.crc = s->crc.p; K.len = s->len.p; K.off = s->off.p;
    K.C = s->d_const; K.st = t->d_st; K.dst = nullptr; K.bytes = 0;
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    if(n_mem) {
        hipLaunchKernelGGL(k_deflate_crc, dim3((n_mem + CRC_WAVES - 1) / CRC_WAVES), dim3(64 * CRC_WAVES), 0, t->st, K);
        hipLaunchKernelGGL(k_deflate, dim3(grid), dim3(64), 0, t->st, K);
        hipLaunchKernelGGL(k_deflate_scan, dim3(1), dim3(TEXT_SCAN_WG), 0, t->st, K);
        HIPCHK(hipGetLastError());
    }
    { const int rc = deflate_status(t, what); if(rc) return rc; }
    K.bytes = (n_mem ? t->h_st->total : 0) + (eof ? 28 : 0);
    s->measured = true;
    *out_bytes = K.bytes;
    return 0;
}

extern "C" int md_text_deflate_fill(md_text *t, void *d_out, int64_t out_bytes) {
    DeflateState *s = t ? t->deflate : nullptr;
    if(!s || !s->measured || out_bytes != s->K.bytes || (out_bytes && !d_out)) return fail(MDK_ERR_ARG, "md_text_deflate_fill: md_text_deflate_measure first, then a buffer of exactly the measured size", hipSuccess);
    s->measured = false;
    if(!out_bytes) return 0;
    HIPCHK(hipSetDevice(t->device));
    KDeflate &K = s->K; K.dst = (uint8_t *)d_out;
    HIPCHK(hipMemsetAsync(t->d_st, 0, sizeof(TextStatus), t->st));
    hipLaunchKernelGGL(k_deflate_pack, dim3(K.n_mem + K.eof), dim3(256), 0, t->st, K);
    HIPCHK(hipGetLastError());
    return deflate_status(t, "md_text_deflate_fill");
}
