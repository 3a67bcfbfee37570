// mdk_bigwig.hip -- libmdk_track.so (include/mdk_track.h): a table of calls as a bigWig track, made on the device.  The rule -- the file byte
// by byte -- is mdk_bigwig_core.h's; a section's compression is the rule of mdk_deflate_core.h.  The host build of the same decomposition is
// tools/bigwig_emu, and the file made here must equal its file.  A library of its own, as mdk_tabix.hip's and mdk_qdiff.hip's are -- one
// code object, its own stream, its own pinned status block, its own error text -- that links nothing of libmdk_hip.so.
//
// md_track_bigwig_measure does all of the device work, in this order (every kernel walks its work with a grid-stride loop):
//   k_bw_check     a lane per row: bw_row_check, bw_pair_check with the row before; the smallest (row << 8 | code) by one 64-bit atomicMin
//                  (an overlap names the earlier row); every contig's first and last row.  A refusal ends the call here
//   k_bw_zoom0     a lane per level-0 bin (bw_zoom0: a binary search into the contig's rows, then the bin's rows in order)
//   k_bw_zoomk     a lane per bin of level k = 1 .. 7, from its up to four children
//   k_bw_count     a workgroup per chunk of 256 bins: the chunk's non-empty bins, for every level
//   k_bw_scan      a workgroup per level: the chunks' counts into their exclusive sums, in place; the level's record count
//   k_bw_records   (written levels) a workgroup per chunk: every non-empty bin's bw_zoom_record at its rank.  A level's records lie one
//                  behind the other from a 16 KiB boundary, and 512 records are 16 KiB: they ARE the level's raw sections, BW_RAW_STRIDE apart
//   then, in batches of a fixed number of sections (data sections first, then the written levels' in ascending order):
//   k_bw_sections  a workgroup per data section: the 24-byte header and 12 bytes a row, BW_RAW_STRIDE apart, and the section's bounds
//   k_bw_zlib      ONE WAVEFRONT PER SECTION, data and zoom alike, into a slot of BW_SLOT bytes: 78 9C, the raw deflate stream, the
//                  Adler-32 from bw_adler_lane sums; a zoom section's bounds from its first and last record
//   k_bw_offsets   one workgroup: the batch's sizes as offsets into the packed store, and their sum
//   k_bw_pack      a workgroup per section: the slot's bytes to their place in the packed store
// The host runs bw_plan_levels between the scan and the records, adds level 7's bins to the total summary (bw_total_add, ascending), takes
// 4 + 16 bytes per section back and runs bw_make_layout.  The file is then the host-made pieces (uploaded once) plus 1 + levels regions of
// the packed store (bw_make_regions); md_track_bigwig_fill_range maps a byte range onto them with bw_cut_range and copies on the device.
// Memory: the bins of all eight levels (32 bytes a bin), a 4-byte count per 256 bins, the written levels' records (at most a record a
// bin), the packed store (the file's own bytes), 24 bytes per section, and per BATCH 16 KiB of raw section and one slot a section, with
// 64 KiB of tokens per workgroup at work: nothing but the file's bytes grows with the row count.  Every buffer hangs on the handle and
// grows with the largest input seen.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "mdk_track.h"
#include "mdk_bigwig_core.h"
#include "mdk_deflate_core.h"

#define BW_WG 256
#define BW_CHUNK 256u                      // bins whose non-empty ones one workgroup counts and ranks at a time
#define BW_BATCH 4096
#define BW_E_SLOT 1u                       // a section left its slot or is longer than its stored form: never, by the sizes counted in dfl_choose

struct TrackStatus { unsigned long long first; uint32_t err, pad; long long zcount[BW_LEVELS]; long long batch_bytes; };

struct KTrack {
    const int32_t *contig, *start, *end, *m, *u; uint32_t n; int32_t n_contigs; int mode;
    const uint32_t *len; uint32_t *first, *last;                   // per contig: its length, its rows [first, last)
    const uint32_t *base[BW_LEVELS]; uint32_t bins_n[BW_LEVELS];   // base[k][c]: the first bin of contig c in level k's table; bins_n[k]: the table's bins
    bw_bin *bins[BW_LEVELS];
    uint32_t *chunk[BW_LEVELS]; uint32_t chunks_n[BW_LEVELS];      // per chunk of a level: its non-empty bins, after k_bw_scan those of the chunks before it
    uint32_t *rec;                                                 // the written levels' records
    uint64_t rec_at[BW_LEVELS]; uint32_t rec_n[BW_LEVELS];         // level k's records begin at record rec_at[k] (a multiple of 512) and are rec_n[k]
    const uint32_t *sec_base; uint32_t n_data;                     // sec_base[c]: the first data section of contig c
    uint32_t zsec_at[BW_LEVELS + 1];                               // the first section of level k in the list; unwritten levels have none
    uint8_t *raw, *slots; uint32_t *tok; long long *off;           // the batch's raw data sections, slots, token strips (per workgroup) and store offsets
    uint32_t *size; bw_entry *entry;                               // per section of the list
    uint8_t *store; long long store_at;                            // the packed store; where the batch begins in it
    uint32_t b0, b1;                                               // the batch: sections [b0, b1) of the list
    int level;
    TrackStatus *st;
};

// ---- rows ----
__global__ __launch_bounds__(BW_WG) void k_bw_check(const KTrack K) {
    for(uint64_t i64 = (uint64_t)blockIdx.x * BW_WG + threadIdx.x; i64 < K.n; i64 += (uint64_t)gridDim.x * BW_WG) {
        const uint32_t i = (uint32_t)i64;
        const int32_t c = K.contig[i], s = K.start[i], e = K.end[i];
        unsigned long long key = ~0ull;
        const uint32_t code = bw_row_check(K.mode, K.n_contigs, K.len, c, s, e, K.m[i], K.u[i]);
        if(code) key = (unsigned long long)i << 8 | code;
        int32_t before = -1;
        if(i) {
            before = K.contig[i - 1];
            const uint32_t pair = bw_pair_check(before, K.start[i - 1], K.end[i - 1], c, s);
            const unsigned long long k2 = (unsigned long long)(pair == BW_E_OVERLAP ? i - 1 : i) << 8 | pair;
            if(pair && k2 < key) key = k2;
        }
        if(key != ~0ull) atomicMin(&K.st->first, key);
        if(c < 0 || c >= K.n_contigs) continue;
        if(!i || before != c) K.first[c] = i;                      // (rows in order: one writer per contig; out of order the call is refused)
        if(i == K.n - 1 || K.contig[i + 1] != c) K.last[c] = i + 1;
    }
}

// ---- zoom ----
__global__ __launch_bounds__(BW_WG) void k_bw_zoom0(const KTrack K) {
    const uint32_t T = K.bins_n[0];
    for(uint64_t x64 = (uint64_t)blockIdx.x * BW_WG + threadIdx.x; x64 < T; x64 += (uint64_t)gridDim.x * BW_WG) {
        const uint32_t x = (uint32_t)x64, c = bw_find_contig(K.base[0], (uint32_t)K.n_contigs, x);
        bw_bin b;
        bw_zoom0(b, K.mode, K.start, K.end, K.m, K.u, K.first[c], K.last[c], x - K.base[0][c], K.len[c]);
        K.bins[0][x] = b;
    }
}

__global__ __launch_bounds__(BW_WG) void k_bw_zoomk(const KTrack K) {
    const int k = K.level;
    const uint32_t T = K.bins_n[k];
    for(uint64_t x64 = (uint64_t)blockIdx.x * BW_WG + threadIdx.x; x64 < T; x64 += (uint64_t)gridDim.x * BW_WG) {
        const uint32_t x = (uint32_t)x64, c = bw_find_contig(K.base[k], (uint32_t)K.n_contigs, x), bin = x - K.base[k][c];
        const uint32_t kid0 = K.base[k - 1][c], kids = K.base[k - 1][c + 1] - kid0;
        bw_bin b;
        bw_bin_clear(b);
        for(uint32_t j = 0; j < 4; j++) { const uint64_t cb = 4ull * bin + j; if(cb >= kids) break; bw_bin_child(b, K.bins[k - 1][kid0 + (uint32_t)cb]); }
        K.bins[k][x] = b;
    }
}

__global__ __launch_bounds__(BW_WG) void k_bw_count(const KTrack K) {
    const int k = K.level;
    for(uint32_t ch = blockIdx.x; ch < K.chunks_n[k]; ch += gridDim.x) {
        const uint64_t x = (uint64_t)ch * BW_CHUNK + threadIdx.x;
        const int on = x < K.bins_n[k] && K.bins[k][x].valid != 0;
        const int cnt = __syncthreads_count(on);
        if(threadIdx.x == 0) K.chunk[k][ch] = (uint32_t)cnt;
    }
}

// the workgroup's inclusive sums of v, a value per thread, and their total; `part` holds a value per wavefront
__device__ __forceinline__ unsigned long long block_incl_sum(unsigned long long v, unsigned long long *part, unsigned long long &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for(int d = 1; d < 64; d <<= 1) { const unsigned long long y = __shfl_up(v, d, 64); if(lane >= d) v += y; }
    __syncthreads();                                               // `part` of the call before is read
    if(lane == 63) part[wave] = v;
    __syncthreads();
    unsigned long long before = 0; total = 0;
    for(int w = 0; w < BW_WG / 64; w++) { const unsigned long long p = part[w]; if(w < wave) before += p; total += p; }
    return v + before;
}

// the library's own scan (as k_tbx_scan is mdk_tabix.hip's): workgroup k turns level k's chunk counts into their exclusive sums
__global__ __launch_bounds__(BW_WG) void k_bw_scan(const KTrack K) {
    __shared__ unsigned long long part[BW_WG / 64];
    const int k = blockIdx.x;
    unsigned long long carry = 0;
    for(uint32_t c0 = 0; c0 < K.chunks_n[k]; c0 += BW_WG) {
        const uint32_t ch = c0 + threadIdx.x;
        const unsigned long long v = ch < K.chunks_n[k] ? K.chunk[k][ch] : 0ull;
        unsigned long long total;
        const unsigned long long incl = block_incl_sum(v, part, total);
        if(ch < K.chunks_n[k]) K.chunk[k][ch] = (uint32_t)(carry + incl - v);
        carry += total;
    }
    if(threadIdx.x == 0) K.st->zcount[k] = (long long)carry;
}

__global__ __launch_bounds__(BW_WG) void k_bw_records(const KTrack K) {
    __shared__ unsigned long long part[BW_WG / 64];
    const int k = K.level;
    for(uint32_t ch = blockIdx.x; ch < K.chunks_n[k]; ch += gridDim.x) {
        const uint64_t x64 = (uint64_t)ch * BW_CHUNK + threadIdx.x;
        bw_bin b;
        bw_bin_clear(b);
        if(x64 < K.bins_n[k]) b = K.bins[k][x64];
        unsigned long long total;
        const unsigned long long on = b.valid != 0, incl = block_incl_sum(on, part, total);
        if(!on) continue;                                          // (no barrier follows in this round)
        const uint64_t pos = (uint64_t)K.chunk[k][ch] + incl - 1;
        if(pos >= K.rec_n[k]) { atomicOr(&K.st->err, BW_E_SLOT); continue; }       // never: the counts are these bins'
        const uint32_t x = (uint32_t)x64, c = bw_find_contig(K.base[k], (uint32_t)K.n_contigs, x);
        bw_zoom_record(K.rec + 8 * (K.rec_at[k] + pos), c, x - K.base[k][c], k, K.len[c], b);
    }
}

// ---- sections ----
__global__ __launch_bounds__(BW_WG) void k_bw_sections(const KTrack K) {
    const uint32_t s1 = K.b1 < K.n_data ? K.b1 : K.n_data;
    for(uint32_t s = K.b0 + blockIdx.x; s < s1; s += gridDim.x) {
        const uint32_t c = bw_find_contig(K.sec_base, (uint32_t)K.n_contigs, s);
        const uint32_t r0 = K.first[c] + (s - K.sec_base[c]) * BW_ITEMS, left = K.last[c] - r0, cnt = left < BW_ITEMS ? left : BW_ITEMS;
        uint32_t *const raw = (uint32_t *)(K.raw + (size_t)(s - K.b0) * BW_RAW_STRIDE);
        if(threadIdx.x == 0) {
            const uint32_t s0 = (uint32_t)K.start[r0], e1 = (uint32_t)K.end[r0 + cnt - 1];
            bw_section_header(raw, c, s0, e1, cnt);
            K.entry[s] = bw_entry{c, s0, c, e1};
        }
        for(uint32_t j = threadIdx.x; j < cnt; j += BW_WG) bw_item(raw + 6 + 3 * j, (uint32_t)K.start[r0 + j], (uint32_t)K.end[r0 + j], bw_value(K.mode, K.m[r0 + j], K.u[r0 + j]));
    }
}

// THE COPY: dfl_build_tree and, in k_bw_zlib, the stripe loop and the emission loop are k_deflate's wave orchestration (mdk_deflate.hip),
// which lives in libmdk_hip.so's one device link and cannot be shared from there; its host twin is tools/deflate_walk.h.  All three walk
// the phases of mdk_deflate_core.h, which stays the shared part: a change of the order of phases is made in all three.
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

__device__ __forceinline__ uint32_t wave_incl_sum_u32(uint32_t v, int lane) {
    for(int d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)v, d, 64); if(lane >= d) v += y; }
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    for(int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(64) void k_bw_zlib(const KTrack K) {
    __shared__ dfl_state S;
    const uint32_t lane = threadIdx.x;
    uint32_t *const tok = K.tok + (size_t)blockIdx.x * BW_RAW_STRIDE;
    for(uint32_t sec = K.b0 + blockIdx.x; sec < K.b1; sec += gridDim.x) {
        // the section's raw bytes: a data section of the batch, or 512 records of a written level where k_bw_records left them
        const uint8_t *in; uint32_t n;
        if(sec < K.n_data) {
            in = K.raw + (size_t)(sec - K.b0) * BW_RAW_STRIDE;
            n = 24 + 12 * (((const uint32_t *)in)[5] >> 16);
        } else {
            int k = 0;
            while(k < BW_LEVELS - 1 && sec >= K.zsec_at[k + 1]) k++;
            const uint32_t j = sec - K.zsec_at[k], left = K.rec_n[k] - j * BW_ZITEMS, cnt = left < BW_ZITEMS ? left : BW_ZITEMS;
            in = (const uint8_t *)(K.rec + 8 * (K.rec_at[k] + (uint64_t)j * BW_ZITEMS));
            n = 32 * cnt;
            if(lane == 0) { const uint32_t *r0 = (const uint32_t *)in, *r1 = r0 + 8 * (cnt - 1); K.entry[sec] = bw_entry{r0[0], r0[1], r1[0], r1[2]}; }
        }
        uint8_t *const slot = K.slots + (size_t)(sec - K.b0) * BW_SLOT;
        uint32_t *const slot32 = (uint32_t *)slot;
        __syncthreads();                                           // the previous section's state is done with
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
        const uint32_t mode = S.mode;
        uint32_t stream_bytes;
        if(mode == DFL_MODE_STORED) {
            stream_bytes = 5 + n;                                  // (23 + n <= 16407: inside the slot)
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
                for(uint32_t k = lane; k < nd; k += 64) { const uint32_t d = S.win[k]; if(wd0 + k == 4) S.first_dw = d; else if(wd0 + k < BW_SLOT / 4) slot32[wd0 + k] = d; }
                const uint32_t carry = S.win[nd];
                __syncthreads();
                for(uint32_t k = lane; k < DFL_WIN; k += 64) S.win[k] = k == 0 ? carry : 0u;
                __syncthreads();
            }
            stream_bytes = (bitpos + 7) >> 3;
            const uint32_t wd0 = (DFL_STREAM_BIT0 + bitpos) >> 5, end = 18 + stream_bytes;
            if(wd0 == 4) { if(lane == 0) S.first_dw = S.win[0]; }
            else if(wd0 * 4 + lane < end && wd0 * 4 + lane < BW_SLOT) slot[wd0 * 4 + lane] = (uint8_t)(S.win[0] >> (8 * (lane & 3u)));      // (at most 3 bytes are left)
        }
        // ---- the zlib framing ----
        uint64_t a, b;
        bw_adler_lane(in, n, lane, a, b);
        a = wave_sum_u64(a); b = wave_sum_u64(b);
        const uint32_t adler = bw_adler_finish(a, b, n), len = 2 + stream_bytes + 4;
        __syncthreads();                                           // first_dw is there
        if(BW_SLOT_LEAD + len > BW_SLOT || stream_bytes > 5 + n) { if(lane == 0) { atomicOr(&K.st->err, BW_E_SLOT); K.size[sec] = 0; } continue; }
        if(lane == 0) { slot32[4] = bw_zlib_dword(S.first_dw); K.size[sec] = len; }
        if(lane < 4) slot[18 + stream_bytes + lane] = bw_adler_byte(lane, adler);
    }
}

__global__ __launch_bounds__(BW_WG) void k_bw_offsets(const KTrack K) {
    __shared__ unsigned long long part[BW_WG / 64];
    unsigned long long carry = 0;
    for(uint32_t s0 = K.b0; s0 < K.b1; s0 += BW_WG) {
        const uint32_t s = s0 + threadIdx.x;
        const unsigned long long v = s < K.b1 ? K.size[s] : 0ull;
        unsigned long long total;
        const unsigned long long incl = block_incl_sum(v, part, total);
        if(s < K.b1) K.off[s - K.b0] = K.store_at + (long long)(carry + incl - v);
        carry += total;
    }
    if(threadIdx.x == 0) K.st->batch_bytes = (long long)carry;
}

__global__ __launch_bounds__(BW_WG) void k_bw_pack(const KTrack K) {
    for(uint32_t s = K.b0 + blockIdx.x; s < K.b1; s += gridDim.x) {
        const uint32_t len = K.size[s];
        const uint8_t *const src = K.slots + (size_t)(s - K.b0) * BW_SLOT + BW_SLOT_LEAD; uint8_t *const dst = K.store + K.off[s - K.b0];
        // the destination's aligned dwords from the slot's bytes, the up to 3 bytes before and after them singly (k_deflate_pack's way)
        const uint32_t head = (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3), h = head < len ? head : len, nq = (len - h) >> 2, tail0 = h + 4 * nq;
        if(threadIdx.x < h) dst[threadIdx.x] = src[threadIdx.x];
        for(uint32_t k = threadIdx.x; k < nq; k += BW_WG) ((uint32_t *)(dst + h))[k] = dfl_load32(src + h + 4 * k);
        if(tail0 + threadIdx.x < len) dst[tail0 + threadIdx.x] = src[tail0 + threadIdx.x];
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
#define SIDE_ERR_ARG MD_TRACK_ERR_ARG
#define SIDE_ERR_HIP MD_TRACK_ERR_HIP
#define SIDE_ERR_NOMEM MD_TRACK_ERR_NOMEM
#include "mdk_side.hpp"
extern "C" const char *md_track_last_error(void) { return g_err; }

// the handle's buffers grow with the largest input seen: room for what is asked and an eighth more
template <typename T, bool pinned = false> struct TrackBuf : SideBuf<T, pinned> {
    int need(size_t n, const char *what) { return SideBuf<T, pinned>::need(n, n + n / 8 + 64, what); }
};

struct md_track : SideHandle<TrackStatus> {
    int cus = 64, max_wg = 0, batch = BW_BATCH;
    TrackBuf<uint32_t> meta, chunk, rec, tok, size; TrackBuf<bw_bin> bins; TrackBuf<uint8_t> raw, slots, store, pieces; TrackBuf<long long> off; TrackBuf<bw_entry> entry;
    TrackBuf<uint32_t, true> h_meta, h_size; TrackBuf<bw_bin, true> h_top; TrackBuf<bw_entry, true> h_entry; TrackBuf<uint8_t, true> h_pieces;
    // the measured file
    bool measured = false; bw_layout lay; std::vector<bw_region> regions; std::vector<int64_t> piece_at;
};

extern "C" int md_track_open(int device, md_track **out) {
    return side_open(device, out, "md_track_open", md_track_close, [](md_track *h) {
        if(hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || h->cus < 1) h->cus = 64;
        return hipSuccess; });
}

extern "C" void md_track_close(md_track *h) {
    if(!h) return;
    h->close();
    h->meta.release(); h->chunk.release(); h->rec.release(); h->tok.release(); h->size.release(); h->bins.release(); h->raw.release(); h->slots.release();
    h->store.release(); h->pieces.release(); h->off.release(); h->entry.release();
    h->h_meta.release(); h->h_size.release(); h->h_top.release(); h->h_entry.release(); h->h_pieces.release();
    delete h;
}

extern "C" int md_track_limits(md_track *h, int max_workgroups, int batch_sections) {
    if(!h || max_workgroups < 0 || batch_sections < 0 || batch_sections > 65536) return fail(MD_TRACK_ERR_ARG, "md_track_limits: a handle, workgroups of 0 or more and a batch of 0 to 65536 sections", hipSuccess);
    h->max_wg = max_workgroups; h->batch = batch_sections ? batch_sections : BW_BATCH;
    return 0;
}

// the workgroups of a launch over `blocks` workgroups' worth of work: at most the limit, at least one
static uint32_t grid_of(const md_track *h, uint64_t blocks, int per_cu) {
    const uint64_t cap = h->max_wg ? (uint64_t)h->max_wg : (uint64_t)per_cu * (uint64_t)h->cus;
    const uint64_t g = blocks < cap ? blocks : cap;
    return (uint32_t)(g ? g : 1);
}

// the pieces of a layout as one block on the device: fill_range copies from it
static int upload_pieces(md_track *h, const char *what) {
    size_t bytes = 0;
    h->piece_at.clear();
    for(const bw_piece &p : h->lay.pieces) { h->piece_at.push_back((int64_t)bytes); bytes += p.bytes.size(); }
    int rc;
    if((rc = h->h_pieces.need(bytes, what)) || (rc = h->pieces.need(bytes, what))) return rc;
    for(size_t i = 0; i < h->lay.pieces.size(); i++) memcpy(h->h_pieces.p + h->piece_at[i], h->lay.pieces[i].bytes.data(), h->lay.pieces[i].bytes.size());
    SIDECHK(hipMemcpyAsync(h->pieces.p, h->h_pieces.p, bytes, hipMemcpyHostToDevice, h->st));
    SIDECHK(hipStreamSynchronize(h->st));
    return 0;
}

extern "C" int md_track_bigwig_measure(md_track *h, const int32_t *contig, const int32_t *start, const int32_t *end, const int32_t *nmeth, const int32_t *nunmeth,
                                       int64_t n, int32_t n_contigs, const char *const *names, const int64_t *lengths, int value, int64_t *bytes) {
    const char *const what = "md_track_bigwig_measure";
    if(!h || !bytes || n < 0 || n > BW_MAX_ROWS || n_contigs < 0 || (n_contigs && (!names || !lengths)) || (value != MD_TRACK_PERCENT && value != MD_TRACK_COVERAGE))
        return fail(MD_TRACK_ERR_ARG, what, hipSuccess);
    if(n && (!contig || !start || !end || !nmeth || !nunmeth)) return fail(MD_TRACK_ERR_ARG, what, hipSuccess);
    *bytes = 0;
    h->measured = false;
    const uint32_t nc = (uint32_t)n_contigs;
    std::vector<std::string> name(nc); std::vector<uint32_t> len(nc);
    for(uint32_t c = 0; c < nc; c++) {
        if(!names[c] || lengths[c] < 0 || lengths[c] > 0x7fffffffll) {
            snprintf(g_err, sizeof g_err, "%s: contig %u has no name, or a length outside 0 .. 2^31 - 1", what, c);
            return MD_TRACK_ERR_ARG;
        }
        name[c] = names[c]; len[c] = (uint32_t)lengths[c];
    }
    SIDECHK(hipSetDevice(h->device));
    bool written[BW_LEVELS]; int64_t zcount[BW_LEVELS]; uint64_t zsec[BW_LEVELS];
    for(int k = 0; k < BW_LEVELS; k++) { written[k] = false; zcount[k] = 0; zsec[k] = 0; }
    bw_summary total = {0, 0.0, 0.0, 0.0, 0.0};
    if(!n) {                                                       // the file without sections: no launch
        h->lay = bw_make_layout(name, len, 0, written, zcount, zsec, nullptr, nullptr, 0, total);
        h->regions.clear();
        const int rc = upload_pieces(h, what);
        if(rc) return rc;
        h->measured = true; *bytes = h->lay.total;
        return 0;
    }
    if(!nc) { snprintf(g_err, sizeof g_err, "row 0: %s", bw_error_text(BW_E_ROW)); return MD_TRACK_ERR_ARG; }
    // ---- the tables of the contigs: len, first, last, sec_base, base[0 .. 7], one block of dwords ----
    uint64_t bins_n[BW_LEVELS], bins_all = 0, chunks_n[BW_LEVELS], chunks_all = 0;
    for(int k = 0; k < BW_LEVELS; k++) {
        bins_n[k] = 0;
        for(uint32_t c = 0; c < nc; c++) bins_n[k] += bw_level_bins(len[c], k);
        chunks_n[k] = (bins_n[k] + BW_CHUNK - 1) / BW_CHUNK;
        bins_all += bins_n[k]; chunks_all += chunks_n[k];
    }
    if(bins_n[0] > (uint64_t)BW_MAX_BINS) { snprintf(g_err, sizeof g_err, "%s: the contigs have more than 2^30 bins of 1024 bases", what); return MD_TRACK_ERR_ARG; }
    const size_t o_len = 0, o_first = nc, o_last = 2 * (size_t)nc, o_sec = 3 * (size_t)nc, o_base = o_sec + nc + 1, meta_n = o_base + BW_LEVELS * ((size_t)nc + 1);
    int rc;
    if((rc = h->meta.need(meta_n, what)) || (rc = h->h_meta.need(meta_n, what)) || (rc = h->bins.need((size_t)bins_all, what)) || (rc = h->chunk.need((size_t)chunks_all, what))) return rc;
    uint32_t *const hm = h->h_meta.p;
    memset(hm, 0, meta_n * sizeof(uint32_t));
    for(uint32_t c = 0; c < nc; c++) hm[o_len + c] = len[c];
    for(int k = 0; k < BW_LEVELS; k++) { uint32_t *b = hm + o_base + (size_t)k * (nc + 1); for(uint32_t c = 0; c < nc; c++) b[c + 1] = b[c] + bw_level_bins(len[c], k); }
    KTrack K;
    memset(&K, 0, sizeof K);
    K.contig = contig; K.start = start; K.end = end; K.m = nmeth; K.u = nunmeth; K.n = (uint32_t)n; K.n_contigs = n_contigs; K.mode = value == MD_TRACK_COVERAGE ? BW_VALUE_COVERAGE : BW_VALUE_PERCENT;
    K.len = h->meta.p + o_len; K.first = h->meta.p + o_first; K.last = h->meta.p + o_last; K.sec_base = h->meta.p + o_sec; K.st = h->d_st;
    {
        size_t b_at = 0, c_at = 0;
        for(int k = 0; k < BW_LEVELS; k++) {
            K.base[k] = h->meta.p + o_base + (size_t)k * (nc + 1); K.bins_n[k] = (uint32_t)bins_n[k]; K.bins[k] = h->bins.p + b_at; b_at += (size_t)bins_n[k];
            K.chunk[k] = h->chunk.p + c_at; K.chunks_n[k] = (uint32_t)chunks_n[k]; c_at += (size_t)chunks_n[k];
        }
    }
    memset(h->pin, 0, sizeof(TrackStatus));
    SIDECHK(hipMemcpyAsync(h->meta.p, hm, meta_n * sizeof(uint32_t), hipMemcpyHostToDevice, h->st));
    SIDE_STATUS_UP(h, h->pin, TrackStatus);
    // ---- the rows ----
    hipLaunchKernelGGL(k_bw_check, dim3(grid_of(h, ((uint64_t)n + BW_WG - 1) / BW_WG, 32)), dim3(BW_WG), 0, h->st, K);
    SIDECHK(hipGetLastError());
    SIDECHK(hipMemcpyAsync(h->pin, h->d_st, sizeof(TrackStatus), hipMemcpyDeviceToHost, h->st));
    SIDECHK(hipMemcpyAsync(hm + o_first, h->meta.p + o_first, 2 * (size_t)nc * sizeof(uint32_t), hipMemcpyDeviceToHost, h->st));
    SIDECHK(hipStreamSynchronize(h->st));
    if(h->pin->first != ~0ull) {
        snprintf(g_err, sizeof g_err, "row %llu: %s", h->pin->first >> 8, bw_error_text((uint32_t)(h->pin->first & 0xffu)));
        return MD_TRACK_ERR_ARG;
    }
    uint64_t n_data = 0; uint32_t raw_max = 0;
    for(uint32_t c = 0; c < nc; c++) {
        hm[o_sec + c] = (uint32_t)n_data;
        const uint32_t rows = hm[o_last + c] - hm[o_first + c];
        n_data += (rows + BW_ITEMS - 1) / BW_ITEMS;
        const uint32_t most = rows < BW_ITEMS ? rows : BW_ITEMS;
        if(rows && 24 + 12 * most > raw_max) raw_max = 24 + 12 * most;
    }
    hm[o_sec + nc] = (uint32_t)n_data;
    K.n_data = (uint32_t)n_data;
    SIDECHK(hipMemcpyAsync(h->meta.p + o_sec, hm + o_sec, ((size_t)nc + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, h->st));
    // ---- zoom: all eight levels, their counts ----
    hipLaunchKernelGGL(k_bw_zoom0, dim3(grid_of(h, (bins_n[0] + BW_WG - 1) / BW_WG, 32)), dim3(BW_WG), 0, h->st, K);
    for(int k = 1; k < BW_LEVELS; k++) { K.level = k; hipLaunchKernelGGL(k_bw_zoomk, dim3(grid_of(h, (bins_n[k] + BW_WG - 1) / BW_WG, 32)), dim3(BW_WG), 0, h->st, K); }
    for(int k = 0; k < BW_LEVELS; k++) { K.level = k; hipLaunchKernelGGL(k_bw_count, dim3(grid_of(h, chunks_n[k], 32)), dim3(BW_WG), 0, h->st, K); }
    hipLaunchKernelGGL(k_bw_scan, dim3(BW_LEVELS), dim3(BW_WG), 0, h->st, K);
    SIDECHK(hipGetLastError());
    const size_t top_n = (size_t)bins_n[BW_LEVELS - 1];
    if((rc = h->h_top.need(top_n, what))) return rc;
    SIDECHK(hipMemcpyAsync(h->pin, h->d_st, sizeof(TrackStatus), hipMemcpyDeviceToHost, h->st));
    SIDECHK(hipMemcpyAsync(h->h_top.p, K.bins[BW_LEVELS - 1], top_n * sizeof(bw_bin), hipMemcpyDeviceToHost, h->st));
    SIDECHK(hipStreamSynchronize(h->st));
    for(int k = 0; k < BW_LEVELS; k++) zcount[k] = h->pin->zcount[k];
    bw_plan_levels(n, zcount, written);
    for(size_t x = 0; x < top_n; x++) bw_total_add(total, h->h_top.p[x]);
    // ---- the written levels' records: each level from a multiple of 512 records, so that its sections lie BW_RAW_STRIDE apart ----
    uint64_t rec_all = 0, n_sec = n_data;
    for(int k = 0; k < BW_LEVELS; k++) {
        K.zsec_at[k] = (uint32_t)n_sec; K.rec_at[k] = rec_all; K.rec_n[k] = 0;
        if(!written[k]) continue;
        zsec[k] = ((uint64_t)zcount[k] + BW_ZITEMS - 1) / BW_ZITEMS;
        K.rec_n[k] = (uint32_t)zcount[k];
        rec_all += zsec[k] * BW_ZITEMS; n_sec += zsec[k];
        const uint32_t most = zcount[k] < (int64_t)BW_ZITEMS ? (uint32_t)zcount[k] : BW_ZITEMS;
        if(32 * most > raw_max) raw_max = 32 * most;
    }
    K.zsec_at[BW_LEVELS] = (uint32_t)n_sec;
    // (zsec_at of an unwritten level equals the next one's: k_bw_zlib's search passes over it)
    if((rc = h->rec.need((size_t)rec_all * 8, what))) return rc;
    K.rec = h->rec.p;
    for(int k = 0; k < BW_LEVELS; k++) if(written[k]) { K.level = k; hipLaunchKernelGGL(k_bw_records, dim3(grid_of(h, chunks_n[k], 32)), dim3(BW_WG), 0, h->st, K); }
    SIDECHK(hipGetLastError());
    // ---- the sections, a batch at a time ----
    const uint32_t batch = (uint32_t)h->batch, zgrid = grid_of(h, batch, 5);          // dfl_state is ~29 KiB of LDS: five wavefronts a compute unit
    if((rc = h->size.need((size_t)n_sec, what)) || (rc = h->entry.need((size_t)n_sec, what)) || (rc = h->h_size.need((size_t)n_sec, what)) || (rc = h->h_entry.need((size_t)n_sec, what)) ||
       (rc = h->raw.need((size_t)batch * BW_RAW_STRIDE, what)) || (rc = h->slots.need((size_t)batch * BW_SLOT, what)) || (rc = h->off.need(batch, what)) ||
       (rc = h->tok.need((size_t)zgrid * BW_RAW_STRIDE, what))) return rc;
    K.size = h->size.p; K.entry = h->entry.p; K.raw = h->raw.p; K.slots = h->slots.p; K.off = h->off.p; K.tok = h->tok.p;
    long long store_at = 0;
    for(uint64_t b0 = 0; b0 < n_sec; b0 += batch) {
        const uint64_t b1 = b0 + batch < n_sec ? b0 + batch : n_sec;
        K.b0 = (uint32_t)b0; K.b1 = (uint32_t)b1; K.store_at = store_at;
        if(b0 < n_data) hipLaunchKernelGGL(k_bw_sections, dim3(grid_of(h, (b1 < n_data ? b1 : n_data) - b0, 32)), dim3(BW_WG), 0, h->st, K);
        const uint32_t g = grid_of(h, b1 - b0, 5);
        hipLaunchKernelGGL(k_bw_zlib, dim3(g < zgrid ? g : zgrid), dim3(64), 0, h->st, K);
        hipLaunchKernelGGL(k_bw_offsets, dim3(1), dim3(BW_WG), 0, h->st, K);
        SIDECHK(hipGetLastError());
        SIDE_STATUS_DOWN(h, h->pin, TrackStatus);
        if(h->pin->err) { snprintf(g_err, sizeof g_err, "%s: a section does not fit its slot, or a level's records are not the counted ones", what); return MD_TRACK_ERR_HIP; }
        const long long need = store_at + h->pin->batch_bytes;
        if((size_t)need > h->store.cap) {                          // the store grows and keeps what the batches before left in it
            TrackBuf<uint8_t> bigger;
            if((rc = bigger.need((size_t)need + (size_t)need / 2, what))) return rc;
            hipError_t e = store_at ? hipMemcpyAsync(bigger.p, h->store.p, (size_t)store_at, hipMemcpyDeviceToDevice, h->st) : hipSuccess;
            if(e == hipSuccess) e = hipStreamSynchronize(h->st);
            if(e != hipSuccess) { bigger.release(); return fail(MD_TRACK_ERR_HIP, what, e); }
            h->store.release();
            h->store = bigger;
        }
        K.store = h->store.p;
        hipLaunchKernelGGL(k_bw_pack, dim3(grid_of(h, b1 - b0, 32)), dim3(BW_WG), 0, h->st, K);
        SIDECHK(hipGetLastError());
        store_at = need;
    }
    SIDECHK(hipMemcpyAsync(h->h_size.p, h->size.p, (size_t)n_sec * sizeof(uint32_t), hipMemcpyDeviceToHost, h->st));
    SIDECHK(hipMemcpyAsync(h->h_entry.p, h->entry.p, (size_t)n_sec * sizeof(bw_entry), hipMemcpyDeviceToHost, h->st));
    SIDECHK(hipStreamSynchronize(h->st));
    // ---- the file ----
    h->lay = bw_make_layout(name, len, n_data, written, zcount, zsec, h->h_entry.p, h->h_size.p, raw_max, total);
    h->regions = bw_make_regions(h->lay, n_data, written, zsec, h->h_size.p);
    if((rc = upload_pieces(h, what))) return rc;
    h->measured = true; *bytes = h->lay.total;
    return 0;
}

extern "C" int md_track_bigwig_fill_range(md_track *h, void *d_out, int64_t offset, int64_t bytes) {
    const char *const what = "md_track_bigwig_fill_range";
    if(!h || !h->measured) return fail(MD_TRACK_ERR_ARG, "md_track_bigwig_fill_range: md_track_bigwig_measure first", hipSuccess);
    if(offset < 0 || bytes < 0 || offset > h->lay.total || bytes > h->lay.total - offset || (bytes && !d_out)) return fail(MD_TRACK_ERR_ARG, "md_track_bigwig_fill_range: the range must lie inside the measured file", hipSuccess);
    if(!bytes) return 0;
    SIDECHK(hipSetDevice(h->device));
    int64_t got = 0;
    for(const bw_cut &c : bw_cut_range(h->lay, h->regions, offset, bytes)) {
        const uint8_t *const src = c.piece ? h->pieces.p + h->piece_at[c.index] + c.src : h->store.p + c.src;
        SIDECHK(hipMemcpyAsync((uint8_t *)d_out + c.dst, src, (size_t)c.bytes, hipMemcpyDeviceToDevice, h->st));
        got += c.bytes;
    }
    SIDECHK(hipStreamSynchronize(h->st));
    if(got != bytes) return fail(MD_TRACK_ERR_HIP, "md_track_bigwig_fill_range: the layout's pieces and regions do not cover the range", hipSuccess);
    return 0;
}
