// mdk_cohort.hip -- libmdk_cohort.so (include/mdk_cohort.h): a united table as text and back, on the device.  The formats, the refusals
// and their order are mdk_cohort_core.h's.  A library of its own, as mdk_smooth.hip's is: one code object, its own stream, its own pinned
// status block, its own error text, no link to the other libraries.
//
// The counts are [S, n], contiguous along the site axis; a line of text is one site across all samples.  Both directions are that
// transposition, and both go through LDS so that the matrices are read and written along the site axis.
//
// WRITE
//   k_ctext_len   a lane per site loops over the samples (a wavefront's loads run along the site axis): the line's length, the offset of
//                 every block of `sample_block` samples inside its line (uint16 part[block][site]: the fill places a block without walking
//                 the row again), and the first refusal by atomicMin.
//   k_scan64      the lengths into 64-bit offsets: one workgroup, a contiguous run of entries per thread.
//   k_ctext_fill  a workgroup takes work items in a grid-stride loop: (tile of `tile_sites` sites, block of samples), and per tile one more
//                 for the prefixes.  A block's counts are loaded coalesced into LDS (rows padded by one word: a wavefront then reads one
//                 site's samples without a bank conflict).  A wavefront assembles one row's stretch at a time in its image in LDS -- a lane
//                 per sample, a wave prefix sum over the cell widths -- at the offset the destination has inside its 16-byte quad, and
//                 stores it as aligned quads with byte stores at the ragged ends (txt_plan_image).  Prefixes: a lane per row writes its
//                 prefix into the row's slot, sixteen lanes per row store it the same way.
// READ
//   k_cparse_len     a lane per 16 bytes: the line starts of a 4096-byte span counted (prs_newlines, prs_starts).
//   k_cparse_starts  the same walk behind the scan of the counts: every line's first byte.
//   k_cparse_fill    a workgroup takes a tile of consecutive lines, a wavefront one line at a time: its lanes take aligned 16-byte
//                    stretches and count their tabs, a wave prefix sum gives every field its index, and the lane that holds the tab before
//                    a field parses it (coh_field: a bounded look).  Counts go to the tile's stage in LDS, [which][sample][row] with the
//                    row stride odd, and leave along the site axis; a tile has as many rows as 64 KiB of LDS take, 64 at the most.
//   k_cparse_order   a lane per row: strictly ascending behind its predecessor.
// Whatever a text or a table holds, nothing outside the buffers is touched: a stretch outside the text is read byte by byte inside it, a
// field index past the last column is never stored, a refused table is never filled.  Plain C++, vector loads and stores, no atomics but
// the status word's and the span counters' in LDS.
// SUMS OVER INTERVALS (md_cohort_regions) are csrc/mdk_cregion.hip, included at the end of this file: they use this handle's stream, status
// word, contig count and limits, and temporaries of their own beside the ones above.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "mdk_cohort.h"
#include "mdk_cohort_core.h"

#define COH_WG 256
#define COH_WAVES (COH_WG / 64)
#define COH_TILE_DEFAULT 64
#define COH_BLOCK_DEFAULT 32
#define COH_BLOCK_MAX 64
#define COH_GRID_DEFAULT (1 << 16)
#define COH_LDS_BYTES (64 << 10)
#define COH_SLOT 320                     // a prefix's slot: 16 + COH_PREFIX_MAX rounded up to quads
#define COH_SLOT_ROWS 64                 // prefixes assembled at a time
#define COH_SPAN 4096                    // bytes of the text a workgroup of k_cparse_len owns
#define COH_PARSE_ROWS 64                // the most rows of a tile of k_cparse_fill

struct CohStatus { unsigned long long first; };

struct KCohW {
    const int32_t *contig, *start, *end; const uint8_t *context; const int8_t *strand; const int32_t *nsamples;
    const int32_t *m, *u; int32_t S; int64_t n; int32_t fmt;
    const uint32_t *name_off; const uint8_t *names; int32_t n_contigs;
    int64_t *len; uint16_t *part; int32_t tile, sblock, nb;
    int64_t r0, r1, base; uint8_t *out;
    CohStatus *st;
};

__global__ __launch_bounds__(COH_WG) void k_ctext_len(const KCohW K) {
    const int64_t i = (int64_t)blockIdx.x * COH_WG + threadIdx.x, n = K.n;
    if(i >= n) return;
    const int32_t c = K.contig[i], a = K.start[i], b = K.end[i], ns = K.nsamples[i];
    const uint32_t ctx = K.context[i];
    const uint32_t what = coh_site_check(c, a, b, ctx, K.n_contigs);
    if(what) { atomicMin(&K.st->first, (unsigned long long)coh_write_key(i, what, 0)); K.len[i] = 0; return; }
    uint32_t acc = coh_prefix_len(K.fmt, K.name_off[c + 1] - K.name_off[c], a, b, ctx, ns);
    int32_t bad = -1;
    for(int32_t blk = 0; blk < K.nb; blk++) {
        K.part[(int64_t)blk * n + i] = (uint16_t)acc;
        const int32_t s1 = (blk + 1) * K.sblock < K.S ? (blk + 1) * K.sblock : K.S;
        for(int32_t s = blk * K.sblock; s < s1; s++) {
            const int32_t m = K.m[(int64_t)s * n + i], u = K.u[(int64_t)s * n + i];
            if((m < 0 || u < 0) && bad < 0) bad = s;
            acc += coh_cell_len(K.fmt, (uint32_t)m, (uint32_t)u);
        }
    }
    if(bad >= 0) atomicMin(&K.st->first, (unsigned long long)coh_write_key(i, COH_W_NEGATIVE, bad));
    K.len[i] = (int64_t)acc + 1;
}

// a[0 .. n) into its exclusive prefix sums, a[n] their total: one workgroup of 1024
__global__ __launch_bounds__(1024) void k_scan64(int64_t *a, int64_t n) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, i0 = t * per < n ? t * per : n, i1 = i0 + per < n ? i0 + per : n;
    int64_t sum = 0;
    for(int64_t i = i0; i < i1; i++) sum += a[i];
    part[t] = sum;
    __syncthreads();
    for(int d = 1; d < 1024; d <<= 1) {
        const int64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - sum;
    for(int64_t i = i0; i < i1; i++) { const int64_t x = a[i]; a[i] = run; run += x; }
    if(t == 1023) a[n] = part[1023];
}

__device__ __forceinline__ int32_t wave_incl_scan(int32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for(int d = 1; d < 64; d <<= 1) { const int32_t o = __shfl_up(v, d, 64); if(lane >= d) v += o; }
    return v;
}

// image bytes [p.sh, p.end) to dst, by the lanes l of nl: whole quads, then the ragged ends (img and dst - p.sh are 16-byte aligned)
__device__ __forceinline__ void coh_store_image(const uint8_t *img, const txt_image_plan &p, uint8_t *dst, uint32_t l, uint32_t nl) {
    uint8_t *const base = dst - p.sh;
    for(uint32_t q = p.quad0 + l; q < p.quad1; q += nl) *(uint4 *)(base + 16u * q) = *(const uint4 *)(img + 16u * q);
    for(uint32_t i = p.sh + l; i < p.head_end; i += nl) base[i] = img[i];
    for(uint32_t i = p.tail0 + l; i < p.end; i += nl) base[i] = img[i];
}

static __host__ __device__ inline uint32_t coh_image_bytes(int32_t sblock) { return (16u + (uint32_t)sblock * COH_CELL_MAX + 1u + 15u) & ~15u; }

__global__ __launch_bounds__(COH_WG) void k_ctext_fill(const KCohW K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char coh_lds[];
    const int32_t T = K.tile, Tp = T + 1, B = K.sblock;
    const uint32_t imgw = coh_image_bytes(B);
    uint8_t *const images = coh_lds;                                         // COH_WAVES images, or COH_SLOT_ROWS prefix slots
    int32_t *const Ms = (int32_t *)(coh_lds + COH_WAVES * imgw), *const Us = Ms + (size_t)B * Tp;
    const int64_t n = K.n, rows = K.r1 - K.r0, ntiles = (rows + T - 1) / T, items = ntiles * (K.nb + 1);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for(int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t tile = item / (K.nb + 1);
        const int32_t blk = (int32_t)(item - tile * (K.nb + 1)) - 1;         // -1: the prefixes
        const int64_t t0 = K.r0 + tile * T, t1 = t0 + T < K.r1 ? t0 + T : K.r1;
        if(blk < 0) {
            for(int64_t g0 = t0; g0 < t1; g0 += COH_SLOT_ROWS) {
                __syncthreads();
                txt_image_plan p;
                if(tid < COH_SLOT_ROWS && g0 + tid < t1) {
                    const int64_t i = g0 + tid;
                    const int32_t c = K.contig[i];
                    const uint32_t o = K.name_off[c], nl = K.name_off[c + 1] - o;
                    const uint64_t dst = (uint64_t)(K.out + (K.len[i] - K.base));
                    uint8_t *const slot = images + (size_t)tid * COH_SLOT;
                    coh_put_prefix((char *)slot + (dst & 15u), K.fmt, K.names + o, nl, K.start[i], K.end[i], K.context[i], K.strand[i], K.nsamples[i]);
                }
                __syncthreads();
                for(uint32_t r = tid >> 4; r < COH_SLOT_ROWS; r += COH_WG / 16) {
                    const int64_t i = g0 + r;
                    if(i >= t1) break;
                    uint8_t *const dst = K.out + (K.len[i] - K.base);
                    p = txt_plan_image((uint64_t)dst, K.part[i]);             // (block 0 starts where the prefix ends)
                    coh_store_image(images + (size_t)r * COH_SLOT, p, dst, tid & 15u, 16u);
                }
            }
            __syncthreads();
            continue;
        }
        const int32_t s0 = blk * B, nbk = K.S - s0 < B ? K.S - s0 : B;
        const bool last = blk == K.nb - 1;
        __syncthreads();
        for(int32_t idx = tid; idx < nbk * T; idx += COH_WG) {
            const int32_t s = idx / T, r = idx - s * T;
            const int64_t i = t0 + r;
            if(i < t1) { Ms[s * Tp + r] = K.m[(int64_t)(s0 + s) * n + i]; Us[s * Tp + r] = K.u[(int64_t)(s0 + s) * n + i]; }
        }
        __syncthreads();
        uint8_t *const img = images + (size_t)wave * imgw;
        for(int32_t r = wave; r < T; r += COH_WAVES) {
            const int64_t i = t0 + r;
            const bool active = i < t1;
            uint32_t m = 0, u = 0; int32_t w = 0;
            if(active && (int32_t)lane < nbk) { m = (uint32_t)Ms[lane * Tp + r]; u = (uint32_t)Us[lane * Tp + r]; w = (int32_t)coh_cell_len(K.fmt, m, u); }
            const int32_t incl = wave_incl_scan(w);
            const uint32_t total = active ? (uint32_t)__shfl(incl, 63, 64) + (last ? 1u : 0u) : 0u;
            uint8_t *const dst = active ? K.out + (K.len[i] - K.base) + K.part[(int64_t)blk * n + i] : K.out;
            const txt_image_plan p = txt_plan_image((uint64_t)dst, total);
            if(active && (int32_t)lane < nbk) coh_put_cell((char *)img + p.sh + (uint32_t)(incl - w), K.fmt, m, u);
            if(active && last && lane == 0) img[p.sh + total - 1] = '\n';
            __syncthreads();
            if(active) coh_store_image(img, p, dst, lane, 64u);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------
// read
// ------------------------------------------------------------------------------------------------
struct KCohR {
    const uint8_t *text; int64_t bytes, begin; int32_t S;
    const uint32_t *name_off; const uint8_t *names; const uint32_t *sorted; int32_t n_contigs;
    int64_t *cnt, *line; int64_t rows;
    int32_t *contig, *start, *end; uint8_t *context; int8_t *strand; int32_t *nsamples;
    int32_t *m, *u; int64_t stride, row_at; int32_t R, Rp;
    int32_t has_prev, prev_contig, prev_start;
    CohStatus *st;
};

// the 16 bytes of the text at p (a multiple of 16; the text is 16-byte aligned), zeros behind its end
__device__ __forceinline__ uint4 coh_load16(const uint8_t *text, int64_t bytes, int64_t p) {
    if(p + COH_LANE <= bytes) return *(const uint4 *)(text + p);
    uint32_t w[4] = { 0, 0, 0, 0 };
    for(int k = 0; k < COH_LANE && p + k < bytes; k++) w[k >> 2] |= (uint32_t)text[p + k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
// the line starts among the 16 bytes at p: bit k for byte k
__device__ __forceinline__ uint32_t coh_starts_at(const KCohR &K, int64_t p) {
    if(p >= K.bytes || p + COH_LANE <= K.begin) return 0u;
    const uint4 w = coh_load16(K.text, K.bytes, p);
    return coh_line_starts(w.x, w.y, w.z, w.w, p > K.begin && K.text[p - 1] == '\n', p, K.begin, K.bytes);
}

__global__ __launch_bounds__(COH_WG) void k_cparse_len(const KCohR K) {
    __shared__ int32_t total;
    if(threadIdx.x == 0) total = 0;
    __syncthreads();
    const int64_t p = ((int64_t)blockIdx.x * COH_WG + threadIdx.x) * COH_LANE;
    const int32_t c = __popc(coh_starts_at(K, p));
    if(c) atomicAdd(&total, c);
    __syncthreads();
    if(threadIdx.x == 0) K.cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(COH_WG) void k_cparse_starts(const KCohR K) {
    __shared__ int32_t sums[COH_WG];
    const int t = threadIdx.x;
    const int64_t p = ((int64_t)blockIdx.x * COH_WG + t) * COH_LANE;
    uint32_t s = coh_starts_at(K, p);
    const int32_t c = __popc(s);
    sums[t] = c;
    __syncthreads();
    for(int d = 1; d < COH_WG; d <<= 1) {
        const int32_t v = t >= d ? sums[t - d] : 0;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    int64_t at = K.cnt[blockIdx.x] + sums[t] - c;
    while(s) {
        const int k = __ffs(s) - 1; s &= s - 1;
        if(at < K.rows) K.line[at] = p + k;
        at++;
    }
    if(blockIdx.x == 0 && t == 0) K.line[K.rows] = K.bytes;
}

__global__ __launch_bounds__(COH_WG) void k_cparse_fill(const KCohR K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char coh_lds[];
    const int32_t R = K.R, Rp = K.Rp, S = K.S;
    int32_t *const stage = (int32_t *)coh_lds;                               // [2][S][Rp]
    int32_t *const rec = stage + (size_t)2 * S * Rp;                         // [R][COH_SITE_FIELDS]
    uint32_t *const rank_of = (uint32_t *)(rec + (size_t)R * COH_SITE_FIELDS);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, want = COH_SITE_FIELDS + 2u * (uint32_t)S;
    const uint8_t *const text = K.text;
    prs_tab T; T.name_off = K.name_off; T.names = K.names; T.sorted = K.sorted; T.n_contigs = K.n_contigs; T.ref = nullptr; T.ref_len = nullptr;
    const int64_t ntiles = (K.rows + R - 1) / R;
    for(int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * R;
        const int32_t nr = K.rows - row0 < R ? (int32_t)(K.rows - row0) : R;
        __syncthreads();                                                      // the tile before has left the stage
        for(int32_t r = wave; r < nr; r += COH_WAVES) {
            const int64_t ls = K.line[row0 + r], nx = K.line[row0 + r + 1], le = coh_line_end(text, ls, nx);
            uint32_t rank = coh_line_rank(text, ls, le, nx - ls);
            if(rank == COH_RANK_NONE) {
                int32_t v = 0;
                if(lane == 0) { rank = coh_field(text, ls, le, 0, T, v); if(rank == COH_RANK_NONE) rec[r * COH_SITE_FIELDS] = v; }
                uint32_t tabs = 0;
                for(int64_t q = ls & ~(int64_t)(COH_LANE - 1); q < le; q += 64 * COH_LANE) {
                    const int64_t p = q + (int64_t)lane * COH_LANE;
                    uint32_t mask = 0;
                    if(p < le) { const uint4 w = coh_load16(text, K.bytes, p); mask = coh_tabs(w.x, w.y, w.z, w.w) & coh_inside(p, ls, le); }
                    const int32_t c = __popc(mask), incl = wave_incl_scan(c);
                    uint32_t f = tabs + (uint32_t)(incl - c);
                    while(mask) {
                        const int k = __ffs(mask) - 1; mask &= mask - 1; f++;
                        if(f < want) {
                            const uint32_t e = coh_field(text, p + k + 1, le, f, T, v);
                            if(e != COH_RANK_NONE) rank = e < rank ? e : rank;
                            else if(f < COH_SITE_FIELDS) rec[r * COH_SITE_FIELDS + f] = v;
                            else stage[(size_t)(((f - COH_SITE_FIELDS) & 1u) * S + ((f - COH_SITE_FIELDS) >> 1)) * Rp + r] = v;
                        }
                    }
                    tabs += (uint32_t)__shfl(incl, 63, 64);
                }
                const uint32_t e = coh_count_rank(tabs, S);
                rank = e < rank ? e : rank;
#pragma unroll
                for(int d = 32; d; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int32_t)rank, d, 64); rank = o < rank ? o : rank; }
            }
            if(lane == 0) rank_of[r] = rank;
        }
        __syncthreads();
        if((int32_t)tid < nr) {
            const int32_t *const e = rec + tid * COH_SITE_FIELDS;
            uint32_t rank = rank_of[tid];
            if(rank == COH_RANK_NONE) rank = coh_row_rank(e[1], e[2], e[5], S);
            const int64_t row = row0 + tid;
            if(rank != COH_RANK_NONE) atomicMin(&K.st->first, (unsigned long long)((uint64_t)row << 8 | coh_rank_code(rank)));
            else {
                K.contig[row] = e[0]; K.start[row] = e[1]; K.end[row] = e[2]; K.context[row] = (uint8_t)e[3]; K.strand[row] = (int8_t)e[4]; K.nsamples[row] = e[5];
            }
        }
        for(int32_t idx = tid; idx < 2 * S * nr; idx += COH_WG) {
            const int32_t s2 = idx / nr, r = idx - s2 * nr;
            if(rank_of[r] != COH_RANK_NONE) continue;
            int32_t *const out = s2 < S ? K.m : K.u;
            out[(int64_t)(s2 < S ? s2 : s2 - S) * K.stride + K.row_at + row0 + r] = stage[(size_t)s2 * Rp + r];
        }
    }
}

__global__ __launch_bounds__(COH_WG) void k_cparse_order(const KCohR K) {
    const int64_t i = (int64_t)blockIdx.x * COH_WG + threadIdx.x;
    if(i >= K.rows || (i == 0 && !K.has_prev)) return;
    const int32_t c0 = i ? K.contig[i - 1] : K.prev_contig, x0 = i ? K.start[i - 1] : K.prev_start;
    if(!coh_ascends(c0, x0, K.contig[i], K.start[i])) atomicMin(&K.st->first, (unsigned long long)((uint64_t)i << 8 | COH_E_ORDER));
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
#define SIDE_ERR_ARG MD_COHORT_ERR_ARG
#define SIDE_ERR_HIP MD_COHORT_ERR_HIP
#define SIDE_ERR_NOMEM MD_COHORT_ERR_NOMEM
#include "mdk_side.hpp"
extern "C" const char *md_cohort_last_error(void) { return g_err; }

struct md_cohort : SideHandle<CohStatus> {
    int64_t *pin64 = nullptr;
    int32_t tile = COH_TILE_DEFAULT, sblock = COH_BLOCK_DEFAULT, grid = COH_GRID_DEFAULT;
    uint32_t *d_name_off = nullptr, *d_sorted = nullptr; uint8_t *d_names = nullptr; int32_t n_contigs = 0;
    SideBuf<int64_t> d_len; SideBuf<uint16_t> d_part;          // (these four: as large as the largest table asked for, and no larger)
    KCohW W; bool measured = false; int64_t total = 0;
    SideBuf<int64_t> d_cnt, d_line;
    KCohR P; bool counted = false; int64_t err_offset = -1;
    SideBuf<uint8_t> d_rpass; SideBuf<uint32_t> d_rlo, d_rhi, d_rsites; SideBuf<int64_t> d_rm, d_ru;      // md_cohort_regions' (mdk_cregion.hip), kept likewise
};

extern "C" int md_cohort_open(int device, md_cohort **out) {
    return side_open(device, out, "md_cohort_open", md_cohort_close, [](md_cohort *h) { return hipHostMalloc((void **)&h->pin64, 2 * sizeof(int64_t), hipHostMallocDefault); });
}

extern "C" void md_cohort_close(md_cohort *h) {
    if(!h) return;
    h->close();
    (void)hipFree(h->d_name_off); (void)hipFree(h->d_sorted); (void)hipFree(h->d_names);
    h->d_len.release(); h->d_part.release(); h->d_cnt.release(); h->d_line.release();
    h->d_rpass.release(); h->d_rlo.release(); h->d_rhi.release(); h->d_rsites.release(); h->d_rm.release(); h->d_ru.release();
    if(h->pin64) (void)hipHostFree(h->pin64);
    delete h;
}

static size_t coh_fill_lds(int32_t tile, int32_t sblock) {
    const size_t a = (size_t)COH_WAVES * coh_image_bytes(sblock) + (size_t)8 * sblock * (tile + 1), b = (size_t)COH_SLOT_ROWS * COH_SLOT;
    return a > b ? a : b;
}

extern "C" int md_cohort_limits(md_cohort *h, int32_t tile_sites, int32_t sample_block, int32_t max_workgroups) {
    const char *const what = "md_cohort_limits";
    if(!h) return fail(MD_COHORT_ERR_ARG, what, hipSuccess);
    const int32_t tile = tile_sites ? tile_sites : COH_TILE_DEFAULT, sblock = sample_block ? sample_block : COH_BLOCK_DEFAULT, grid = max_workgroups ? max_workgroups : COH_GRID_DEFAULT;
    if(tile < 64 || tile > 256 || tile % 64 || sblock < 1 || sblock > COH_BLOCK_MAX || grid < 1 || coh_fill_lds(tile, sblock) > COH_LDS_BYTES) {
        snprintf(g_err, sizeof g_err, "%s: tile_sites a multiple of 64 up to 256, sample_block 1 to %d, their counts and images at most %d bytes of LDS, max_workgroups above 0",
                 what, COH_BLOCK_MAX, COH_LDS_BYTES);
        return MD_COHORT_ERR_ARG;
    }
    h->tile = tile; h->sblock = sblock; h->grid = grid; h->measured = false; h->counted = false;
    return 0;
}

extern "C" int md_cohort_names(md_cohort *h, const uint8_t *names, const uint32_t *name_off, int32_t n_contigs) {
    const char *const what = "md_cohort_names";
    if(!h || n_contigs < 0 || (n_contigs && (!names || !name_off))) return fail(MD_COHORT_ERR_ARG, what, hipSuccess);
    for(int32_t c = 0; c < n_contigs; c++)
        if(name_off[c + 1] <= name_off[c] || name_off[c + 1] - name_off[c] > MD_TEXT_NAME_MAX) {
            snprintf(g_err, sizeof g_err, "%s: contig %d's name is empty or longer than %d bytes", what, c, MD_TEXT_NAME_MAX);
            return MD_COHORT_ERR_ARG;
        }
    SIDECHK(hipSetDevice(h->device));
    (void)hipFree(h->d_name_off); (void)hipFree(h->d_sorted); (void)hipFree(h->d_names);
    h->d_name_off = h->d_sorted = nullptr; h->d_names = nullptr; h->n_contigs = 0; h->measured = false; h->counted = false;
    const uint32_t zero = 0, total = n_contigs ? name_off[n_contigs] : 0;
    std::vector<uint32_t> sorted((size_t)n_contigs);
    for(int32_t c = 0; c < n_contigs; c++) sorted[c] = (uint32_t)c;
    std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) {
        return prs_name_cmp(names + name_off[a], name_off[a + 1] - name_off[a], names + name_off[b], name_off[b + 1] - name_off[b]) < 0; });
    SIDECHK(hipMalloc((void **)&h->d_name_off, (size_t)(n_contigs + 1) * sizeof(uint32_t)));
    SIDECHK(hipMalloc((void **)&h->d_sorted, (size_t)(n_contigs + 1) * sizeof(uint32_t)));
    SIDECHK(hipMalloc((void **)&h->d_names, (size_t)total + 16));
    SIDECHK(hipMemcpy(h->d_name_off, n_contigs ? name_off : &zero, (size_t)(n_contigs + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    if(n_contigs) SIDECHK(hipMemcpy(h->d_sorted, sorted.data(), (size_t)n_contigs * sizeof(uint32_t), hipMemcpyHostToDevice));
    if(total) SIDECHK(hipMemcpy(h->d_names, names, total, hipMemcpyHostToDevice));
    h->n_contigs = n_contigs;
    return 0;
}

extern "C" int md_cohort_measure(md_cohort *h, int fmt, const md_cohort_sites *sites, const int32_t *nmeth, const int32_t *nunmeth, int32_t n_samples, int64_t n, int64_t *total_bytes) {
    const char *const what = "md_cohort_measure";
    if(!h || !total_bytes || fmt < 0 || fmt >= COH_N_FORMATS || n_samples < 1 || n_samples > COH_MAX_SAMPLES || n < 0 || n > ((int64_t)1 << 30)) return fail(MD_COHORT_ERR_ARG, what, hipSuccess);
    if(n && (!sites || !sites->contig || !sites->start || !sites->end || !sites->context || !sites->strand || !sites->nsamples || !nmeth || !nunmeth)) return fail(MD_COHORT_ERR_ARG, what, hipSuccess);
    if(!h->d_name_off) return fail(MD_COHORT_ERR_ARG, "md_cohort_measure: no contig names (md_cohort_names)", hipSuccess);
    h->measured = false; *total_bytes = 0;
    SIDECHK(hipSetDevice(h->device));
    KCohW &K = h->W;
    K.S = n_samples; K.n = n; K.fmt = fmt; K.tile = h->tile; K.sblock = n_samples < h->sblock ? n_samples : h->sblock; K.nb = (n_samples + K.sblock - 1) / K.sblock;
    if(int rc = h->d_len.need((size_t)n + 1, "md_cohort_measure: the lines' lengths")) return rc;
    if(int rc = h->d_part.need((size_t)(n ? n : 1) * K.nb, "md_cohort_measure: the lines' lengths")) return rc;
    if(n) {
        K.contig = (const int32_t *)sites->contig; K.start = (const int32_t *)sites->start; K.end = (const int32_t *)sites->end;
        K.context = (const uint8_t *)sites->context; K.strand = (const int8_t *)sites->strand; K.nsamples = (const int32_t *)sites->nsamples;
    }
    K.m = nmeth; K.u = nunmeth; K.name_off = h->d_name_off; K.names = h->d_names; K.n_contigs = h->n_contigs;
    K.len = h->d_len; K.part = h->d_part; K.st = h->d_st; K.r0 = K.r1 = K.base = 0; K.out = nullptr;
    SIDE_STATUS_UP(h, h->pin, CohStatus);
    if(n) {
        hipLaunchKernelGGL(k_ctext_len, dim3((uint32_t)((n + COH_WG - 1) / COH_WG)), dim3(COH_WG), 0, h->st, K);
        SIDECHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_scan64, dim3(1), dim3(1024), 0, h->st, h->d_len, n);
    SIDECHK(hipGetLastError());
    SIDECHK(hipMemcpyAsync(h->pin, h->d_st, sizeof(CohStatus), hipMemcpyDeviceToHost, h->st));
    SIDECHK(hipMemcpyAsync(h->pin64, h->d_len + n, sizeof(int64_t), hipMemcpyDeviceToHost, h->st));
    SIDECHK(hipStreamSynchronize(h->st));
    const unsigned long long first = h->pin->first;
    if(first != ~0ull) {
        const uint32_t w = (uint32_t)(first >> 11) & 31u;
        if(w == COH_W_NEGATIVE) snprintf(g_err, sizeof g_err, "%s: %s (site %lld, sample %u)", what, coh_write_error_text(w), (long long)(first >> 16), (unsigned)(first & 2047u));
        else snprintf(g_err, sizeof g_err, "%s: %s (site %lld)", what, coh_write_error_text(w), (long long)(first >> 16));
        return MD_COHORT_ERR_ARG;
    }
    h->total = *total_bytes = h->pin64[0]; h->measured = true;
    return 0;
}

static int coh_offset(md_cohort *h, int64_t row, int64_t *v) {
    SIDECHK(hipMemcpyAsync(h->pin64, h->d_len + row, sizeof(int64_t), hipMemcpyDeviceToHost, h->st));
    SIDECHK(hipStreamSynchronize(h->st));
    *v = h->pin64[0];
    return 0;
}

extern "C" int md_cohort_cut(md_cohort *h, int64_t row0, int64_t max_bytes, int64_t *row1, int64_t *bytes) {
    if(!h || !h->measured || !row1 || !bytes || row0 < 0 || row0 >= h->W.n || max_bytes < 1) return fail(MD_COHORT_ERR_ARG, "md_cohort_cut", hipSuccess);
    SIDECHK(hipSetDevice(h->device));
    int64_t base, v;
    if(int rc = coh_offset(h, row0, &base)) return rc;
    int64_t lo = row0 + 1, hi = h->W.n;                                     // the largest r in [row0 + 1, n] with offset[r] - base <= max_bytes, or row0 + 1
    while(lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if(int rc = coh_offset(h, mid, &v)) return rc;
        if(v - base <= max_bytes) lo = mid; else hi = mid - 1;
    }
    if(int rc = coh_offset(h, lo, &v)) return rc;
    *row1 = lo; *bytes = v - base;
    return 0;
}

extern "C" int md_cohort_fill(md_cohort *h, int64_t row0, int64_t row1, void *out, int64_t bytes) {
    const char *const what = "md_cohort_fill";
    if(!h || !h->measured || row0 < 0 || row1 <= row0 || row1 > h->W.n || !out) return fail(MD_COHORT_ERR_ARG, what, hipSuccess);
    SIDECHK(hipSetDevice(h->device));
    int64_t base, end;
    if(int rc = coh_offset(h, row0, &base)) return rc;
    if(int rc = coh_offset(h, row1, &end)) return rc;
    if(end - base != bytes) return fail(MD_COHORT_ERR_ARG, "md_cohort_fill: the buffer is not the size the rows were measured at", hipSuccess);
    KCohW K = h->W;
    K.r0 = row0; K.r1 = row1; K.base = base; K.out = (uint8_t *)out;
    const int64_t items = ((row1 - row0 + K.tile - 1) / K.tile) * (K.nb + 1);
    hipLaunchKernelGGL(k_ctext_fill, dim3((uint32_t)(items < h->grid ? items : h->grid)), dim3(COH_WG), coh_fill_lds(K.tile, K.sblock), h->st, K);
    SIDECHK(hipGetLastError());
    SIDECHK(hipStreamSynchronize(h->st));
    return 0;
}

extern "C" int md_cohort_parse_measure(md_cohort *h, const void *text, int64_t bytes, int64_t begin, int32_t n_samples, int64_t *rows) {
    const char *const what = "md_cohort_parse_measure";
    if(!h || !rows || bytes < 0 || bytes > (int64_t)INT32_MAX || begin < 0 || begin > bytes || n_samples < 1 || n_samples > COH_MAX_SAMPLES || (bytes && !text) || ((uintptr_t)text & 15u))
        return fail(MD_COHORT_ERR_ARG, what, hipSuccess);
    if(!h->d_name_off) return fail(MD_COHORT_ERR_ARG, "md_cohort_parse_measure: no contig names (md_cohort_names)", hipSuccess);
    h->counted = false; h->err_offset = -1; *rows = 0;
    SIDECHK(hipSetDevice(h->device));
    KCohR &K = h->P;
    memset(&K, 0, sizeof K);
    const int64_t spans = (bytes + COH_SPAN - 1) / COH_SPAN;
    if(int rc = h->d_cnt.need((size_t)spans + 1, "md_cohort_parse_measure: the spans' counts")) return rc;
    K.text = (const uint8_t *)text; K.bytes = bytes; K.begin = begin; K.S = n_samples;
    K.name_off = h->d_name_off; K.names = h->d_names; K.sorted = h->d_sorted; K.n_contigs = h->n_contigs; K.cnt = h->d_cnt; K.st = h->d_st;
    if(spans) {
        hipLaunchKernelGGL(k_cparse_len, dim3((uint32_t)spans), dim3(COH_WG), 0, h->st, K);
        SIDECHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_scan64, dim3(1), dim3(1024), 0, h->st, h->d_cnt, spans);
    SIDECHK(hipGetLastError());
    SIDECHK(hipMemcpyAsync(h->pin64, h->d_cnt + spans, sizeof(int64_t), hipMemcpyDeviceToHost, h->st));
    SIDECHK(hipStreamSynchronize(h->st));
    K.rows = *rows = h->pin64[0];
    if(int rc = h->d_line.need((size_t)K.rows + 1, "md_cohort_parse_measure: the line starts")) return rc;
    K.line = h->d_line;
    if(K.rows) {
        hipLaunchKernelGGL(k_cparse_starts, dim3((uint32_t)spans), dim3(COH_WG), 0, h->st, K);
        SIDECHK(hipGetLastError());
        SIDECHK(hipStreamSynchronize(h->st));
    }
    h->counted = true;
    return 0;
}

extern "C" int md_cohort_parse_fill(md_cohort *h, const md_cohort_sites *sites, int32_t *nmeth, int32_t *nunmeth, int64_t stride, int64_t row_at, int64_t rows,
                                    int has_prev, int32_t prev_contig, int32_t prev_start) {
    const char *const what = "md_cohort_parse_fill";
    if(!h || !h->counted || rows != h->P.rows || row_at < 0 || stride < row_at + rows) return fail(MD_COHORT_ERR_ARG, what, hipSuccess);
    h->counted = false;
    if(!rows) return 0;
    if(!sites || !sites->contig || !sites->start || !sites->end || !sites->context || !sites->strand || !sites->nsamples || !nmeth || !nunmeth) return fail(MD_COHORT_ERR_ARG, what, hipSuccess);
    SIDECHK(hipSetDevice(h->device));
    KCohR K = h->P;
    // the sites' columns hold THIS text's rows from their entry 0; the matrices hold them from row_at
    K.contig = (int32_t *)sites->contig; K.start = (int32_t *)sites->start; K.end = (int32_t *)sites->end;
    K.context = (uint8_t *)sites->context; K.strand = (int8_t *)sites->strand; K.nsamples = (int32_t *)sites->nsamples;
    K.m = nmeth; K.u = nunmeth; K.stride = stride; K.row_at = row_at;
    K.has_prev = has_prev; K.prev_contig = prev_contig; K.prev_start = prev_start;
    // a tile's rows: what 64 KiB take with the row stride odd, within the handle's tile and COH_PARSE_ROWS
    int32_t R = h->tile < COH_PARSE_ROWS ? h->tile : COH_PARSE_ROWS;
    auto lds = [&](int32_t r) { return (size_t)8 * K.S * (r | 1) + (size_t)r * (COH_SITE_FIELDS + 1) * 4; };
    while(R > 1 && lds(R) > COH_LDS_BYTES) R--;
    K.R = R; K.Rp = R | 1;
    SIDE_STATUS_UP(h, h->pin, CohStatus);
    const int64_t ntiles = (rows + R - 1) / R;
    hipLaunchKernelGGL(k_cparse_fill, dim3((uint32_t)(ntiles < h->grid ? ntiles : h->grid)), dim3(COH_WG), lds(R), h->st, K);
    SIDECHK(hipGetLastError());
    hipLaunchKernelGGL(k_cparse_order, dim3((uint32_t)((rows + COH_WG - 1) / COH_WG)), dim3(COH_WG), 0, h->st, K);
    SIDECHK(hipGetLastError());
    SIDE_STATUS_DOWN(h, h->pin, CohStatus);
    const unsigned long long first = h->pin->first;
    if(first == ~0ull) return 0;
    SIDECHK(hipMemcpyAsync(h->pin64, h->d_line + (int64_t)(first >> 8), sizeof(int64_t), hipMemcpyDeviceToHost, h->st));
    SIDECHK(hipStreamSynchronize(h->st));
    h->err_offset = h->pin64[0];
    snprintf(g_err, sizeof g_err, "%s", coh_error_text((uint32_t)(first & 0xffu)));
    return MD_COHORT_ERR_ARG;
}

extern "C" int64_t md_cohort_parse_error_offset(md_cohort *h) { return h ? h->err_offset : -1; }

// ------------------------------------------------------------------------------------------------
// every sample's sums over intervals
// ------------------------------------------------------------------------------------------------
#include "mdk_cregion.hip"
