// mdk_smooth.hip -- libmdk_smooth.so (include/mdk_smooth.h): kernel-weighted methylation levels of every site of a table, per sample, on
// the device.  The rule is mdk_smooth_core.h's.  A library of its own, as mdk_qdiff.hip's is -- one code object, its own stream, its own
// pinned status block, its own error text -- that links nothing of the other libraries.
//
// One synchronous call and two kernels:
//   k_smooth_window  a lane per site, once for all samples: the contig's run by two bounds on `contig`, d_k by bisection over the runs of
//                    k rows that hold the site (log2 k steps; a scan would take up to k), then half, lo, hi by two more bounds; the row
//                    is checked against its predecessor.  Stores half and nsites (outputs) and lo (the handle's scratch), coalesced.
//   k_smooth_sum     a workgroup takes work items (tile, batch) in a grid-stride loop: a tile of `tile` consecutive sites, a lane each,
//                    and a batch of up to SMO_BATCH samples.  lo and hi are monotone, so the tile's source rows are the one range
//                    [lo(first), hi(last)); it is streamed through LDS in chunks of `chunk` rows, ascending.  A chunk in LDS:
//                        double  M[batch][chunk]   (double)m           sample b's row r at M[b * chunk + r]
//                        double  D[batch][chunk]   (double)(m + u)
//                        int32   x[chunk]          the starts
//                    converted once when staged, not once per pair.  Each lane walks the chunk's rows inside its own [lo_i, hi_i),
//                    ascending -- so the summation order is the rule's whatever the blocking --, computes w once per pair and applies
//                    it to every sample of the batch, 2 x SMO_BATCH accumulators in registers.  Neighbouring lanes' lo differ by 0 or
//                    1 mostly, so at step q the wavefront reads rows lo_i + q: consecutive 8-byte LDS addresses per sample.  One code
//                    path for any window width: nothing assumes a window fits LDS.  An entry is checked where it is staged, by the
//                    workgroup whose tile owns its site and by no other.
// A refusal is (site << 8 | bit number) into the status by atomicMin, the kernels' one atomic.  Whatever the table holds nothing outside
// it is read and nothing outside the outputs written: the searches stay inside [0, n), every lane's range is cut to the chunk that is
// staged, and a tile's source range is cut to tile + 2 smo_window_cap rows, which no valid table reaches.
// Plain C++, vector loads and stores, no MFMA, no flag that relaxes the arithmetic.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include "mdk_smooth.h"
#include "mdk_smooth_core.h"

#define SMO_WG 256                       // the window kernel's workgroup, and the most sites of a tile
#define SMO_BATCH 8                      // the most samples of a batch: 16 accumulators a lane
#define SMO_TILE_DEFAULT 256
#define SMO_CHUNK_DEFAULT 384
#define SMO_BATCH_DEFAULT 8
#define SMO_GRID_DEFAULT (1 << 20)
#define SMO_LDS_BYTES (64 << 10)         // what a chunk and a batch may take together: no opt-in for more is asked of the runtime

struct SmoothStatus { unsigned long long first; };             // the smallest (site << 8 | refusal's bit number); all ones: none

struct KSmooth {
    const int32_t *contig, *start; const void *m, *u;
    int32_t S; int64_t n; int32_t half_bases, min_sites, kernel;
    double *level, *depth; int32_t *nsites, *half, *lo;
    int32_t tile, chunk, batch; int64_t items, cap;
    SmoothStatus *st;
};

__global__ __launch_bounds__(SMO_WG) void k_smooth_window(const KSmooth K) {
    const int64_t i = (int64_t)blockIdx.x * SMO_WG + threadIdx.x;
    if(i >= K.n) return;
    const int32_t *const __restrict__ contig = K.contig, *const __restrict__ x = K.start;
    const uint32_t err = smo_row_check(i > 0, i > 0 ? contig[i - 1] : 0, i > 0 ? x[i - 1] : 0, contig[i], x[i]);
    if(err) atomicMin(&K.st->first, (unsigned long long)smo_refusal_key(i, err));
    int64_t c0, c1;
    smo_contig_run(contig, K.n, i, &c0, &c1);
    const smo_window w = smo_window_of(x, c0, c1, i, K.half_bases, K.min_sites);
    K.half[i] = (int32_t)w.half; K.nsites[i] = (int32_t)(w.hi - w.lo); K.lo[i] = (int32_t)w.lo;
}

template <typename T>
__global__ __launch_bounds__(SMO_WG) void k_smooth_sum(const KSmooth K) {
    MDK_SMO_NO_CONTRACT
    extern __shared__ __attribute__((aligned(16))) unsigned char smo_lds[];
    const int32_t C = K.chunk;
    double *const Ms = (double *)smo_lds, *const Ds = Ms + (size_t)K.batch * C;
    int32_t *const xs = (int32_t *)(Ds + (size_t)K.batch * C);
    const T *const __restrict__ Mg = (const T *)K.m, *const __restrict__ Ug = (const T *)K.u;
    const int32_t *const __restrict__ x = K.start;
    const int64_t n = K.n;
    const int32_t nbatch = (K.S + K.batch - 1) / K.batch;
    for(int64_t item = blockIdx.x; item < K.items; item += gridDim.x) {
        const int64_t tile = item / nbatch;
        const int32_t s0 = (int32_t)(item - tile * nbatch) * K.batch, nb = K.S - s0 < K.batch ? K.S - s0 : K.batch;
        const int64_t t0 = tile * K.tile, t1 = t0 + K.tile < n ? t0 + K.tile : n;
        const int64_t i = t0 + threadIdx.x;
        const bool active = i < t1;
        // the lane's window, cut to the table
        int64_t lo_i = 0, hi_i = 0, half_i = 0, x_i = 0;
        if(active) {
            lo_i = K.lo[i]; hi_i = lo_i + K.nsites[i]; half_i = K.half[i]; x_i = x[i];
            lo_i = lo_i < 0 ? 0 : lo_i > n ? n : lo_i; hi_i = hi_i < lo_i ? lo_i : hi_i > n ? n : hi_i;
        }
        const double inv = smo_inverse(half_i);
        // the tile's source rows (the same addresses in every lane)
        int64_t r0 = K.lo[t0], r1 = (int64_t)K.lo[t1 - 1] + K.nsites[t1 - 1];
        r0 = r0 < 0 ? 0 : r0 > n ? n : r0; r1 = r1 > n ? n : r1;
        if(r1 > r0 + K.tile + 2 * K.cap) r1 = r0 + K.tile + 2 * K.cap;
        double M[SMO_BATCH], D[SMO_BATCH];
#pragma unroll
        for(int32_t b = 0; b < SMO_BATCH; b++) { M[b] = 0.0; D[b] = 0.0; }
        uint32_t err = 0; int64_t err_at = 0;
        for(int64_t cb = r0; cb < r1; cb += C) {
            const int64_t ce = cb + C < r1 ? cb + C : r1;
            __syncthreads();                                   // the chunk before is used up
            for(int64_t r = threadIdx.x; r < ce - cb; r += blockDim.x) {
                const int64_t j = cb + r;
                xs[r] = x[j];
                const bool own = j >= t0 && j < t1;
                for(int32_t b = 0; b < nb; b++) {
                    const int64_t at = (int64_t)(s0 + b) * n + j;
                    const int64_t m = (int64_t)Mg[at], u = (int64_t)Ug[at];
                    if(own) {
                        const uint32_t e = smo_entry_check(m) | smo_entry_check(u);
                        if(e && (!err || j < err_at)) { err = e; err_at = j; } else if(e && j == err_at) err |= e;
                    }
                    Ms[(size_t)b * C + r] = (double)m;
                    Ds[(size_t)b * C + r] = (double)(m + u);
                }
            }
            __syncthreads();
            if(active) {
                const int64_t jb = lo_i > cb ? lo_i : cb, je = hi_i < ce ? hi_i : ce;
                for(int64_t j = jb; j < je; j++) {
                    const int32_t r = (int32_t)(j - cb);
                    const int64_t dx = (int64_t)xs[r] - x_i;
                    const double w = smo_weight(K.kernel, dx < 0 ? -dx : dx, half_i, inv);
#pragma unroll
                    for(int32_t b = 0; b < SMO_BATCH; b++)
                        if(b < nb) smo_add(w, Ms[(size_t)b * C + r], Ds[(size_t)b * C + r], &M[b], &D[b]);
                }
            }
        }
        if(err) atomicMin(&K.st->first, (unsigned long long)smo_refusal_key(err_at, err));
        if(active) {
#pragma unroll
            for(int32_t b = 0; b < SMO_BATCH; b++)
                if(b < nb) {
                    const int64_t at = (int64_t)(s0 + b) * n + i;
                    K.level[at] = smo_level(M[b], D[b]); K.depth[at] = D[b];
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
#define SIDE_ERR_ARG MD_SMOOTH_ERR_ARG
#define SIDE_ERR_HIP MD_SMOOTH_ERR_HIP
#define SIDE_ERR_NOMEM MD_SMOOTH_ERR_NOMEM
#include "mdk_side.hpp"
extern "C" const char *md_smooth_last_error(void) { return g_err; }

struct md_smooth : SideHandle<SmoothStatus> {
    SideBuf<int32_t> d_lo;                                      // lo of every site: the window kernel's word to the sum kernel
    int32_t tile = SMO_TILE_DEFAULT, chunk = SMO_CHUNK_DEFAULT, batch = SMO_BATCH_DEFAULT, grid = SMO_GRID_DEFAULT;
};

static size_t smo_lds_bytes(int32_t chunk, int32_t batch) { return (size_t)chunk * (16u * (size_t)batch + 4u); }

extern "C" int md_smooth_open(int device, md_smooth **out) { return side_open(device, out, "md_smooth_open", md_smooth_close); }

extern "C" void md_smooth_close(md_smooth *h) {
    if(!h) return;
    h->close(); h->d_lo.release();
    delete h;
}

extern "C" int md_smooth_limits(md_smooth *h, int32_t tile_sites, int32_t chunk_sites, int32_t sample_batch, int32_t max_workgroups) {
    const char *const what = "md_smooth_limits";
    if(!h) return fail(MD_SMOOTH_ERR_ARG, what, hipSuccess);
    const int32_t tile = tile_sites ? tile_sites : SMO_TILE_DEFAULT, chunk = chunk_sites ? chunk_sites : SMO_CHUNK_DEFAULT;
    const int32_t batch = sample_batch ? sample_batch : SMO_BATCH_DEFAULT, grid = max_workgroups ? max_workgroups : SMO_GRID_DEFAULT;
    if(tile < 64 || tile > SMO_WG || tile % 64 || chunk < 64 || chunk > (1 << 20) || batch < 1 || batch > SMO_BATCH || grid < 1 || smo_lds_bytes(chunk, batch) > SMO_LDS_BYTES) {
        snprintf(g_err, sizeof g_err, "%s: tile_sites a multiple of 64 up to %d, chunk_sites at least 64, sample_batch 1 to %d, chunk_sites * (16 * sample_batch + 4) at most %d bytes, max_workgroups above 0",
                 what, SMO_WG, SMO_BATCH, SMO_LDS_BYTES);
        return MD_SMOOTH_ERR_ARG;
    }
    h->tile = tile; h->chunk = chunk; h->batch = batch; h->grid = grid;
    return 0;
}

// the kernels' arguments under the handle's blocking, and the two launches (tools/smooth_bench.hip times them one by one)
static KSmooth smo_arguments(const md_smooth *h, const int32_t *contig, const int32_t *start, const void *nmeth, const void *nunmeth, int32_t n_samples, int64_t n,
                             int32_t half_bases, int32_t min_sites, int32_t kernel, double *level, double *depth, int32_t *nsites, int32_t *half) {
    KSmooth K;
    K.contig = contig; K.start = start; K.m = nmeth; K.u = nunmeth; K.S = n_samples; K.n = n;
    K.half_bases = half_bases; K.min_sites = min_sites; K.kernel = kernel;
    K.level = level; K.depth = depth; K.nsites = nsites; K.half = half; K.lo = h->d_lo;
    K.tile = h->tile; K.chunk = h->chunk; K.batch = n_samples < h->batch ? n_samples : h->batch;          // (LDS for the samples there are: more workgroups a CU)
    K.items = ((n + K.tile - 1) / K.tile) * ((n_samples + K.batch - 1) / K.batch);
    K.cap = smo_window_cap(half_bases, min_sites); K.st = h->d_st;
    return K;
}
static void smo_launch_window(const md_smooth *h, const KSmooth &K) {
    hipLaunchKernelGGL(k_smooth_window, dim3((uint32_t)((K.n + SMO_WG - 1) / SMO_WG)), dim3(SMO_WG), 0, h->st, K);
}
static void smo_launch_sum(const md_smooth *h, const KSmooth &K, int elem_bytes) {
    const dim3 grid((uint32_t)(K.items < h->grid ? K.items : h->grid));
    const size_t lds = smo_lds_bytes(K.chunk, K.batch);
    if(elem_bytes == 4) hipLaunchKernelGGL(k_smooth_sum<int32_t>, grid, dim3(h->tile), lds, h->st, K);
    else hipLaunchKernelGGL(k_smooth_sum<int64_t>, grid, dim3(h->tile), lds, h->st, K);
}

extern "C" int md_smooth_run(md_smooth *h, const int32_t *contig, const int32_t *start, const void *nmeth, const void *nunmeth, int elem_bytes,
                             int32_t n_samples, int64_t n, int32_t half_bases, int32_t min_sites, int32_t kernel,
                             double *level, double *depth, int32_t *nsites, int32_t *half) {
    const char *const what = "md_smooth_run";
    if(!h || (elem_bytes != 4 && elem_bytes != 8) || n_samples < 1 || n_samples > SMO_MAX_SAMPLES || n < 0 || n > SMO_MAX_SITES)
        return fail(MD_SMOOTH_ERR_ARG, what, hipSuccess);
    if(n && (!contig || !start || !nmeth || !nunmeth || !level || !depth || !nsites || !half)) return fail(MD_SMOOTH_ERR_ARG, what, hipSuccess);
    if(half_bases < 0 || half_bases > SMO_MAX_HALF_BASES || min_sites < 1 || min_sites > SMO_MAX_MIN_SITES || (kernel != SMO_TRICUBE && kernel != SMO_FLAT)) {
        snprintf(g_err, sizeof g_err, "%s: half_bases within 0 and 2^20, min_sites within 1 and 2^16, kernel 0 (tricube) or 1 (flat)", what);
        return MD_SMOOTH_ERR_ARG;
    }
    if(!n) return 0;
    SIDECHK(hipSetDevice(h->device));
    if(int rc = h->d_lo.need((size_t)n, "md_smooth_run: the windows' scratch")) return rc;
    SIDE_STATUS_UP(h, h->pin, SmoothStatus);
    const KSmooth K = smo_arguments(h, contig, start, nmeth, nunmeth, n_samples, n, half_bases, min_sites, kernel, level, depth, nsites, half);
    smo_launch_window(h, K);
    SIDECHK(hipGetLastError());
    smo_launch_sum(h, K, elem_bytes);
    SIDECHK(hipGetLastError());
    SIDE_STATUS_DOWN(h, h->pin, SmoothStatus);
    const unsigned long long first = h->pin->first;
    if(first == ~0ull) return 0;
    const uint32_t bit = 1u << (first & 0xffu);
    snprintf(g_err, sizeof g_err, "%s: %s (site %lld)", what,
             bit == SMO_E_ORDER ? "a row is not strictly ascending in (contig, start) behind its predecessor" :
             bit == SMO_E_POSITION ? "a contig or a start is negative" :
             bit == SMO_E_NEGATIVE ? "a count is negative" : "a count is 2^26 or more",
             (long long)(first >> 8));
    return MD_SMOOTH_ERR_ARG;
}
