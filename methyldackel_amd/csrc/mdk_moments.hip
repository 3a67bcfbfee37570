// mdk_moments.hip -- the pairwise sample moments of two [S, n] count matrices and their centring (include/mdk_moments.h: md_stats_moments,
// md_stats_center, md_stats_moments_limits).  The rule is mdk_moments_core.h's.  Part of libmdk_stats.so: mdk_qdiff.hip includes this
// file below its own host side, so the calls live on the md_stats handle, its stream, its status word and its error text.
//
// The work grows with S^2 n.  It is cut into ITEMS: an item is a block of the [S, S] matrices -- a band of rows I and a band of columns J,
// every ordered pair of bands, so a cell of the result has one owner and no symmetry is relied on -- times a range of sites.  A workgroup
// (256 lanes) takes items blockIdx.x, blockIdx.x + gridDim.x, ...; it sums an item on chip and adds the item's block to the four matrices
// with one 64-bit integer atomic add per cell and matrix.  Integer sums commute: the matrices do not depend on the items, their order or
// the grid.  A cell of the tables is quantised by mom_cell into one 32-bit word, level and covered bit; an uncovered, refused or absent
// (past S, past the range) cell is the word 0, which adds nothing to any sum, so the inner loops have no branch.
// Two shapes, because the parallelism flips with S:
//   k_mom_lanes<T, t>   a band is t samples (t = 1, 2, 4).  A lane per site, striding the range by 256: the 2 t cells of the site read
//                       coalesced along n and quantised (t where I = J), the t x t pairs accumulated in registers -- n in 32 bits, sx, sxx
//                       and sxy in 64 --, then a wavefront reduction by shuffles, the four wavefronts through 2 KiB of LDS, and the
//                       atomic adds by the first 4 t^2 lanes.  At S <= 4 a site's cells are read and divided once.
//   k_mom_staged<T, t>  a band is 16 t samples.  The workgroup stages a chunk of sites x the two bands in LDS (one band where I = J) as
//                       32-bit words -- 65536 does not fit 16 bits --, site-major with a row of 16 t + 4 words: a lane (li, lj) of the
//                       16 x 16 owns the t x t pairs of rows li t.., columns lj t.. and reads its 2 t words of a site as two vectors,
//                       the 16 columns of a wavefront on different banks.  It walks the chunk with v_mad_u64_u32, keeps its sums over
//                       the whole range and flushes them itself.  The division is once per cell and band pair, not per pair.  (The
//                       three large sums as doubles, one exact v_fma_f64 each, were built and measured: slower)
// What is flushed, 32 bytes per pair, is a small part of what an item reads: the default range is at least 8192 sites for k_mom_lanes
// (512 bytes against 256 KiB) and 2048 for k_mom_staged (128 KiB against 2 MiB at t = 4).
//   k_mom_center        a lane per ordered pair: mom_sums_check, then mom_cxy and mom_vxx.
// A refusal goes into the status word by atomicMin as in k_qdiff.  Vector loads, stores and atomics, plain C++.
#include "mdk_moments_core.h"

#define MOM_WG 256
#define MOM_GRID_DEFAULT 2048
#define MOM_LANES_RANGE 8192              // the least sites of an item by default: k_mom_lanes
#define MOM_STAGED_RANGE 2048             // ... k_mom_staged
#define MOM_LANES_MAX_S 8                 // the default shape: k_mom_lanes up to here (measured: DESIGN.md section 4)
#define MOM_LDS_BYTES 65536
enum { MOM_SHAPE_AUTO = 0, MOM_SHAPE_LANES = 1, MOM_SHAPE_STAGED = 2 };

struct KMom {
    const void *m, *u; int32_t S; int64_t n, min_depth;
    int32_t nbands; int64_t nranges, range, items; int32_t chunk;      // bands of a side, ranges of sites, the sites of a range; a staged chunk
    unsigned long long *on, *osx, *osxx, *osxy;
    StatsStatus *st;
};

// one site's words of band I (wi) and band J (wj) into the t x t sums
template <int t>
__device__ __forceinline__ void mom_add(const uint32_t (&wi)[t], const uint32_t (&wj)[t], uint32_t (&cn)[t][t], uint64_t (&sx)[t][t], uint64_t (&sxx)[t][t], uint64_t (&sxy)[t][t]) {
#pragma unroll
    for(int a = 0; a < t; a++) {
        const uint32_t xi = wi[a] & MOM_LEVEL_MASK, ci = wi[a] >> MOM_COVERED_BIT;
#pragma unroll
        for(int b = 0; b < t; b++) {
            const uint32_t xj = wj[b] & MOM_LEVEL_MASK, cj = wj[b] >> MOM_COVERED_BIT;
            const uint32_t xm = cj ? xi : 0u;                      // x_i where j is covered too (x_i is 0 where i is not)
            cn[a][b] += ci & cj;
            sx[a][b] += xm;
            sxx[a][b] += (uint64_t)xm * xi;
            sxy[a][b] += (uint64_t)xi * xj;
        }
    }
}

template <typename T, int t>
__global__ __launch_bounds__(MOM_WG) void k_mom_lanes(const KMom K) {
    __shared__ unsigned long long part[MOM_WG / 64][4 * t * t];
    const T *const __restrict__ M = (const T *)K.m, *const __restrict__ U = (const T *)K.u;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long first = ~0ull;
    for(int64_t item = blockIdx.x; item < K.items; item += gridDim.x) {
        const int64_t bp = item / K.nranges, r = item - bp * K.nranges;
        const int32_t I0 = (int32_t)(bp / K.nbands) * t, J0 = (int32_t)(bp % K.nbands) * t;
        const int64_t k0 = r * K.range, k1 = k0 + K.range < K.n ? k0 + K.range : K.n;
        uint32_t cn[t][t]; uint64_t sx[t][t], sxx[t][t], sxy[t][t];
#pragma unroll
        for(int a = 0; a < t; a++)
#pragma unroll
            for(int b = 0; b < t; b++) { cn[a][b] = 0; sx[a][b] = 0; sxx[a][b] = 0; sxy[a][b] = 0; }
        for(int64_t k = k0 + threadIdx.x; k < k1; k += MOM_WG) {
            uint32_t wi[t], wj[t], e = 0;
#pragma unroll
            for(int a = 0; a < t; a++) {
                const int64_t at = (int64_t)(I0 + a) * K.n + k;
                wi[a] = I0 + a < K.S ? mom_cell((int64_t)M[at], (int64_t)U[at], K.min_depth, &e) : 0u;
            }
#pragma unroll
            for(int b = 0; b < t; b++) {
                const int64_t at = (int64_t)(J0 + b) * K.n + k;
                wj[b] = J0 == I0 ? wi[b] : J0 + b < K.S ? mom_cell((int64_t)M[at], (int64_t)U[at], K.min_depth, &e) : 0u;
            }
            if(e) { const unsigned long long key = mom_refusal_key(k, e); first = key < first ? key : first; }
            mom_add<t>(wi, wj, cn, sx, sxx, sxy);
        }
        // the wavefront's sums on its lane 0, the four wavefronts' in LDS, one atomic add per cell and matrix
#pragma unroll
        for(int a = 0; a < t; a++)
#pragma unroll
            for(int b = 0; b < t; b++) {
                unsigned long long v[4] = { cn[a][b], sx[a][b], sxx[a][b], sxy[a][b] };
#pragma unroll
                for(int q = 0; q < 4; q++) {
#pragma unroll
                    for(int off = 32; off; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
                    if(lane == 0) part[wave][q * t * t + a * t + b] = v[q];
                }
            }
        __syncthreads();
        if(threadIdx.x < 4 * t * t) {
            unsigned long long v = 0;
#pragma unroll
            for(int w = 0; w < MOM_WG / 64; w++) v += part[w][threadIdx.x];
            const int q = threadIdx.x / (t * t), ab = threadIdx.x % (t * t), i = I0 + ab / t, j = J0 + ab % t;
            if(v && i < K.S && j < K.S) atomicAdd((q == 0 ? K.on : q == 1 ? K.osx : q == 2 ? K.osxx : K.osxy) + (int64_t)i * K.S + j, v);
        }
        __syncthreads();                                           // (part is written again by the next item)
    }
    if(first != ~0ull) atomicMin(&K.st->first, first);
}

extern __shared__ __align__(16) uint32_t mom_lds[];
template <typename T, int t>
__global__ __launch_bounds__(MOM_WG) void k_mom_staged(const KMom K) {
    constexpr int band = 16 * t, stride = band + 4;                // (words; + 4: the rows stay 16-byte aligned and a wavefront's 16 columns leave each other's banks)
    const T *const __restrict__ M = (const T *)K.m, *const __restrict__ U = (const T *)K.u;
    const int li = threadIdx.x >> 4, lj = threadIdx.x & 15;
    unsigned long long first = ~0ull;
    for(int64_t item = blockIdx.x; item < K.items; item += gridDim.x) {
        const int64_t bp = item / K.nranges, r = item - bp * K.nranges;
        const int32_t I0 = (int32_t)(bp / K.nbands) * band, J0 = (int32_t)(bp % K.nbands) * band;
        const int64_t k0 = r * K.range, k1 = k0 + K.range < K.n ? k0 + K.range : K.n;
        uint32_t *const xsI = mom_lds, *const xsJ = J0 == I0 ? mom_lds : mom_lds + (size_t)K.chunk * stride;
        uint32_t cn[t][t]; uint64_t sx[t][t], sxx[t][t], sxy[t][t];
#pragma unroll
        for(int a = 0; a < t; a++)
#pragma unroll
            for(int b = 0; b < t; b++) { cn[a][b] = 0; sx[a][b] = 0; sxx[a][b] = 0; sxy[a][b] = 0; }
        for(int64_t c0 = k0; c0 < k1; c0 += K.chunk) {
            const int32_t rows = k1 - c0 < K.chunk ? (int32_t)(k1 - c0) : K.chunk;
            __syncthreads();                                       // (the chunk before is walked)
            for(int32_t x = threadIdx.x; x < band * K.chunk; x += MOM_WG) {          // staged: a sample's sites are neighbouring lanes'
                const int32_t s = x / K.chunk, kk = x - s * K.chunk;
                uint32_t e = 0, wI = 0, wJ = 0;
                if(kk < rows) {
                    if(I0 + s < K.S) { const int64_t at = (int64_t)(I0 + s) * K.n + c0 + kk; wI = mom_cell((int64_t)M[at], (int64_t)U[at], K.min_depth, &e); }
                    if(J0 != I0 && J0 + s < K.S) { const int64_t at = (int64_t)(J0 + s) * K.n + c0 + kk; wJ = mom_cell((int64_t)M[at], (int64_t)U[at], K.min_depth, &e); }
                    if(e) { const unsigned long long key = mom_refusal_key(c0 + kk, e); first = key < first ? key : first; }
                }
                xsI[kk * stride + s] = wI;
                if(J0 != I0) xsJ[kk * stride + s] = wJ;
            }
            __syncthreads();
            for(int32_t kk = 0; kk < rows; kk++) {
                uint32_t wi[t], wj[t];
                if constexpr(t == 4) {
                    const uint4 vi = *(const uint4 *)&xsI[kk * stride + li * 4], vj = *(const uint4 *)&xsJ[kk * stride + lj * 4];
                    wi[0] = vi.x; wi[1] = vi.y; wi[2] = vi.z; wi[3] = vi.w; wj[0] = vj.x; wj[1] = vj.y; wj[2] = vj.z; wj[3] = vj.w;
                } else {
#pragma unroll
                    for(int a = 0; a < t; a++) { wi[a] = xsI[kk * stride + li * t + a]; wj[a] = xsJ[kk * stride + lj * t + a]; }
                }
                mom_add<t>(wi, wj, cn, sx, sxx, sxy);
            }
        }
#pragma unroll
        for(int a = 0; a < t; a++)
#pragma unroll
            for(int b = 0; b < t; b++) {
                const int32_t i = I0 + li * t + a, j = J0 + lj * t + b;
                if(i < K.S && j < K.S) {
                    const int64_t at = (int64_t)i * K.S + j;
                    if(cn[a][b]) atomicAdd(K.on + at, (unsigned long long)cn[a][b]);
                    if(sx[a][b]) atomicAdd(K.osx + at, (unsigned long long)sx[a][b]);
                    if(sxx[a][b]) atomicAdd(K.osxx + at, (unsigned long long)sxx[a][b]);
                    if(sxy[a][b]) atomicAdd(K.osxy + at, (unsigned long long)sxy[a][b]);
                }
            }
    }
    if(first != ~0ull) atomicMin(&K.st->first, first);
}

struct KMomCenter { const int64_t *n, *sx, *sxx, *sxy; int32_t S; double *cxy, *vxx; StatsStatus *st; };
__global__ __launch_bounds__(MOM_WG) void k_mom_center(const KMomCenter K) {
    const int32_t at = blockIdx.x * MOM_WG + threadIdx.x;
    if(at >= K.S * K.S) return;
    const int32_t i = at / K.S, j = at - i * K.S;
    const int64_t n = K.n[at], sx = K.sx[at], sxx = K.sxx[at], sxy = K.sxy[at], sx_t = K.sx[j * K.S + i];
    const uint32_t err = mom_sums_check(n, sx, sxx, sxy);
    if(err) {                                                      // (a refused cell is not centred: the products may pass 128 bits)
        atomicMin(&K.st->first, (unsigned long long)mom_refusal_key(at, err));
        K.cxy[at] = 0.0; K.vxx[at] = 0.0;
        return;
    }
    // (the transposed cell is checked by its own lane; where it is refused the call fails, and this product still fits: |sx_t| < 2^63, sx <= 2^46)
    K.cxy[at] = mom_cxy(n, sxy, sx, sx_t);
    K.vxx[at] = mom_vxx(n, sxx, sx);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// the sites of a staged chunk that fit the LDS at pair tile t: two bands of 16 t + 4 words a site
static int32_t mom_chunk_cap(int32_t t) { const int32_t c = MOM_LDS_BYTES / (2 * (16 * t + 4) * 4) / 64 * 64; return c < 256 ? c : 256; }

extern "C" int md_stats_moments_limits(md_stats *h, int32_t shape, int32_t chunk_sites, int32_t pair_tile, int32_t max_workgroups) {
    const char *const what = "md_stats_moments_limits";
    if(!h) return fail(MD_STATS_ERR_ARG, what, hipSuccess);
    const bool tile_ok = pair_tile == 0 || pair_tile == 1 || pair_tile == 2 || pair_tile == 4;
    if(shape < MOM_SHAPE_AUTO || shape > MOM_SHAPE_STAGED || !tile_ok || chunk_sites < 0 || chunk_sites % 64 || chunk_sites > mom_chunk_cap(pair_tile ? pair_tile : 4) || max_workgroups < 0) {
        snprintf(g_err, sizeof g_err, "%s: shape 0 (by S), 1 (a lane per site) or 2 (staged in LDS), chunk_sites a multiple of 64 up to 256 (64 at pair_tile 4 or 0, 192 at 2), pair_tile 0, 1, 2 or 4, max_workgroups 0 or more", what);
        return MD_STATS_ERR_ARG;
    }
    h->mom_shape = shape; h->mom_chunk = chunk_sites; h->mom_tile = pair_tile; h->mom_grid = max_workgroups;
    return 0;
}

// what a call launches at these limits: the kernel's arguments without its pointers
struct MomPlan { int32_t shape, t, grid; size_t lds; };
static MomPlan mom_plan(const md_stats *h, int32_t S, int64_t n, KMom *K) {
    MomPlan p;
    p.shape = h->mom_shape ? h->mom_shape : S <= MOM_LANES_MAX_S ? MOM_SHAPE_LANES : MOM_SHAPE_STAGED;
    if(p.shape == MOM_SHAPE_LANES) p.t = h->mom_tile ? h->mom_tile : S >= 3 ? 4 : S;
    else p.t = h->mom_tile ? h->mom_tile : S <= 16 ? 1 : S <= 32 ? 2 : 4;
    const int32_t band = p.shape == MOM_SHAPE_LANES ? p.t : 16 * p.t;
    K->S = S; K->n = n;
    K->nbands = (S + band - 1) / band;
    K->chunk = h->mom_chunk ? h->mom_chunk : p.shape == MOM_SHAPE_LANES ? 256 : mom_chunk_cap(p.t);
    const int64_t pairs = (int64_t)K->nbands * K->nbands, wanted = MOM_GRID_DEFAULT / pairs > 0 ? MOM_GRID_DEFAULT / pairs : 1;
    const int64_t least = h->mom_chunk ? h->mom_chunk : p.shape == MOM_SHAPE_LANES ? MOM_LANES_RANGE : MOM_STAGED_RANGE;
    K->range = (n + wanted - 1) / wanted;
    if(K->range < least) K->range = least;
    K->nranges = (n + K->range - 1) / K->range;
    K->items = pairs * K->nranges;
    const int64_t most = h->mom_grid ? h->mom_grid : MOM_GRID_DEFAULT;
    p.grid = (int32_t)(K->items < most ? K->items : most);
    p.lds = p.shape == MOM_SHAPE_STAGED ? (size_t)K->chunk * 2 * (16 * p.t + 4) * 4 : 0;
    return p;
}

template <typename T> static void mom_launch_as(const md_stats *h, const MomPlan &p, const KMom &K) {
    const dim3 grid(p.grid), wg(MOM_WG);
    if(p.shape == MOM_SHAPE_LANES) {
        if(p.t == 1) hipLaunchKernelGGL((k_mom_lanes<T, 1>), grid, wg, 0, h->st, K);
        else if(p.t == 2) hipLaunchKernelGGL((k_mom_lanes<T, 2>), grid, wg, 0, h->st, K);
        else hipLaunchKernelGGL((k_mom_lanes<T, 4>), grid, wg, 0, h->st, K);
    } else {
        if(p.t == 1) hipLaunchKernelGGL((k_mom_staged<T, 1>), grid, wg, p.lds, h->st, K);
        else if(p.t == 2) hipLaunchKernelGGL((k_mom_staged<T, 2>), grid, wg, p.lds, h->st, K);
        else hipLaunchKernelGGL((k_mom_staged<T, 4>), grid, wg, p.lds, h->st, K);
    }
}
static void mom_launch(const md_stats *h, const MomPlan &p, const KMom &K, int elem_bytes) {
    if(elem_bytes == 4) mom_launch_as<int32_t>(h, p, K); else mom_launch_as<int64_t>(h, p, K);
}

extern "C" int md_stats_moments(md_stats *h, const void *nmeth, const void *nunmeth, int elem_bytes, int32_t n_samples, int64_t n, int64_t min_depth,
                                int64_t *n_out, int64_t *sx_out, int64_t *sxx_out, int64_t *sxy_out) {
    const char *const what = "md_stats_moments";
    if(!h || (elem_bytes != 4 && elem_bytes != 8) || n_samples < 1 || n_samples > MOM_MAX_SAMPLES || n < 0 || n > MOM_MAX_SITES || !n_out || !sx_out || !sxx_out || !sxy_out)
        return fail(MD_STATS_ERR_ARG, what, hipSuccess);
    if(n && (!nmeth || !nunmeth)) return fail(MD_STATS_ERR_ARG, what, hipSuccess);
    if(min_depth < 1 || min_depth >= MOM_LIMIT) {
        snprintf(g_err, sizeof g_err, "%s: min_depth must be within 1 and 2^26 - 1", what);
        return MD_STATS_ERR_ARG;
    }
    SIDECHK(hipSetDevice(h->device));
    const size_t bytes = (size_t)n_samples * n_samples * sizeof(int64_t);
    SIDECHK(hipMemsetAsync(n_out, 0, bytes, h->st)); SIDECHK(hipMemsetAsync(sx_out, 0, bytes, h->st));
    SIDECHK(hipMemsetAsync(sxx_out, 0, bytes, h->st)); SIDECHK(hipMemsetAsync(sxy_out, 0, bytes, h->st));
    if(!n) { SIDECHK(hipStreamSynchronize(h->st)); return 0; }
    SIDE_STATUS_UP(h, &h->pin->st, StatsStatus);
    KMom K;
    K.m = nmeth; K.u = nunmeth; K.min_depth = min_depth; K.st = h->d_st;
    K.on = (unsigned long long *)n_out; K.osx = (unsigned long long *)sx_out; K.osxx = (unsigned long long *)sxx_out; K.osxy = (unsigned long long *)sxy_out;
    const MomPlan p = mom_plan(h, n_samples, n, &K);
    mom_launch(h, p, K, elem_bytes);
    SIDECHK(hipGetLastError());
    SIDE_STATUS_DOWN(h, &h->pin->st, StatsStatus);
    const unsigned long long first = h->pin->st.first;
    if(first == ~0ull) return 0;
    snprintf(g_err, sizeof g_err, "%s: %s (site %lld)", what, (1u << (first & 0xffu)) == MOM_E_NEGATIVE ? "a count is negative" : "a count is 2^26 or more", (long long)(first >> 8));
    return MD_STATS_ERR_ARG;
}

extern "C" int md_stats_center(md_stats *h, const int64_t *n_in, const int64_t *sx_in, const int64_t *sxx_in, const int64_t *sxy_in, int32_t n_samples,
                               double *cxy_out, double *vxx_out) {
    const char *const what = "md_stats_center";
    if(!h || !n_in || !sx_in || !sxx_in || !sxy_in || n_samples < 1 || n_samples > MOM_MAX_SAMPLES || !cxy_out || !vxx_out) return fail(MD_STATS_ERR_ARG, what, hipSuccess);
    SIDECHK(hipSetDevice(h->device));
    SIDE_STATUS_UP(h, &h->pin->st, StatsStatus);
    KMomCenter K;
    K.n = n_in; K.sx = sx_in; K.sxx = sxx_in; K.sxy = sxy_in; K.S = n_samples; K.cxy = cxy_out; K.vxx = vxx_out; K.st = h->d_st;
    hipLaunchKernelGGL(k_mom_center, dim3((uint32_t)((n_samples * n_samples + MOM_WG - 1) / MOM_WG)), dim3(MOM_WG), 0, h->st, K);
    SIDECHK(hipGetLastError());
    SIDE_STATUS_DOWN(h, &h->pin->st, StatsStatus);
    const unsigned long long first = h->pin->st.first;
    if(first == ~0ull) return 0;
    const uint32_t bit = 1u << (first & 0xffu);
    const long long cell = (long long)(first >> 8);
    snprintf(g_err, sizeof g_err, "%s: %s (cell %lld, %lld)", what,
             bit == MOM_E_SUM_NEGATIVE ? "a sum is negative" : bit == MOM_E_SUM_N ? "n is more than 2^30" :
             bit == MOM_E_SUM_SX ? "sx is more than n * 65536" : "sxx or sxy is more than n * 2^32", cell / n_samples, cell % n_samples);
    return MD_STATS_ERR_ARG;
}
